"""Red zones around the run-history kernels of csrc/tv_history.hip (k_history_map, k_history_gather,
k_history_extrema, k_history_finish), the scheme of tests/test_guard_bands_problem_exact.py: each history
case of tests/problem_schedule_cases.py (3d_cg: d*d = 9 stress streams; 2d_dg_cg: mixed dof maps) runs its
six scheduled steps in a context created with TVFEM_ALLOC_GUARD, so that the record buffer, the extrema
pass's partial pairs and the probe table each lie between two filled guards.  Every guard of the library's
allocations must still hold its fill (0 damaged: no out-of-bounds write), and the records must hold the
same bits as in a plain run: the kernels are deterministic and the runs differ only in addresses and in
what lies outside the vectors, so a difference is an out-of-bounds read.  (The guards of vectors of doubles
are NaNs, which the extrema skip: an over-read of a stream's end by the extrema pass would not show in its
result.  Its loop bounds are the owned range; the probe values read single, range-checked dofs.)
"""
import pytest

from guard_util import assert_guards_intact, guard_env, plain_env
from problem_schedule_cases import HISTORY_CASES, gpu, history_case, same_bits

pytestmark = pytest.mark.gpu


def _run(name, finish):
    p, lib, (h, dofs, its) = history_case(name)
    finish(lib)
    p.close()
    return h, dofs, its


@pytest.mark.parametrize("name", list(HISTORY_CASES))
def test_history_kernels_stay_inside_their_allocations(name, monkeypatch):
    gpu()
    guard_env(monkeypatch)
    got, dofs, its = _run(name, assert_guards_intact)
    plain_env(monkeypatch)
    plain, dofs_plain, its_plain = _run(name, lambda lib: None)
    assert its == its_plain
    for k in ("T", "sigma"):
        assert dofs[k].tolist() == dofs_plain[k].tolist()
    assert got.keys() == plain.keys()
    for k in got:
        assert same_bits(got[k], plain[k]), f"{k}: guarded and plain run differ: an out-of-bounds read"
    assert got["step"].tolist() == [2, 4, 6]
