"""Red zones around the exact-relaxation kernels of csrc/tv_visco.hip (k_visco_fused_exact,
k_visco_S_exact), the scheme of tests/test_guard_bands.py: each case runs an exact ThermoViscoProblem of
tests/problem_exact_cases.py (T_0 = 920 K) for 3 steps in a context created with TVFEM_ALLOC_GUARD, asserts
that every guard of the library's allocations still holds its fill, and then that every readable field holds
the same bits as in a plain run (the kernels are deterministic; the runs differ only in addresses and in what
lies outside the vectors, so a difference is an out-of-bounds read).  1d_dg_cg and 2d_cg_dg: the T pass and
the sigma pass in both directions; 3d_cg: the fused kernel, one full workgroup and a tail.
"""
import numpy as np
import pytest

from guard_util import assert_guards_intact, guard_env, plain_env
from problem_exact_cases import gpu, problem, same_bits

pytestmark = pytest.mark.gpu


def _run(name, materialize, finish):
    from tvfem._native import FIELDS, NativeError
    p = problem(name, materialize=materialize)
    p.setup()
    for _ in range(3):
        p.solve_timestep()
    out = {}
    for f in FIELDS:
        try:
            out[f] = np.array(p.get_field(f))
        except NativeError:  # not materialised in the lean layout
            pass
    finish(p._lib)
    p.close()
    return out


@pytest.mark.parametrize("materialize", [True, False], ids=["materialized", "lean"])
@pytest.mark.parametrize("name", ["1d_dg_cg", "2d_cg_dg", "3d_cg"])
def test_exact_problem(name, materialize, monkeypatch):
    gpu()
    guard_env(monkeypatch)
    got = _run(name, materialize, assert_guards_intact)
    plain_env(monkeypatch)
    plain = _run(name, materialize, lambda lib: None)
    assert got.keys() == plain.keys()
    assert {"T", "T_prev", "Tf", "Tf_partial", "phi", "xi", "sigma", "s_partial", "sigma_partial",
            "s_tilde_partial", "sigma_tilde_partial"} <= got.keys()
    for k in got:
        assert same_bits(got[k], plain[k]), f"{k}: guarded and plain run differ: an out-of-bounds read"
    assert np.all(np.isfinite(got["sigma"]))
