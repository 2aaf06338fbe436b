"""Red zones around the paper-mode ensemble kernels (the kModel = 1 instantiations of
csrc/tv_ensemble.hip and csrc/tv_ensemble_dg.hip): the scheme and the
case of tests/test_guard_bands.py (its ensemble_cell, imported), the cells of
tests/ensemble_cases.py.  Each case runs the same calls twice, with TVFEM_ALLOC_GUARD and
plain, and asserts intact guards, the same bits in both runs and the guarded T against the
oracle (1e-10); 65 and 130 bars put tail lanes, a second wave and a second workgroup next to
the guards.
"""
import pytest

from ensemble_cases import CELL
from test_guard_bands import ensemble_cell

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n_cells", [1, 3, 16])
@pytest.mark.parametrize("n_bars", [1, 65, 130])
@pytest.mark.parametrize("fam", ["cg", "dg"])
def test_ensemble_paper(fam, n_bars, n_cells, monkeypatch):
    ensemble_cell(CELL[fam + "-paper"], n_bars, n_cells, monkeypatch)
