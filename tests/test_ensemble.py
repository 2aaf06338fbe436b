"""ThermoViscoEnsemble, the CG1 reference cell (csrc/tv_ensemble.hip, k_ensemble<false, 0>):
against the CPU oracle bar by bar, against itself, against the single-bar device path, and
the failure contract.  The checks are those of every cell (tests/ensemble_parity.py,
tests/ensemble_contract.py; tolerances: tests/ensemble_cases.py); schedules and histories of
this cell are tests/test_ensemble_schedule.py.
"""
import pytest

import ensemble_contract as contract
import ensemble_parity as parity
from ensemble_cases import CELL

pytestmark = pytest.mark.gpu

C = CELL["cg-reference"]


@pytest.mark.parametrize("n_cells", [1, 2, 3, 16])
def test_parity_with_oracle(n_cells):
    parity.parity_with_oracle(C, n_cells)


def test_independence_and_padding():
    contract.independence_padding_and_split(C)


def test_long_horizon():
    parity.long_horizon(C)


def test_against_single_bar_path():
    parity.against_single_bar_path(C)


@pytest.mark.parametrize("error_on_nonconvergence", [True, False])
def test_failure_semantics(error_on_nonconvergence):
    contract.failure_semantics(C, error_on_nonconvergence)


def test_thermal_only():
    contract.thermal_only(C)


@pytest.mark.parametrize("n_cells", [1, 5])
def test_field_shapes(n_cells):
    contract.field_shapes(C, n_cells)
