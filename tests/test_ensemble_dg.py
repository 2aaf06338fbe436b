"""ThermoViscoEnsemble, the DG1 reference cell: DG1 temperature and CG1 stress
(csrc/tv_ensemble_dg.hip, k_ensemble_dg<kExt, 0>; main.py's own fe_config): against the CPU
oracle bar by bar, against the golden DG / CG fixture (10:1 jumps in h, where the '+' side
of the SIPG penalty matters), against itself, against the single-bar device path, the failure
contract, schedules and histories, and the shapes of the two field families.  The checks are
those of every cell (tests/ensemble_parity.py, tests/ensemble_contract.py; tolerances:
tests/ensemble_cases.py).
"""
import pytest

import ensemble_contract as contract
import ensemble_parity as parity
from ensemble_cases import CELL

pytestmark = pytest.mark.gpu

C = CELL["dg-reference"]


@pytest.mark.parametrize("n_cells", [1, 2, 3, 16])
def test_parity_with_oracle(n_cells):
    parity.parity_with_oracle(C, n_cells)


@pytest.mark.parametrize("copies", [1, 3])
def test_golden_fixture(copies):
    parity.golden_fixture(copies)


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


@pytest.mark.parametrize("n_cells", [1, 3, 16])
def test_schedule_parity_with_oracle(n_cells):
    parity.schedule_parity_with_oracle(C, n_cells)


def test_schedule_that_changes_nothing_changes_no_bit():
    contract.schedule_that_changes_nothing_changes_no_bit(C)


@pytest.mark.parametrize("n_cells", [3, 16])
def test_stage_change_is_a_restart(n_cells):
    contract.stage_change_is_a_restart(C, n_cells)


def test_scheduled_split():
    """And every scheduled bar the same bits alone and in padding lanes."""
    contract.scheduled_independence_and_splits(C)


@pytest.mark.parametrize("n_cells", [1, 16])
def test_history(n_cells):
    contract.history(C, n_cells)


def test_history_and_a_failed_bar():
    contract.history_and_a_failed_bar(C)


def test_history_capacity():
    contract.history_capacity(C)


@pytest.mark.parametrize("n_cells", [1, 5])
def test_field_shapes(n_cells):
    contract.field_shapes(C, n_cells)
