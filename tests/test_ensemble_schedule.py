"""Process schedules and probe histories of ThermoViscoEnsemble, the CG1 reference cell
(csrc/tv_ensemble.hip, k_ensemble<true, 0>): against the CPU oracle, whose ThermalParams
object is set to the step's stage before each solve_timestep(); against the unscheduled
kernel (a schedule that changes nothing, a stage change as a restart); against itself
(splits, independence of the bars); and the records against get_field of a twin ensemble.
The checks are those of every cell (tests/ensemble_parity.py, tests/ensemble_contract.py;
tolerances: tests/ensemble_cases.py).
"""
import pytest

import ensemble_contract as contract
import ensemble_parity as parity
from ensemble_cases import CELL

pytestmark = pytest.mark.gpu

C = CELL["cg-reference"]


@pytest.mark.parametrize("n_cells", [1, 2, 3, 16])
def test_parity_with_oracle(n_cells):
    parity.schedule_parity_with_oracle(C, n_cells)


def test_schedule_that_changes_nothing_changes_no_bit():
    contract.schedule_that_changes_nothing_changes_no_bit(C)


@pytest.mark.parametrize("n_cells", [3, 16])
def test_stage_change_is_a_restart(n_cells):
    contract.stage_change_is_a_restart(C, n_cells)


def test_independence_and_splits():
    contract.scheduled_independence_and_splits(C)


@pytest.mark.parametrize("n_cells", [1, 16])
def test_history(n_cells):
    contract.history(C, n_cells)


def test_history_and_a_failed_bar():
    contract.history_and_a_failed_bar(C)


def test_history_capacity():
    contract.history_capacity(C)
