"""ThermoViscoEnsemble(model_mode="paper"), the two paper cells: the paper-correct
viscoelastic model in both bar kernels (the kModel = 1 instantiations of
csrc/tv_ensemble_step.h), CG1 / CG1 and DG1 / CG1: against the CPU oracle's paper mode bar
by bar, against the reference-mode ensemble (the thermal problem does not see the mode),
against itself, against the single-bar device path, the failure contract, thermal-only
steps, schedules and histories.  The checks are those of every cell
(tests/ensemble_parity.py, tests/ensemble_contract.py; tolerances and the hot bars outside
the Taylor limit: tests/ensemble_cases.py).
"""
import pytest

import ensemble_contract as contract
import ensemble_parity as parity
from ensemble_cases import CELL

pytestmark = pytest.mark.gpu

fams = pytest.mark.parametrize("fam", ["cg", "dg"])


def cell(fam):
    return CELL[fam + "-paper"]


@pytest.mark.parametrize("n_cells", [1, 2, 3, 16])
@fams
def test_parity_with_oracle(fam, n_cells):
    parity.parity_with_oracle(cell(fam), n_cells)


@fams
def test_thermal_problem_does_not_see_the_mode(fam):
    parity.thermal_problem_does_not_see_the_mode(cell(fam))


@fams
def test_independence_padding_and_split(fam):
    contract.independence_padding_and_split(cell(fam))


@fams
def test_long_horizon(fam):
    parity.long_horizon(cell(fam))


@fams
def test_against_single_bar_path(fam):
    parity.against_single_bar_path(cell(fam))


@pytest.mark.parametrize("error_on_nonconvergence", [True, False])
@fams
def test_failure_semantics(fam, error_on_nonconvergence):
    contract.failure_semantics(cell(fam), error_on_nonconvergence)


@fams
def test_thermal_only(fam):
    contract.thermal_only(cell(fam))


@pytest.mark.parametrize("n_cells", [1, 3, 16])
@fams
def test_schedule_parity_with_oracle(fam, n_cells):
    parity.schedule_parity_with_oracle(cell(fam), n_cells)


@fams
def test_schedule_that_changes_nothing_changes_no_bit(fam):
    contract.schedule_that_changes_nothing_changes_no_bit(cell(fam))


@pytest.mark.parametrize("n_cells", [3, 16])
@fams
def test_stage_change_is_a_restart(fam, n_cells):
    contract.stage_change_is_a_restart(cell(fam), n_cells)


@fams
def test_scheduled_independence_and_splits(fam):
    contract.scheduled_independence_and_splits(cell(fam))


@pytest.mark.parametrize("n_cells", [1, 16])
@fams
def test_history(fam, n_cells):
    contract.history(cell(fam), n_cells)


@fams
def test_history_and_a_failed_bar(fam):
    contract.history_and_a_failed_bar(cell(fam))


@fams
def test_history_capacity(fam):
    contract.history_capacity(cell(fam))


@pytest.mark.parametrize("n_cells", [1, 5])
@fams
def test_field_shapes(fam, n_cells):
    contract.field_shapes(cell(fam), n_cells)


@fams
def test_partial_stress_fields_exist_only_on_a_paper_handle(fam):
    parity.partial_stress_fields_exist_only_on_a_paper_handle(cell(fam))
