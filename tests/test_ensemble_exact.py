"""ThermoViscoEnsemble(model_mode="paper", relaxation="exact"), the two exact cells: the
exact exponential relaxation of the paper-mode bar kernels (the kModel = 2 instantiations of
csrc/tv_ensemble_step.h; EXACT in s_part of csrc/tv_visco_point.h), CG1 / CG1 and DG1 / CG1:
against the CPU oracle with the same relaxation (tests/exact_relaxation.py, the oracle itself
unchanged) bar by bar over 6 and over 500 steps, against the relaxation="taylor" ensemble
(everything but the stress is the same bits), against itself, and the contracts of a paper
ensemble under it: failure, thermal-only steps, schedules, histories.  The checks are those
of every cell (tests/ensemble_parity.py, tests/ensemble_contract.py; tolerances:
tests/ensemble_cases.py).
"""
import pytest

import ensemble_contract as contract
import ensemble_parity as parity
from ensemble_cases import CELL

pytestmark = pytest.mark.gpu

fams = pytest.mark.parametrize("fam", ["cg", "dg"])


def cell(fam):
    return CELL[fam + "-exact"]


@pytest.mark.parametrize("n_cells", [1, 2, 3, 16])
@fams
def test_parity_with_oracle(fam, n_cells):
    parity.parity_with_oracle(cell(fam), n_cells)


@fams
def test_long_horizon_all_ten_bars(fam):
    parity.long_horizon(cell(fam))


@fams
def test_only_the_stress_sees_the_relaxation(fam):
    parity.only_the_stress_sees_the_relaxation(fam)


@fams
def test_independence_padding_and_split(fam):
    contract.independence_padding_and_split(cell(fam))


@fams
def test_failure_semantics(fam):
    for error_on_nonconvergence in (True, False):
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
