"""Process schedules and probe histories of ensembles, without a GPU: the ABI
additions exist, the new entry points refuse a null handle, and the Python
class decides every refusal of `schedule=` / `history=` before it creates
anything (so a machine without a GPU still gets the ValueError)."""
import numpy as np
import pytest

from ensemble_api_util import CFG_CG as CFG, header, load_lib
from oracle.tv_oracle import MAIN_MODEL_PARAMS

NEW_SYMBOLS = ["tv_ensemble_set_schedule", "tv_ensemble_history_open", "tv_ensemble_history_read"]


@pytest.fixture(scope="module")
def lib():
    return load_lib()


def test_symbols_present(lib):
    from tvfem import _native as N
    assert "tv_ensemble_schedule" in header()
    for name in NEW_SYMBOLS:
        assert name in header() and name in N.EXPORTS and hasattr(lib, name), name
    assert lib.tv_abi_version() == 8  # additive: nothing existing moved


def test_null_handle_is_an_argument_error(lib):
    from tvfem import _native as N
    assert lib.tv_ensemble_set_schedule(None, None) == N.TV_ERR_ARG
    assert lib.tv_ensemble_history_open(None, 0, None, 1, 1) == N.TV_ERR_ARG
    assert lib.tv_ensemble_history_read(None, None, 0, None) == N.TV_ERR_ARG


def _make(n_cells=10, mp=None, **kw):
    from tvfem import ThermoViscoEnsemble, interval_mesh
    return ThermoViscoEnsemble(interval_mesh(50.0, n_cells), (0.0, 5.0), 0.1, CFG,
                               dict(MAIN_MODEL_PARAMS, **(mp or {})), **kw)


@pytest.mark.parametrize("case,kw,match", [
    ("unknown stage key", dict(schedule=[dict(until_step=3, htc=900.0, H=1.0), dict(htc=60.0)]), "'H'"),
    ("last stage with an end", dict(schedule=[dict(until_step=3, htc=900.0), dict(until=2.0, htc=60.0)]), "last stage"),
    ("non-last stage without an end", dict(schedule=[dict(htc=900.0), dict(htc=60.0)]), "until"),
    ("both ends in one stage", dict(schedule=[dict(until=1.0, until_step=10, htc=900.0), dict(htc=60.0)]), "until"),
    ("until off the step grid", dict(schedule=[dict(until=np.array([1.0, 1.05, 2.0]), htc=900.0), dict(htc=60.0)]),
     "bar 1"),
    ("decreasing ends", dict(schedule=[dict(until_step=np.array([3, 5, 4]), htc=900.0),
                                       dict(until_step=np.array([3, 4, 9]), htc=500.0), dict(htc=60.0)]), "bar 1"),
    ("negative end", dict(schedule=[dict(until_step=-1, htc=900.0), dict(htc=60.0)]), "before the start"),
    ("inconsistent sizes", dict(mp=dict(htc=np.array([1.0, 2.0])),
                                schedule=[dict(until_step=3, T_ambient=np.array([300.0, 310.0, 320.0])), dict()]),
     "inconsistent"),
    ("probe outside the bar", dict(history=dict(nodes=[0, 11])), "n_cells"),
    ("negative probe", dict(history=dict(nodes=[-1])), "n_cells"),
    ("every < 1", dict(history=dict(nodes=[0], every=0)), "every"),
    ("unknown history key", dict(history=dict(nodes=[0], each=2)), "'each'"),
])
def test_class_refuses_before_creating(lib, case, kw, match):
    with pytest.raises(ValueError, match=match):
        _make(**kw)


def test_until_on_the_grid_and_schedule_sizes_define_n_bars(lib):
    """A valid schedule passes validation: with a GPU the ensemble exists, without
    one creation itself fails loudly (NativeError, not ValueError)."""
    from tvfem import NativeError
    kw = dict(schedule=[dict(until=np.linspace(2.0, 4.0, 5), htc=900.0, T_ambient=293.0), dict(htc=60.0)],
              history=dict(nodes=[0, 5, 10], every=5))
    try:
        ens = _make(**kw)
    except NativeError:
        return
    assert ens.n_bars == 5
    ens.close()
