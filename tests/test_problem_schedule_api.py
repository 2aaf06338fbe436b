"""Process schedules and run histories of ThermoViscoProblem, without a GPU: the
ABI additions exist in the header, the exports and the binding, the ABI version
has not moved, the new entry points refuse a null context, and the class decides
every refusal of `schedule=` / `history=` at the top of its constructor -- before
the mesh is looked at and before the library is loaded, so a machine without a
GPU gets the ValueError too."""
import numpy as np
import pytest

from ensemble_api_util import CFG_CG as CFG, header, load_lib
from oracle.tv_oracle import MAIN_MODEL_PARAMS

NEW_SYMBOLS = ["tv_set_boundary", "tv_set_schedule", "tv_step_count", "tv_history_open", "tv_history_read"]


@pytest.fixture(scope="module")
def lib():
    return load_lib()


def test_symbols_present(lib):
    from tvfem import _native as N
    assert "tv_schedule;" in header()
    for name in NEW_SYMBOLS:
        assert name in header() and name in N.EXPORTS and hasattr(lib, name), name
    assert lib.tv_abi_version() == 8 and N.ABI_VERSION == 8  # additive: nothing existing moved
    assert "#define TV_ABI_VERSION 8" in header()


def test_null_context_is_an_argument_error(lib):
    from tvfem import _native as N
    assert lib.tv_set_boundary(None, 1.0, 300.0, 0.5) == N.TV_ERR_ARG
    assert lib.tv_set_schedule(None, None) == N.TV_ERR_ARG
    assert lib.tv_step_count(None, None) == N.TV_ERR_ARG
    assert lib.tv_history_open(None, 0, None, None, 1, 1) == N.TV_ERR_ARG
    assert lib.tv_history_read(None, None, 0, None) == N.TV_ERR_ARG


def _make(monkeypatch, **kw):
    """The constructor with the library out of reach: a refusal that comes must
    have been decided before load_library()."""
    from tvfem import _native as N
    from tvfem import interval_mesh
    from tvfem.problem import ThermoViscoProblem

    def no_library():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(N, "load_library", no_library)
    return ThermoViscoProblem(interval_mesh(50.0, 10), (0.0, 5.0), 0.1, CFG, dict(MAIN_MODEL_PARAMS),
                              verbose=False, **kw)


OK_STAGES = [dict(until_step=3, htc=900.0), dict(htc=60.0)]


@pytest.mark.parametrize("case,kw,match", [
    ("empty schedule", dict(schedule=[]), "at least one stage"),
    ("unknown stage key", dict(schedule=[dict(until_step=3, htc=900.0, H=1.0), dict(htc=60.0)]), "'H'"),
    ("last stage with an end", dict(schedule=[dict(until_step=3, htc=900.0), dict(until=2.0, htc=60.0)]), "last stage"),
    ("non-last stage without an end", dict(schedule=[dict(htc=900.0), dict(htc=60.0)]), "until"),
    ("both ends in one stage", dict(schedule=[dict(until=1.0, until_step=10, htc=900.0), dict(htc=60.0)]), "until"),
    ("until off the step grid", dict(schedule=[dict(until=1.05, htc=900.0), dict(htc=60.0)]), "step grid"),
    ("fractional until_step", dict(schedule=[dict(until_step=2.5, htc=900.0), dict(htc=60.0)]), "whole steps"),
    ("decreasing ends", dict(schedule=[dict(until_step=5, htc=900.0), dict(until_step=4, htc=500.0), dict(htc=60.0)]),
     "decrease"),
    ("negative end", dict(schedule=[dict(until_step=-1, htc=900.0), dict(htc=60.0)]), "before the start"),
    ("per-bar array", dict(schedule=[dict(until_step=3, htc=np.array([900.0, 800.0])), dict(htc=60.0)]), "scalar"),
    ("2D value", dict(schedule=[dict(until_step=3, htc=np.ones((2, 2))), dict(htc=60.0)]), "scalar"),
    ("value not finite", dict(schedule=[dict(until_step=3, T_ambient=float("nan")), dict(htc=60.0)]), "not finite"),
    ("negative htc", dict(schedule=[dict(until_step=3, htc=-1.0), dict(htc=60.0)]), "negative"),
    ("negative epsilon", dict(schedule=[dict(until_step=3, epsilon=-0.1), dict()]), "negative"),
    ("unknown history key", dict(history=dict(dofs=[0], each=2)), "'each'"),
    ("neither points nor dofs", dict(history=dict(every=2)), "exactly one"),
    ("points and dofs", dict(history=dict(points=[[0.0]], dofs=[0])), "exactly one"),
    ("empty points", dict(history=dict(points=[])), "points"),
    ("points not finite", dict(history=dict(points=[[float("inf"), 0.0, 0.0]])), "points"),
    ("points with 4 coordinates", dict(history=dict(points=[[0.0, 0.0, 0.0, 0.0]])), "points"),
    ("empty dofs", dict(history=dict(dofs=[])), "dofs"),
    ("fractional dof", dict(history=dict(dofs=[0.5])), "dofs"),
    ("negative dof", dict(history=dict(dofs=[0, -1])), "negative"),
    ("dofs dict with a wrong key", dict(history=dict(dofs=dict(T=[0], s=[0]))), "dofs"),
    ("unequal dof counts", dict(history=dict(dofs=dict(T=[0, 1], sigma=[0]))), "as many"),
    ("every < 1", dict(history=dict(dofs=[0], every=0)), "every"),
    ("max_records < 1", dict(history=dict(dofs=[0], max_records=0)), "max_records"),
    ("bad history beside a good schedule", dict(schedule=OK_STAGES, history=dict(dofs=[0], every=-2)), "every"),
])
def test_class_refuses_before_loading_the_library(monkeypatch, case, kw, match):
    with pytest.raises(ValueError, match=match):
        _make(monkeypatch, **kw)


def test_valid_arguments_reach_the_library(monkeypatch):
    """A valid schedule and history pass the checks: the next thing the constructor wants is the library."""
    with pytest.raises(AssertionError, match="library was loaded"):
        _make(monkeypatch, schedule=[dict(until=0.3, htc=900.0, T_ambient=293.0, epsilon=0.93),
                                     dict(until_step=3), dict(htc=60.0, T_ambient=350.0, epsilon=0.5)],
              history=dict(points=[[0.0], [25.0]], every=2))


def test_schedule_tables_and_history_defaults():
    from tvfem.problem import _history_args, _schedule_tables
    end, tabs = _schedule_tables([dict(until=0.3, htc=900.0), dict(until_step=3, T_ambient=1.0), dict(htc=60.0)],
                                 0.0, 0.1, MAIN_MODEL_PARAMS)
    assert end.tolist() == [3, 3]
    assert tabs["htc"].tolist() == [900.0, MAIN_MODEL_PARAMS["htc"], 60.0]  # a missing key keeps the creation value
    assert tabs["T_ambient"].tolist() == [MAIN_MODEL_PARAMS["T_ambient"], 1.0, MAIN_MODEL_PARAMS["T_ambient"]]
    assert "epsilon" not in tabs  # NULL table
    points, dofs, every, max_records = _history_args(dict(points=[[1.0, 2.0]], every=3), 50)
    assert points.tolist() == [[1.0, 2.0, 0.0]] and dofs is None and every == 3 and max_records == 50 // 3
    _, dofs, _, max_records = _history_args(dict(dofs=dict(T=[0, 3], sigma=[1, 2]), max_records=7), 50)
    assert [d.tolist() for d in dofs] == [[0, 3], [1, 2]] and max_records == 7


def test_ensemble_keeps_its_parser():
    """tvfem/ensemble.py's names are those of the shared module."""
    from tvfem import ensemble, schedule
    assert ensemble._parse_stages is schedule.parse_stages
    assert ensemble.STAGE_KEYS == ("htc", "T_ambient", "epsilon") and ensemble.STAGE_ENDS == ("until", "until_step")
