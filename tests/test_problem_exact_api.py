"""tv_set_relaxation without a GPU: the two constants and the prototype are in the header, the library
exports the symbol and the Python binding covers it, a NULL context is refused, the ABI version stays 8
(the call is additive), and ThermoViscoProblem validates relaxation= before the library is loaded."""
import inspect
import re

import pytest

from ensemble_api_util import header, load_lib
from oracle.tv_oracle import MAIN_MODEL_PARAMS

CG = {"element": "CG", "degree": 1}
CFG = {"T": CG, "sigma": CG}


@pytest.fixture(scope="module")
def lib():
    return load_lib()


def test_header_declares_the_setter():
    h = header()
    assert re.search(r"^#define TV_RELAX_TAYLOR\s+0\s*$", h, re.M)
    assert re.search(r"^#define TV_RELAX_EXACT\s+1\s*$", h, re.M)
    assert re.search(r"^int tv_set_relaxation\(void\* ctx, int relaxation\);\s*$", h, re.M)
    assert re.search(r"^#define TV_MODEL_PAPER_EXACT 2\s*$", h, re.M)  # the ensembles' constant has not moved
    assert re.search(r"^#define TV_ABI_VERSION 8\b", h, re.M)


def test_library_exports_and_binds_the_setter(lib):
    from tvfem import _native as N
    assert hasattr(lib, "tv_set_relaxation")
    assert "tv_set_relaxation" in N.EXPORTS
    assert (N.TV_RELAX_TAYLOR, N.TV_RELAX_EXACT) == (0, 1)
    assert lib.tv_abi_version() == 8 and N.ABI_VERSION == 8


@pytest.mark.parametrize("value", [0, 1, 7])
def test_null_context_is_refused(lib, value):
    from tvfem import _native as N
    assert lib.tv_set_relaxation(None, value) == N.TV_ERR_ARG


def test_python_validation_before_the_library(monkeypatch):
    from tvfem import _native as N
    from tvfem import interval_mesh
    from tvfem.problem import ThermoViscoProblem

    def boom():
        raise RuntimeError("stop before the library")

    monkeypatch.setattr(N, "load_library", boom)
    mesh = interval_mesh(50.0, 10)
    mp = dict(MAIN_MODEL_PARAMS)
    with pytest.raises(ValueError, match="relaxation='exact' needs model_mode='paper'"):
        ThermoViscoProblem(mesh, (0, 1), 0.1, CFG, mp, relaxation="exact")
    with pytest.raises(ValueError, match="relaxation='exact' needs model_mode='paper'"):
        ThermoViscoProblem(mesh, (0, 1), 0.1, CFG, mp, model_mode="reference", relaxation="exact")
    for bad in ("Exact", "pade", "", "paper"):
        for mode in ("reference", "paper"):
            with pytest.raises(ValueError, match="relaxation must be 'taylor'"):
                ThermoViscoProblem(mesh, (0, 1), 0.1, CFG, mp, model_mode=mode, relaxation=bad)
    # valid choices get as far as the library, with the attribute already set
    for mode, relaxation in (("reference", "taylor"), ("paper", "taylor"), ("paper", "exact")):
        p = ThermoViscoProblem.__new__(ThermoViscoProblem)
        with pytest.raises(RuntimeError, match="stop before"):
            ThermoViscoProblem.__init__(p, mesh, (0, 1), 0.1, CFG, mp, model_mode=mode, relaxation=relaxation)
        assert p.relaxation == relaxation


def test_same_messages_as_the_ensemble(monkeypatch):
    import numpy as np
    from tvfem import ThermoViscoEnsemble, interval_mesh
    from tvfem.problem import ThermoViscoProblem
    mesh = interval_mesh(50.0, 10)
    mp = dict(MAIN_MODEL_PARAMS)
    for kw in (dict(relaxation="pade"), dict(relaxation="exact")):
        with pytest.raises(ValueError) as e_ens:
            ThermoViscoEnsemble(mesh, (0, 1), 0.1, CFG, dict(mp, htc=np.array([100.0, 200.0])), **kw)
        with pytest.raises(ValueError) as e_prob:
            ThermoViscoProblem(mesh, (0, 1), 0.1, CFG, mp, **kw)
        assert str(e_prob.value) == str(e_ens.value)


def test_signature():
    from tvfem.problem import ThermoViscoProblem
    par = inspect.signature(ThermoViscoProblem.__init__).parameters["relaxation"]
    assert par.default == "taylor" and par.kind is inspect.Parameter.KEYWORD_ONLY
    assert list(inspect.signature(ThermoViscoProblem.set_relaxation).parameters) == ["self", "relaxation"]
