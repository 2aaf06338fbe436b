"""TV_MODEL_PAPER_EXACT without a GPU: the constant exists everywhere the ABI is declared
(additively: the version stays 8), tv_ensemble_create_paper accepts it for both pairings
and refuses any other value, every other constructor refuses it before the GPU is
touched, and the Python class validates relaxation= and routes "exact" to the native
constructor."""
import ctypes as C
import re

import numpy as np
import pytest

from ensemble_api_util import CFG_CG, CFG_DG, CG1_CG1, DG1_CG1, create, header, load_lib, no_gpu_env
from oracle.tv_oracle import MAIN_MODEL_PARAMS

EXACT = 2


@pytest.fixture(scope="module")
def lib():
    return load_lib()


def test_constant_present(lib):
    from tvfem import _native as N
    assert re.search(r"^#define TV_MODEL_PAPER_EXACT 2\s*$", header(), re.M)
    assert N.TV_MODEL_PAPER_EXACT == EXACT
    assert (N.TV_MODEL_REFERENCE, N.TV_MODEL_PAPER) == (0, 1)
    assert re.search(r"^#define TV_ABI_VERSION 8\b", header(), re.M)
    assert lib.tv_abi_version() == 8 and N.ABI_VERSION == 8  # additive: nothing existing moved


@pytest.mark.parametrize("fe", [CG1_CG1, DG1_CG1])
def test_create_paper_accepts_exact_as_far_as_the_device(lib, fe):
    no_gpu_env()
    from tvfem import _native as N
    rc, msg = create(lib, "tv_ensemble_create_paper", fe=fe, model_mode=EXACT)
    assert rc == N.TV_ERR_HIP, (rc, msg)
    assert "GPU" in msg or "HIP" in msg


@pytest.mark.parametrize("fe", [CG1_CG1, DG1_CG1])
@pytest.mark.parametrize("model_mode", [3, -1, 7])
def test_create_paper_refuses_any_other_value(lib, fe, model_mode):
    from tvfem import _native as N
    rc, msg = create(lib, "tv_ensemble_create_paper", fe=fe, model_mode=model_mode)
    assert rc == N.TV_ERR_ARG, (rc, msg)
    assert msg.startswith("tv_ensemble_create_paper: ") and "model_mode" in msg, msg


@pytest.mark.parametrize("fn,fe", [("tv_ensemble_create", CG1_CG1), ("tv_ensemble_create_dg", DG1_CG1)])
def test_reference_constructors_refuse_exact(lib, fn, fe):
    """TV_ERR_ARG also where a GPU is present: decided before the first HIP call."""
    from tvfem import _native as N
    rc, msg = create(lib, fn, fe=fe, model_mode=EXACT)
    assert rc == N.TV_ERR_ARG, (rc, msg)
    assert msg.startswith(fn + ": ") and "model_mode" in msg, msg


def test_single_problem_path_refuses_exact(lib):
    """tv_create would run value 2 as reference mode; it says where the exact relaxation exists."""
    from tvfem import _native as N
    axes = [np.ascontiguousarray(np.linspace(0.0, 1.0, 3)) for _ in range(3)]
    mesh = N.MeshDesc()
    mesh.dim = 3
    for d in range(3):
        mesh.n_cells[d] = 2
        mesh.coords[d] = axes[d].ctypes.data_as(C.POINTER(C.c_double))
    mesh.part_axis, mesh.n_parts, mesh.part = 0, 1, 0
    fe = N.FeConfig(N.TV_CG, 1, N.TV_CG, 1)
    params = N.default_params(None, 0.1)
    opts = N.default_options()
    opts.model_mode = EXACT
    ctx = C.c_void_p()
    rc = lib.tv_create(C.byref(mesh), C.byref(fe), C.byref(params), C.byref(opts), 0, C.byref(ctx))
    msg = (lib.tv_last_error(None) or b"").decode()
    assert rc == N.TV_ERR_ARG, (rc, msg)
    assert not ctx.value
    assert "ensembles only" in msg and "tv_create" in msg, msg


def test_python_validation():
    """Decided before the library is loaded or anything is created."""
    from tvfem import ThermoViscoEnsemble, interval_mesh
    mesh = interval_mesh(50.0, 10)
    mp = dict(MAIN_MODEL_PARAMS, htc=np.array([100.0, 200.0]))
    with pytest.raises(ValueError, match="relaxation='exact' needs model_mode='paper'"):
        ThermoViscoEnsemble(mesh, (0, 1), 0.1, CFG_CG, mp, relaxation="exact")
    with pytest.raises(ValueError, match="relaxation='exact' needs model_mode='paper'"):
        ThermoViscoEnsemble(mesh, (0, 1), 0.1, CFG_DG, mp, model_mode="reference", relaxation="exact")
    for bad in ("Exact", "pade", "", "paper"):
        for mode in ("reference", "paper"):
            with pytest.raises(ValueError, match="relaxation must be"):
                ThermoViscoEnsemble(mesh, (0, 1), 0.1, CFG_CG, mp, model_mode=mode, relaxation=bad)


@pytest.mark.parametrize("cfg", [CFG_CG, CFG_DG], ids=["cg", "dg"])
def test_class_routes_exact_to_the_native_constructor(lib, cfg, monkeypatch):
    """The class hands tv_ensemble_create_paper options with model_mode 2 (taylor: 1); without a
    GPU the native creation is what fails."""
    from tvfem import NativeError, ThermoViscoEnsemble, interval_mesh
    from tvfem import _native as N
    seen = []

    class Spy:  # records the options of the constructor call and refuses, so no handle is made
        def __init__(self, real):
            self._real = real

        def __getattr__(self, name):
            return getattr(self._real, name)

        def tv_ensemble_create_paper(self, desc, fe, params, opts, device, ens_out):
            seen.append(opts._obj.model_mode)
            return N.TV_ERR_ARG

        def tv_ensemble_create(self, *a):
            raise AssertionError("paper mode goes to tv_ensemble_create_paper")

        tv_ensemble_create_dg = tv_ensemble_create

    monkeypatch.setattr(N, "load_library", lambda: Spy(lib))
    mp = dict(MAIN_MODEL_PARAMS, htc=np.array([100.0, 200.0]))
    for relaxation, want in (("exact", N.TV_MODEL_PAPER_EXACT), ("taylor", N.TV_MODEL_PAPER)):
        with pytest.raises(NativeError):
            ThermoViscoEnsemble(interval_mesh(50.0, 10), (0, 1), 0.1, cfg, mp, model_mode="paper",
                                relaxation=relaxation)
        assert seen[-1] == want
    monkeypatch.undo()
    no_gpu_env()
    with pytest.raises(NativeError) as exc:
        ThermoViscoEnsemble(interval_mesh(50.0, 10), (0, 1), 0.1, cfg, mp, model_mode="paper", relaxation="exact",
                            history=dict(nodes=[0, 5, 10], every=2))
    assert exc.value.code == N.TV_ERR_HIP, str(exc.value)


def test_relaxation_attribute(lib, monkeypatch):
    """ens.relaxation holds the choice; "taylor" is the default (set before the native call)."""
    from tvfem import ThermoViscoEnsemble, interval_mesh
    import inspect
    assert inspect.signature(ThermoViscoEnsemble.__init__).parameters["relaxation"].default == "taylor"
    from tvfem import _native as N
    made = []

    def boom():
        raise RuntimeError("stop before the library")

    monkeypatch.setattr(N, "load_library", boom)
    real_init = ThermoViscoEnsemble.__init__
    for relaxation in ("taylor", "exact"):
        ens = ThermoViscoEnsemble.__new__(ThermoViscoEnsemble)
        with pytest.raises(RuntimeError, match="stop before"):
            real_init(ens, interval_mesh(50.0, 10), (0, 1), 0.1, CFG_CG, dict(MAIN_MODEL_PARAMS), model_mode="paper",
                      relaxation=relaxation)
        made.append(ens.relaxation)
    assert made == ["taylor", "exact"]
