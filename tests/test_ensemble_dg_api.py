"""tv_ensemble_create_dg without a GPU: the symbol exists everywhere the ABI is
declared, every refusal is decided before the GPU is touched, and the Python
class routes a DG1 / CG1 config to it."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle.tv_oracle import MAIN_MODEL_PARAMS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "fem-glass-tempering_amd")
CFG = {"T": {"element": "DG", "degree": 1}, "sigma": {"element": "CG", "degree": 1}}


@pytest.fixture(scope="module")
def lib():
    so = os.path.join(PKG, "tvfem", "libtvfem.so")
    if not os.path.exists(so):
        subprocess.run(["make", "-C", PKG, "-j8"], check=True, capture_output=True)
    from tvfem import _native as N
    return N.load_library()


def _no_gpu():
    try:
        import torch
        if torch.cuda.is_available():
            pytest.skip("GPU present")
    except ImportError:
        pass


def _create(lib, n_bars=3, n_cells=4, coords=None, fe=("DG", 1, "CG", 1), model_mode=None):
    from tvfem import _native as N
    if coords is None:
        coords = np.tile(np.linspace(0.0, 1.0, max(n_cells, 0) + 1), (max(n_bars, 1), 1))
    coords = np.ascontiguousarray(coords, dtype=np.float64)
    desc = N.EnsembleDesc()
    desc.n_bars, desc.n_cells = n_bars, n_cells
    desc.coords = coords.ctypes.data_as(C.POINTER(C.c_double))
    fam = {"CG": N.TV_CG, "DG": N.TV_DG}
    fe = N.FeConfig(fam[fe[0]], fe[1], fam[fe[2]], fe[3])
    params = N.default_params(None, 0.1)
    opts = N.default_options()
    if model_mode is not None:
        opts.model_mode = model_mode
    ens = C.c_void_p()
    rc = lib.tv_ensemble_create_dg(C.byref(desc), C.byref(fe), C.byref(params), C.byref(opts), 0, C.byref(ens))
    msg = (lib.tv_last_error(None) or b"").decode()
    if rc == N.TV_OK:
        lib.tv_ensemble_destroy(ens)
    return rc, msg


def test_symbol_present(lib):
    from tvfem import _native as N
    header = open(os.path.join(ROOT, "include", "tvfem.h")).read()
    assert "tv_ensemble_create_dg" in header
    assert "tv_ensemble_create_dg" in N.EXPORTS
    assert hasattr(lib, "tv_ensemble_create_dg")
    assert lib.tv_abi_version() == 8  # additive: nothing existing moved


@pytest.mark.parametrize("case,kw,words", [
    ("CG temperature", dict(fe=("CG", 1, "CG", 1)), ("DG1 temperature with CG1 stress", "tv_ensemble_create")),
    ("DG stress", dict(fe=("DG", 1, "DG", 1)), ("DG1 temperature with CG1 stress",)),
    ("T degree 2", dict(fe=("DG", 2, "CG", 1)), ("DG1 temperature with CG1 stress",)),
    ("sigma degree 2", dict(fe=("DG", 1, "CG", 2)), ("DG1 temperature with CG1 stress",)),
    ("paper mode", dict(model_mode=1), ("PAPER",)),
    ("n_bars = 0", dict(n_bars=0), ("n_bars",)),
    ("n_cells = 0", dict(n_cells=0), ("n_cells",)),
    ("non-increasing row", dict(coords=[[0, 1, 2, 3, 4], [0, 1, 1, 3, 4], [0, 1, 2, 3, 4]]), ("increasing", "bar 1")),
])
def test_create_dg_refuses_before_the_gpu(lib, case, kw, words):
    from tvfem import _native as N
    rc, msg = _create(lib, **kw)
    assert rc == N.TV_ERR_ARG, (case, rc, msg)
    assert msg.startswith("tv_ensemble_create_dg: "), (case, msg)
    for word in words:
        assert word in msg, (case, msg)


def test_create_dg_without_gpu_fails_loudly(lib):
    _no_gpu()
    from tvfem import _native as N
    rc, msg = _create(lib)
    assert rc == N.TV_ERR_HIP
    assert "GPU" in msg or "HIP" in msg


def test_class_routes_dg_config_to_the_native_constructor(lib):
    """Python validation passes; what fails without a GPU is the native creation."""
    _no_gpu()
    from tvfem import NativeError, ThermoViscoEnsemble, interval_mesh
    from tvfem import _native as N
    with pytest.raises(NativeError) as exc:
        ThermoViscoEnsemble(interval_mesh(50.0, 10), (0, 1), 0.1, CFG,
                            dict(MAIN_MODEL_PARAMS, htc=np.array([100.0, 200.0])),
                            history=dict(nodes=[0, 5, 10], every=2))
    assert exc.value.code == N.TV_ERR_HIP
    # the same validation as for CG bars, before anything is created
    with pytest.raises(ValueError, match="probe node outside"):
        ThermoViscoEnsemble(interval_mesh(50.0, 10), (0, 1), 0.1, CFG, dict(MAIN_MODEL_PARAMS),
                            history=dict(nodes=[11]))
