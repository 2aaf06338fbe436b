"""tv_ensemble_create_paper without a GPU: the symbol exists everywhere the ABI is
declared, it insists on options with model_mode PAPER and names the constructor
of the reference mode, every other refusal is that of the family's constructor
and is decided before the GPU is touched, and the Python class routes
model_mode="paper" to it for either config."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle.tv_oracle import MAIN_MODEL_PARAMS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "fem-glass-tempering_amd")
CFG_CG = {"T": {"element": "CG", "degree": 1}, "sigma": {"element": "CG", "degree": 1}}
CFG_DG = {"T": {"element": "DG", "degree": 1}, "sigma": {"element": "CG", "degree": 1}}
PAPER = 1
DG1_CG1 = ("DG", 1, "CG", 1)


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


def _create(lib, n_bars=3, n_cells=4, coords=None, fe=("CG", 1, "CG", 1), model_mode=PAPER, null_options=False):
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
    opts.model_mode = model_mode
    ens = C.c_void_p()
    rc = lib.tv_ensemble_create_paper(C.byref(desc), C.byref(fe), C.byref(params),
                                      None if null_options else C.byref(opts), 0, C.byref(ens))
    msg = (lib.tv_last_error(None) or b"").decode()
    if rc == N.TV_OK:
        lib.tv_ensemble_destroy(ens)
    return rc, msg


def test_symbol_present(lib):
    from tvfem import _native as N
    header = open(os.path.join(ROOT, "include", "tvfem.h")).read()
    assert "tv_ensemble_create_paper" in header
    assert "tv_ensemble_create_paper" in N.EXPORTS
    assert hasattr(lib, "tv_ensemble_create_paper")
    assert lib.tv_abi_version() == 8  # additive: nothing existing moved


@pytest.mark.parametrize("case,kw,words", [
    ("NULL options, CG", dict(null_options=True), ("options", "PAPER", "tv_ensemble_create)")),
    ("NULL options, DG", dict(null_options=True, fe=DG1_CG1), ("options", "PAPER", "tv_ensemble_create_dg)")),
    ("reference mode, CG", dict(model_mode=0), ("model_mode", "PAPER", "tv_ensemble_create)")),
    ("reference mode, DG", dict(model_mode=0, fe=DG1_CG1), ("model_mode", "PAPER", "tv_ensemble_create_dg)")),
    ("DG stress", dict(fe=("DG", 1, "DG", 1)), ("DG1 temperature with CG1 stress",)),
    ("CG temperature, DG stress", dict(fe=("CG", 1, "DG", 1)), ("CG1 temperature with CG1 stress",)),
    ("T degree 2, CG", dict(fe=("CG", 2, "CG", 1)), ("CG1 temperature with CG1 stress",)),
    ("T degree 2, DG", dict(fe=("DG", 2, "CG", 1)), ("DG1 temperature with CG1 stress",)),
    ("sigma degree 2", dict(fe=("CG", 1, "CG", 2)), ("CG1 temperature with CG1 stress",)),
    ("n_bars = 0", dict(n_bars=0), ("n_bars",)),
    ("n_cells = 0", dict(n_cells=0), ("n_cells",)),
    ("non-increasing row", dict(coords=[[0, 1, 2, 3, 4], [0, 1, 1, 3, 4], [0, 1, 2, 3, 4]]), ("increasing", "bar 1")),
    ("non-increasing row, DG", dict(fe=("DG", 1, "CG", 1), coords=[[0, 1, 2, 3, 4], [0, 1, 2, 3, 4], [0, 1, 2, 3, 3]]),
     ("increasing", "bar 2")),
])
def test_create_paper_refuses_before_the_gpu(lib, case, kw, words):
    from tvfem import _native as N
    rc, msg = _create(lib, **kw)
    assert rc == N.TV_ERR_ARG, (case, rc, msg)
    assert msg.startswith("tv_ensemble_create_paper: "), (case, msg)
    for word in words:
        assert word in msg, (case, msg)


@pytest.mark.parametrize("fe", [("CG", 1, "CG", 1), ("DG", 1, "CG", 1)])
def test_create_paper_without_gpu_fails_loudly(lib, fe):
    _no_gpu()
    from tvfem import _native as N
    rc, msg = _create(lib, fe=fe)
    assert rc == N.TV_ERR_HIP
    assert "GPU" in msg or "HIP" in msg


def test_null_arguments(lib):
    from tvfem import _native as N
    ens = C.c_void_p()
    assert lib.tv_ensemble_create_paper(None, None, None, None, 0, C.byref(ens)) == N.TV_ERR_ARG
    assert "tv_ensemble_create_paper" in lib.tv_last_error(None).decode()


@pytest.mark.parametrize("cfg", [CFG_CG, CFG_DG], ids=["cg", "dg"])
def test_class_routes_paper_mode_to_the_native_constructor(lib, cfg):
    """Python validation passes; what fails without a GPU is the native creation, not
    the refusal of PAPER by tv_ensemble_create / tv_ensemble_create_dg."""
    _no_gpu()
    from tvfem import NativeError, ThermoViscoEnsemble, interval_mesh
    from tvfem import _native as N
    from tvfem.ensemble import SIGMA_FAMILY, STATE_FIELDS
    with pytest.raises(NativeError) as exc:
        ThermoViscoEnsemble(interval_mesh(50.0, 10), (0, 1), 0.1, cfg,
                            dict(MAIN_MODEL_PARAMS, htc=np.array([100.0, 200.0])), model_mode="paper",
                            history=dict(nodes=[0, 5, 10], every=2))
    assert exc.value.code == N.TV_ERR_HIP, str(exc.value)
    for name in ("s_partial", "sigma_partial"):
        assert STATE_FIELDS[name] == 6 and name in SIGMA_FAMILY
