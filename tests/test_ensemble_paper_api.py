"""tv_ensemble_create_paper without a GPU: the symbol exists everywhere the ABI is
declared, it insists on options with model_mode PAPER and names the constructor
of the reference mode, every other refusal is that of the family's constructor
and is decided before the GPU is touched, and the Python class routes
model_mode="paper" to it for either config."""
import ctypes as C

import numpy as np
import pytest

from ensemble_api_util import CFG_CG, CFG_DG, DG1_CG1, create, header, load_lib, no_gpu_env
from oracle.tv_oracle import MAIN_MODEL_PARAMS

PAPER = 1


@pytest.fixture(scope="module")
def lib():
    return load_lib()


def test_symbol_present(lib):
    from tvfem import _native as N
    assert "tv_ensemble_create_paper" in header()
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
    rc, msg = create(lib, "tv_ensemble_create_paper", **dict(dict(model_mode=PAPER), **kw))
    assert rc == N.TV_ERR_ARG, (case, rc, msg)
    assert msg.startswith("tv_ensemble_create_paper: "), (case, msg)
    for word in words:
        assert word in msg, (case, msg)


@pytest.mark.parametrize("fe", [("CG", 1, "CG", 1), ("DG", 1, "CG", 1)])
def test_create_paper_without_gpu_fails_loudly(lib, fe):
    no_gpu_env()
    from tvfem import _native as N
    rc, msg = create(lib, "tv_ensemble_create_paper", fe=fe, model_mode=PAPER)
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
    no_gpu_env()
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
