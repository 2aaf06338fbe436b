"""tv_ensemble_create_dg without a GPU: the symbol exists everywhere the ABI is
declared, every refusal is decided before the GPU is touched, and the Python
class routes a DG1 / CG1 config to it."""
import numpy as np
import pytest

from ensemble_api_util import CFG_DG as CFG, DG1_CG1, create, header, load_lib, no_gpu_env
from oracle.tv_oracle import MAIN_MODEL_PARAMS



@pytest.fixture(scope="module")
def lib():
    return load_lib()


def test_symbol_present(lib):
    from tvfem import _native as N
    assert "tv_ensemble_create_dg" in header()
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
    rc, msg = create(lib, "tv_ensemble_create_dg", **dict(dict(fe=DG1_CG1), **kw))
    assert rc == N.TV_ERR_ARG, (case, rc, msg)
    assert msg.startswith("tv_ensemble_create_dg: "), (case, msg)
    for word in words:
        assert word in msg, (case, msg)


def test_create_dg_without_gpu_fails_loudly(lib):
    no_gpu_env()
    from tvfem import _native as N
    rc, msg = create(lib, "tv_ensemble_create_dg", fe=DG1_CG1)
    assert rc == N.TV_ERR_HIP
    assert "GPU" in msg or "HIP" in msg


def test_class_routes_dg_config_to_the_native_constructor(lib):
    """Python validation passes; what fails without a GPU is the native creation."""
    no_gpu_env()
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
