"""The ensemble surface without a GPU: the ABI additions exist, every refusal of
tv_ensemble_create is decided before the GPU is touched, and the Python class
validates its arguments before it creates anything."""
import numpy as np
import pytest

from ensemble_api_util import CFG_CG as CFG, create, header, load_lib, no_gpu_env
from oracle.tv_oracle import MAIN_MODEL_PARAMS

ENSEMBLE_SYMBOLS = ["tv_ensemble_create", "tv_ensemble_destroy", "tv_ensemble_set_initial_condition",
                    "tv_ensemble_step", "tv_ensemble_get_field", "tv_ensemble_set_field", "tv_ensemble_stats"]


@pytest.fixture(scope="module")
def lib():
    return load_lib()


def test_abi_additions_present(lib):
    from tvfem import _native as N
    assert "tv_ensemble_desc" in header()
    for name in ENSEMBLE_SYMBOLS:
        assert name in header() and name in N.EXPORTS and hasattr(lib, name), name
    assert lib.tv_abi_version() == 8  # additive: nothing existing moved


@pytest.mark.parametrize("case,kw,word", [
    ("n_bars = 0", dict(n_bars=0), "n_bars"),
    ("n_cells = 0", dict(n_cells=0), "n_cells"),
    ("non-increasing row", dict(coords=[[0, 1, 2, 3, 4], [0, 1, 1, 3, 4], [0, 1, 2, 3, 4]]), "increasing"),
    ("DG temperature", dict(fe=("DG", "CG")), "CG1"),
    ("DG stress", dict(fe=("CG", "DG")), "CG1"),
    ("paper mode", dict(model_mode=1), "PAPER"),
])
def test_create_refuses_before_the_gpu(lib, case, kw, word):
    from tvfem import _native as N
    if "fe" in kw:
        kw = dict(kw, fe=(kw["fe"][0], 1, kw["fe"][1], 1))
    rc, msg = create(lib, "tv_ensemble_create", **kw)
    assert rc == N.TV_ERR_ARG, (case, rc, msg)
    assert word in msg, (case, msg)
    if case.startswith("non-increasing"):
        assert "bar 1" in msg


def test_create_without_gpu_fails_loudly(lib):
    no_gpu_env()
    from tvfem import _native as N
    rc, msg = create(lib, "tv_ensemble_create")
    assert rc == N.TV_ERR_HIP
    assert "GPU" in msg or "HIP" in msg


def test_class_validates_before_creating(lib):
    from tvfem import RectilinearMesh, ThermoViscoEnsemble, interval_mesh
    with pytest.raises(ValueError, match="'H'"):
        ThermoViscoEnsemble(interval_mesh(50.0, 10), (0, 1), 0.1, CFG,
                            dict(MAIN_MODEL_PARAMS, H=np.array([627.8e3, 600e3])))
    meshes = [RectilinearMesh([np.linspace(0, 1, 11)]), RectilinearMesh([np.linspace(0, 1, 12)])]
    with pytest.raises(ValueError, match="cell count"):
        ThermoViscoEnsemble(meshes, (0, 1), 0.1, CFG, dict(MAIN_MODEL_PARAMS))
    with pytest.raises(ValueError, match="inconsistent"):
        ThermoViscoEnsemble(interval_mesh(50.0, 10), (0, 1), 0.1, CFG,
                            dict(MAIN_MODEL_PARAMS, htc=np.array([1.0, 2.0]), T_0=np.array([800.0, 810.0, 820.0])))
