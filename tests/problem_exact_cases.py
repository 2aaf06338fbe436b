"""The cases of the ThermoViscoProblem exact-relaxation tests, once (tests/test_problem_exact.py,
tests/test_guard_bands_problem_exact.py).  A support module (pytest does not collect it).

main.py's parameters with T_0 = 920 K (above Tb = 869 K, where the Taylor polynomial of paper
mode exceeds 1 and the stress memory grows every step), dt = 0.1, 8 steps.  The meshes are the
smallest on which each kernel of csrc/tv_visco.hip takes every path: 1D, 2D and 3D, the fused
kernel (same families) and the two mixed passes (T pass + sigma pass, both directions), one
full workgroup and a tail (3d_cg: 315 dofs).
"""
import numpy as np
import pytest

from oracle import tv_oracle as O

CG = {"element": "CG", "degree": 1}
DG = {"element": "DG", "degree": 1}
DT = 0.1
N_STEPS = 8
MP = dict(O.MAIN_MODEL_PARAMS, T_0=920.0)

_X2 = [np.linspace(0.0, 3.0, 7), np.linspace(0.0, 1.0, 5)]
CASES = {
    "1d_cg": ([np.linspace(0.0, 50.0, 17)], CG, CG),
    "1d_dg_cg": ([np.concatenate([np.linspace(0, 5, 5), np.linspace(5, 45, 5)[1:], np.linspace(45, 50, 5)[1:]])],
                 DG, CG),
    "2d_cg": (_X2, CG, CG),
    "2d_cg_dg": (_X2, CG, DG),
    "2d_dg_cg": (_X2, DG, CG),
    "3d_cg": ([np.linspace(0.0, 2.0, 9), np.linspace(0.0, 2.0, 7), np.linspace(0.0, 1.0, 5)], CG, CG),
    "3d_dg": ([np.linspace(0.0, 1.0, 4), np.linspace(0.0, 1.0, 4), np.linspace(0.0, 0.5, 3)], DG, DG),
}

THERMAL = ("T", "T_prev", "Tf", "Tf_partial", "phi", "xi")  # what the relaxation does not reach
STRESS = ("sigma", "s_partial", "sigma_partial", "s_tilde_partial", "sigma_tilde_partial")


def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def cfg_of(name):
    _, tf, sf = CASES[name]
    return {"T": tf, "sigma": sf}


def problem(name, relaxation="exact", model_mode="paper", materialize=True, mp=MP):
    from tvfem import RectilinearMesh
    from tvfem.problem import ThermoViscoProblem
    axes = CASES[name][0]
    return ThermoViscoProblem(RectilinearMesh(axes), (0.0, 1.0), DT, cfg_of(name), dict(mp),
                              part_axis=2 if len(axes) == 3 else -1, materialize=materialize, verbose=False,
                              model_mode=model_mode, relaxation=relaxation)


def oracle(name, mp=MP):
    ref = O.OracleProblem(O.rectilinear_mesh(CASES[name][0]), (0.0, 1.0), DT, cfg_of(name), dict(mp), linear="pcg",
                          model_mode="paper")
    ref.setup()
    return ref


def fields(p, names=THERMAL + STRESS):
    return {f: np.array(p.get_field(f)) for f in names}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))
