"""Red zones around the DG general-mesh path (csrc/tv_umdg.hip), built on
tests/guard_util.py: every device allocation of the context between filled
guards (TVFEM_ALLOC_GUARD), the caller's vectors inside NaN arenas at an 8-byte
aligned, not 16-byte aligned address.  F, J x and diag J of
tests/test_unstructured_dg.py's operator case, then two coupled steps; no guard
byte may change, and the operators still meet the 1e-12 bar against the oracle,
so no NaN of a guard has been read in.  "quad" and "hex": 72 and 140 cells, the
last 64-cell group of each partly padding lanes.
"""
import numpy as np
import pytest

from guard_util import assert_guards_intact, guard_env, guarded
from parity_util import relerr
from test_unstructured_dg import device, device_layout, host_layout, mesh, operator_case

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ["quad", "hex"])
def test_dg_general_mesh_operators_and_steps(name, monkeypatch):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    guard_env(monkeypatch)
    oc = operator_case(name)
    d = mesh(name).dim
    n = oc["T"].size
    dev = device(name)
    dev.setup()
    dev.set_field("T", oc["T"])
    dev.set_field("T_prev", oc["Tp"])
    lib, ctx = dev._lib, dev._ctx
    checks = []

    def vec(values):
        view, ptr, check = guarded(device_layout(d, values), lead=1)
        checks.append(check)
        return view, ptr

    _, Td = vec(oc["T"])
    Fv, Fd = vec(np.zeros(n))
    assert lib.tv_residual(ctx, Td, Fd) == 0
    _, xd = vec(oc["x"])
    yv, yd = vec(np.zeros(n))
    assert lib.tv_jacobian_apply(ctx, xd, yd) == 0
    dv, dd = vec(np.zeros(n))
    assert lib.tv_jacobian_diag(ctx, dd) == 0
    F, Jx, diag = (host_layout(d, v.cpu().numpy()) for v in (Fv, yv, dv))
    dev._set_initial_condition(dev.material_model.T_init)
    for _ in range(2):
        dev.solve_timestep()
    T = np.array(dev.functions_current["T"].x.array)
    assert_guards_intact(lib)
    for check in checks:
        check()
    dev.close()
    assert np.all(np.isfinite(T))
    assert relerr(F, oc["F"]) < 1e-12
    assert relerr(Jx, oc["J"] @ oc["x"]) < 1e-12
    assert relerr(diag, oc["diag"]) < 1e-12
