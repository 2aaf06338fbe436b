"""Red zones around the auxiliary-space multigrid of the DG general-mesh path
(TV_PC_AUX: csrc/tv_umdg_aux.hip, csrc/tv_amg.cpp aux_setup), built on
tests/guard_util.py as tests/test_guard_bands_umdg.py: every device allocation of
the context between filled guards (TVFEM_ALLOC_GUARD), the caller's vectors of
tv_precond_apply inside NaN arenas at an 8-byte aligned, not 16-byte aligned
address; then two coupled steps.  No guard byte may change, and the cycle still
meets the 1e-10 bar against the numpy restatement (tests/dg_aux_reference.py), so
no guard NaN has been read in through a padding lane of the incidence or block
tables.  "quad" and "hex": 72 and 140 cells, 90 and 240 vertices -- the last
64-item group of every table partly padding.
"""
import numpy as np
import pytest

from dg_aux_reference import AuxCycle
from guard_util import assert_guards_intact, guard_env, guarded
from parity_util import relerr
from test_unstructured_dg import device, device_layout, host_layout, mesh

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ["quad", "hex"])
def test_aux_cycle_and_steps_stay_inside_their_allocations(name, monkeypatch):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    guard_env(monkeypatch)
    d = mesh(name).dim
    n = mesh(name).num_cells * 2 ** d
    rng = np.random.default_rng(5)
    T = 700.0 + rng.uniform(0.0, 150.0, n)
    r = rng.standard_normal(n)
    dev = device(name, preconditioner="aux")
    dev.setup()
    dev.set_field("T", T)
    dev._flush()
    lib, ctx = dev._lib, dev._ctx
    _, rd, check_r = guarded(device_layout(d, r), lead=1)
    zv, zd, check_z = guarded(np.zeros(n), lead=1)
    assert lib.tv_precond_apply(ctx, rd, zd) == 0, lib.tv_last_error(ctx)
    z = host_layout(d, zv.cpu().numpy())
    dev._set_initial_condition(dev.material_model.T_init)
    for _ in range(2):
        dev.solve_timestep()
    T_end = np.array(dev.functions_current["T"].x.array)
    assert_guards_intact(lib)
    check_r()
    check_z()
    dev.close()
    e = relerr(z, AuxCycle(name, T).apply(r))
    print(f"[guard] aux cycle {name}: vs numpy {e:.2e}")
    assert np.all(np.isfinite(T_end))
    assert e <= 1e-10, e
