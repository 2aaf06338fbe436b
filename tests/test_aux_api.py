"""CPU: the public names of the auxiliary-space multigrid (TV_PC_AUX, DG1 temperature
on unstructured meshes): the header's value, the ABI version it leaves alone (one
additive enum value, no struct moves), the ctypes constant and the Python option."""
import os
import re

import pytest

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "tvfem.h")


def test_header_defines_the_value_and_keeps_the_abi():
    text = open(HEADER).read()
    assert re.search(r"^#define\s+TV_PC_AUX\s+3\b", text, re.M)
    assert re.search(r"^#define\s+TV_ABI_VERSION\s+8\b", text, re.M)
    assert re.search(r"^#define\s+TV_PC_AMG\s+2\b", text, re.M)


def test_native_constant():
    from tvfem import _native as N
    assert N.TV_PC_AUX == 3
    assert (N.TV_PC_JACOBI, N.TV_PC_GMG, N.TV_PC_AMG) == (0, 1, 2)


def test_unknown_preconditioner_names_aux():
    import numpy as np
    from oracle import tv_oracle as O
    from tvfem import RectilinearMesh
    from tvfem.problem import ThermoViscoProblem
    cg = {"element": "CG", "degree": 1}
    with pytest.raises(ValueError) as ei:
        ThermoViscoProblem(RectilinearMesh([np.linspace(0.0, 1.0, 3)]), (0.0, 1.0), 0.1, {"T": cg, "sigma": cg},
                           dict(O.MAIN_MODEL_PARAMS), verbose=False, preconditioner="nonsense")
    assert "'aux'" in str(ei.value)
