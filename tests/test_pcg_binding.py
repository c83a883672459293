"""The diagonal and Jacobi-PCG entry points through every layer that needs no GPU: exported by libsparsex.so,
declared in include/sparsex_hip.h, bound in sparsex_amd/api.py; and the C example compiles as strict C."""
import os
import re
import subprocess

import pytest

import sparsex_amd as sx
from sparsex_amd import api
from helpers import ROOT

SYMBOLS = [
    "spx_hip_mat_diag_plan", "spx_hip_mat_diag_plan_drop", "spx_hip_mat_get_diag", "spx_hip_mat_get_diag_vec",
    "spx_hip_mat_get_diag_host", "spx_hip_mat_diag_plan_get", "spx_hip_vec_mul_elem", "spx_hip_vec_reciprocal",
    "spx_hip_vec_pcg_update", "spx_hip_vec_pcg_direction",
]
# arguments of the prototype, the hipStream_t included
ARGS = dict(zip(SYMBOLS, [1, 1, 3, 3, 2, 2, 4, 4, 10, 5]))


@pytest.mark.parametrize("name", SYMBOLS)
def test_symbol_is_exported_declared_and_bound(name):
    fn = getattr(sx.lib(), name)                      # AttributeError: not exported
    assert fn.argtypes is not None and len(fn.argtypes) == ARGS[name], "no argtypes in api.lib()"
    with open(os.path.join(ROOT, "include", "sparsex_hip.h")) as f:
        header = f.read()
    m = re.search(r"^spx_error_t %s\(([^;]*)\);" % name, header, re.M)
    assert m, "no prototype in sparsex_hip.h"
    assert m.group(1).count(",") + 1 == ARGS[name]
    with open(api.__file__) as f:
        assert len(re.findall(r"\b%s\b" % name, f.read())) >= 2      # argtypes and a caller


def test_python_surface():
    for meth in ("diag_plan", "diag_plan_drop", "diag_plan_info", "get_diag", "get_diag_host"):
        assert callable(getattr(sx.Matrix, meth))
    for meth in ("mul_elem_into", "reciprocal_into"):
        assert callable(getattr(sx.DeviceVector, meth))
    assert callable(sx.pcg_update) and callable(sx.pcg_direction)
    assert "spx_hip_diag_plan_t" in open(os.path.join(ROOT, "include", "sparsex_hip.h")).read()


def test_c_example_compiles_as_strict_c(tmp_path):
    subprocess.check_call(["gcc", "-std=gnu99", "-Wall", "-Werror", "-c", os.path.join(ROOT, "examples", "pcg_device.c"),
                           "-I" + os.path.join(ROOT, "include"), "-o", str(tmp_path / "pcg_device.o")])
