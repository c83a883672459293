"""The interface of the multi-vector products with the float copy of the values, without a GPU: the three entry
points are declared and exported, the Python names exist, a host-only matrix and a NULL handle refuse both products
(group -1), and Matrix.matmat_f32 / matmat_rm_f32 check their tensors like matmat / matmat_rm before the library is
called."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

import sparsex_amd as sx
from helpers import ROOT
import matmat_cases as mc

NAMES = ("spx_hip_matmat_kernel_f32", "spx_hip_matmat_rm_kernel_f32", "spx_hip_matmat_group_f32")
PYTHON_NAMES = ("hip_matmat_kernel_f32", "hip_matmat_rm_kernel_f32", "matmat_f32", "matmat_rm_f32", "matmat_group_f32")
NR, NC = 300, 800
MATMAT_ARGS = [C.c_double, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_double, C.c_void_p, C.c_size_t, C.c_void_p]


def test_entry_points_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "sparsex_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", sx.lib_path()], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name + " is not declared in sparsex_hip.h"
        assert name in exported, name + " is not exported by libsparsex.so"


def test_python_names_exist():
    for name in PYTHON_NAMES:
        assert callable(getattr(sx.Matrix, name, None)), "Matrix." + name


def test_abi_version_did_not_move():
    """(the info struct did not grow)"""
    hdr = open(os.path.join(ROOT, "include", "sparsex_hip.h")).read()
    assert int(re.search(r"#define\s+SPX_HIP_ABI_VERSION\s+(\d+)", hdr).group(1)) == sx.lib().spx_hip_abi_version()


@pytest.fixture(scope="module")
def host_matrix():
    csr, m = mc.band(NR, 40, 0.2, ncols=NC)
    A = mc.load_rect(sx, csr, NC, dict(mc.NOSAMPLE, **{"spx.gpu.values_f32": "true"}), host_only=True)
    assert (A.nrows, A.ncols) == (NR, NC)
    yield A
    sx.options_reset()


def _raw():
    L = sx.lib()
    for f in (L.spx_hip_matmat_kernel_f32, L.spx_hip_matmat_rm_kernel_f32):
        f.restype = C.c_int
        f.argtypes = MATMAT_ARGS
    L.spx_hip_matmat_group_f32.restype = C.c_int
    L.spx_hip_matmat_group_f32.argtypes = [C.c_void_p]
    return L


def test_host_only_matrix_refuses(host_matrix):
    A = host_matrix
    L = _raw()
    x, y = 1 << 40, 1 << 41                 # (never dereferenced: the handle is refused first)
    assert L.spx_hip_matmat_kernel_f32(1.0, A.handle, 2, x, NC, 0.0, y, NR, None) == sx.SPX_FAILURE
    assert L.spx_hip_matmat_rm_kernel_f32(1.0, A.handle, 2, x, 2, 0.0, y, 2, None) == sx.SPX_FAILURE
    # (nvec == 0 does nothing only where there is a product at all)
    assert L.spx_hip_matmat_kernel_f32(1.0, A.handle, 0, None, NC, 0.0, None, NR, None) == sx.SPX_FAILURE
    assert L.spx_hip_matmat_rm_kernel_f32(1.0, A.handle, 0, None, 0, 0.0, None, 0, None) == sx.SPX_FAILURE
    with pytest.raises(sx.SpxError):
        A.hip_matmat_kernel_f32(1.0, x, NC, 2, 0.0, y, NR)
    with pytest.raises(sx.SpxError):
        A.hip_matmat_rm_kernel_f32(1.0, x, 2, 2, 0.0, y, 2)
    assert A.matmat_group_f32() == -1
    assert L.spx_hip_matmat_group_f32(A.handle) == -1


def test_null_handle():
    L = _raw()
    assert L.spx_hip_matmat_group_f32(None) == -1
    assert L.spx_hip_matmat_kernel_f32(1.0, None, 2, 1 << 40, NC, 0.0, 1 << 41, NR, None) == sx.SPX_FAILURE
    assert L.spx_hip_matmat_rm_kernel_f32(1.0, None, 2, 1 << 40, 2, 0.0, 1 << 41, 2, None) == sx.SPX_FAILURE


def _bad_calls():
    """name -> (method, X, Y, what the message names): the checks of matmat and matmat_rm"""
    f64 = torch.float64
    return {
        "cm cpu": ("matmat_f32", torch.zeros(2, NC, dtype=f64), torch.zeros(2, NR, dtype=f64), "device"),
        "cm float32": ("matmat_f32", torch.zeros(2, NC, dtype=torch.float32), torch.zeros(2, NR, dtype=f64), "float64"),
        "cm shape": ("matmat_f32", torch.zeros(2, NR, dtype=f64), torch.zeros(2, NR, dtype=f64), "shape"),
        "cm counts": ("matmat_f32", torch.zeros(2, NC, dtype=f64), torch.zeros(3, NR, dtype=f64), "vectors"),
        "cm stride": ("matmat_f32", torch.zeros(2, 2 * NC, dtype=f64)[:, ::2], torch.zeros(2, NR, dtype=f64), "stride"),
        "cm not a tensor": ("matmat_f32", [[0.0] * NC], torch.zeros(1, NR, dtype=f64), "tensor"),
        "rm cpu": ("matmat_rm_f32", torch.zeros(NC, 2, dtype=f64), torch.zeros(NR, 2, dtype=f64), "device"),
        "rm float32": ("matmat_rm_f32", torch.zeros(NC, 2, dtype=f64), torch.zeros(NR, 2, dtype=torch.float32), "float64"),
        "rm shape": ("matmat_rm_f32", torch.zeros(2, NC, dtype=f64), torch.zeros(2, NR, dtype=f64), "shape"),
        "rm counts": ("matmat_rm_f32", torch.zeros(NC, 2, dtype=f64), torch.zeros(NR, 3, dtype=f64), "vectors"),
        "rm stride": ("matmat_rm_f32", torch.zeros(NC, 4, dtype=f64)[:, ::2], torch.zeros(NR, 2, dtype=f64), "stride"),
        "rm not a tensor": ("matmat_rm_f32", torch.zeros(NC, 1, dtype=f64), [[0.0]] * NR, "tensor"),
    }


@pytest.mark.parametrize("case", list(_bad_calls().keys()))
def test_tensor_checks_are_those_of_the_fp64_calls(host_matrix, case):
    method, X, Y, what = _bad_calls()[case]
    fp64 = method[:-len("_f32")]
    for name in (method, fp64):
        if isinstance(Y, torch.Tensor):
            Y.fill_(7.0)
        with pytest.raises(ValueError, match=what):
            getattr(host_matrix, name)(1.0, X, 0.0, Y)
        if isinstance(Y, torch.Tensor):
            assert bool((Y == 7.0).all())
