"""The row-major multi-vector product's interface without a GPU: spx_hip_matmat_rm_kernel and
spx_hip_matmat_rm_group are declared and exported, a host-only matrix and a NULL handle refuse them, and
Matrix.matmat_rm checks its tensors before the library is called."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

import sparsex_amd as sx
from sparsex_amd import synth
from helpers import ROOT, tune

NAMES = ("spx_hip_matmat_rm_kernel", "spx_hip_matmat_rm_group")
ARGTYPES = [C.c_double, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_double, C.c_void_p, C.c_size_t, C.c_void_p]


def test_entry_points_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "sparsex_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", sx.lib_path()], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name + " is not declared in sparsex_hip.h"
        assert name in exported, name + " is not exported by libsparsex.so"


def test_abi_version_stays_5():
    L = sx.lib()
    L.spx_hip_abi_version.restype = C.c_int
    assert L.spx_hip_abi_version() == 5


@pytest.fixture(scope="module")
def host_matrix():
    csr = synth.syn_cant(0.02)
    A = tune(csr, {}, host_only=True)
    yield A, csr
    sx.options_reset()


def test_host_only_matrix_refuses(host_matrix):
    A, csr = host_matrix
    L = sx.lib()
    L.spx_hip_matmat_rm_kernel.restype = C.c_int
    L.spx_hip_matmat_rm_kernel.argtypes = ARGTYPES
    for nvec in (0, 1, 4):
        assert L.spx_hip_matmat_rm_kernel(1.0, A.handle, nvec, 8, 4, 0.0, 1 << 40, 4, None) == sx.SPX_FAILURE
    with pytest.raises(sx.SpxError):
        A.hip_matmat_rm_kernel(1.0, 8, 2, 2, 0.0, 1 << 40, 2)
    assert A.matmat_rm_group() == -1
    L.spx_hip_matmat_rm_group.restype = C.c_int
    L.spx_hip_matmat_rm_group.argtypes = [C.c_void_p]
    assert L.spx_hip_matmat_rm_group(None) == -1


def test_null_matrix_handle():
    L = sx.lib()
    L.spx_hip_matmat_rm_kernel.restype = C.c_int
    L.spx_hip_matmat_rm_kernel.argtypes = ARGTYPES
    assert L.spx_hip_matmat_rm_kernel(1.0, None, 1, 8, 1, 0.0, 1 << 40, 1, None) == sx.SPX_FAILURE


def _bad_calls(n):
    f64 = torch.float64
    return {
        "cpu": (torch.zeros(n, 2, dtype=f64), torch.zeros(n, 2, dtype=f64), "device"),
        "float32": (torch.zeros(n, 2, dtype=torch.float32), torch.zeros(n, 2, dtype=f64), "float64"),
        "float32 Y": (torch.zeros(n, 2, dtype=f64), torch.zeros(n, 2, dtype=torch.float32), "float64"),
        "1-D": (torch.zeros(n, dtype=f64), torch.zeros(n, dtype=f64), "shape"),
        "3-D": (torch.zeros(1, n, 2, dtype=f64), torch.zeros(1, n, 2, dtype=f64), "shape"),
        "short X": (torch.zeros(n - 1, 2, dtype=f64), torch.zeros(n, 2, dtype=f64), "shape"),
        "long Y": (torch.zeros(n, 2, dtype=f64), torch.zeros(n + 1, 2, dtype=f64), "shape"),
        "vector count": (torch.zeros(n, 3, dtype=f64), torch.zeros(n, 2, dtype=f64), "vectors"),
        "inner stride": (torch.zeros(n, 4, dtype=f64)[:, ::2], torch.zeros(n, 2, dtype=f64), "stride"),
        "inner stride Y": (torch.zeros(n, 2, dtype=f64), torch.zeros(n, 4, dtype=f64)[:, ::2], "stride"),
        "transposed": (torch.zeros(2, n, dtype=f64).t(), torch.zeros(n, 2, dtype=f64), "stride"),
        "not a tensor": ([[0.0] * 2] * n, torch.zeros(n, 2, dtype=f64), "tensor"),
    }


@pytest.mark.parametrize("case", list(_bad_calls(8).keys()))
def test_matmat_rm_rejects_bad_tensors(host_matrix, case):
    A, csr = host_matrix
    X, Y, what = _bad_calls(csr[3])[case]
    y_before = Y.clone() if isinstance(Y, torch.Tensor) else None
    with pytest.raises(ValueError, match=what):
        A.matmat_rm(1.0, X, 0.0, Y)
    if y_before is not None:
        assert torch.equal(Y, y_before)
