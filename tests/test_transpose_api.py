"""The transposed product's interface without a GPU: the four entry points are declared and exported, a
host-only matrix refuses them (mode -1), Matrix.matvec_trans checks its tensors before the library is called,
and an unknown spx.gpu.trans_windows value fails the tune."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

import sparsex_amd as sx
from helpers import ROOT
import matmat_cases as mc

NAMES = ("spx_hip_matvec_trans_mult", "spx_hip_matvec_trans_kernel", "spx_hip_matvec_trans_kernel_vec",
         "spx_hip_matvec_trans_mode")
NR, NC = 300, 800


def test_entry_points_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "sparsex_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", sx.lib_path()], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name + " is not declared in sparsex_hip.h"
        assert name in exported, name + " is not exported by libsparsex.so"


@pytest.fixture(scope="module")
def host_matrix():
    """300 x 800, host-only: x of a transposed product has 300 elements, y 800."""
    csr, m = mc.band(NR, 40, 0.2, ncols=NC)
    A = mc.load_rect(sx, csr, NC, mc.NOSAMPLE, host_only=True)
    assert (A.nrows, A.ncols) == (NR, NC)
    yield A
    sx.options_reset()


def test_host_only_matrix_refuses(host_matrix):
    A = host_matrix
    L = sx.lib()
    assert L.spx_hip_matvec_trans_kernel(1.0, A.handle, 8, 0.0, 1 << 40, None) == sx.SPX_FAILURE
    assert L.spx_hip_matvec_trans_mult(1.0, A.handle, 8, 1 << 40, None) == sx.SPX_FAILURE
    with pytest.raises(sx.SpxError):
        A.hip_matvec_trans_kernel(1.0, 8, 0.0, 1 << 40)
    assert A.trans_mode() == -1
    assert L.spx_hip_matvec_trans_mode(None) == -1


def test_null_arguments():
    L = sx.lib()
    assert L.spx_hip_matvec_trans_kernel(1.0, None, 8, 0.0, 1 << 40, None) == sx.SPX_FAILURE
    assert L.spx_hip_matvec_trans_mult(1.0, None, 8, 1 << 40, None) == sx.SPX_FAILURE
    assert L.spx_hip_matvec_trans_kernel_vec(1.0, None, None, 0.0, None, None) == sx.SPX_FAILURE


def _bad_calls():
    f64 = torch.float64
    return {
        "cpu": (torch.zeros(NR, dtype=f64), torch.zeros(NC, dtype=f64), "device"),
        "float32": (torch.zeros(NR, dtype=torch.float32), torch.zeros(NC, dtype=f64), "float64"),
        "float32 y": (torch.zeros(NR, dtype=f64), torch.zeros(NC, dtype=torch.float32), "float64"),
        "2-D": (torch.zeros(1, NR, dtype=f64), torch.zeros(1, NC, dtype=f64), "shape"),
        "x of ncols": (torch.zeros(NC, dtype=f64), torch.zeros(NC, dtype=f64), "shape"),
        "y of nrows": (torch.zeros(NR, dtype=f64), torch.zeros(NR, dtype=f64), "shape"),
        "forward lengths": (torch.zeros(NC, dtype=f64), torch.zeros(NR, dtype=f64), "shape"),
        "strided x": (torch.zeros(2 * NR, dtype=f64)[::2], torch.zeros(NC, dtype=f64), "stride"),
        "strided y": (torch.zeros(NR, dtype=f64), torch.zeros(2 * NC, dtype=f64)[::2], "stride"),
        "not a tensor": ([0.0] * NR, torch.zeros(NC, dtype=f64), "tensor"),
    }


@pytest.mark.parametrize("case", list(_bad_calls().keys()))
def test_matvec_trans_rejects_bad_tensors(host_matrix, case):
    x, y, what = _bad_calls()[case]
    y.fill_(7.0)
    y_before = y.clone()
    with pytest.raises(ValueError, match=what):
        host_matrix.matvec_trans(1.0, x, 0.0, y)
    assert torch.equal(y, y_before)


@pytest.mark.parametrize("value", ["true", "false", "auto"])
def test_known_option_values_tune(value):
    csr, m = mc.band(NR, 40, 0.2, ncols=NC)
    A = mc.load_rect(sx, csr, NC, dict(mc.NOSAMPLE, **{"spx.gpu.trans_windows": value}), host_only=True)
    assert A.trans_mode() == -1
    A.destroy()
    sx.options_reset()


@pytest.mark.parametrize("value", ["yes", "2", ""])
def test_unknown_option_value_fails_the_tune(value):
    csr, m = mc.band(NR, 40, 0.2, ncols=NC)
    try:
        with pytest.raises(sx.SpxError):
            mc.load_rect(sx, csr, NC, dict(mc.NOSAMPLE, **{"spx.gpu.trans_windows": value}), host_only=True)
    finally:
        sx.options_reset()
