"""The interface of the product with a float copy of the values (spx.gpu.values_f32) without a GPU: the four entry
points are declared and exported, a host-only matrix refuses the products (bytes -1), Matrix.matvec_f32 checks its
tensors before the library is called, an unknown option value fails the tune, the saved file does not depend on the
option, and the ABI version stays 5."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

import sparsex_amd as sx
from helpers import ROOT
import matmat_cases as mc

NAMES = ("spx_hip_matvec_mult_f32", "spx_hip_matvec_kernel_f32", "spx_hip_matvec_kernel_f32_vec",
         "spx_hip_mat_values_f32_bytes")
OPT = "spx.gpu.values_f32"
NR, NC = 300, 800


def test_entry_points_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "sparsex_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", sx.lib_path()], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name + " is not declared in sparsex_hip.h"
        assert name in exported, name + " is not exported by libsparsex.so"
    for name in ("matvec_f32", "hip_matvec_kernel_f32", "values_f32_bytes"):
        assert callable(getattr(sx.Matrix, name))
    assert callable(sx.matvec_kernel_f32_vec)


def test_abi_version_stays_5():
    L = sx.lib()
    L.spx_hip_abi_version.restype = C.c_int
    assert L.spx_hip_abi_version() == 5


@pytest.fixture(scope="module")
def host_matrix():
    """300 x 800, host-only, tuned with the option on: x of a product has 800 elements, y 300."""
    csr, m = mc.band(NR, 40, 0.2, ncols=NC)
    A = mc.load_rect(sx, csr, NC, dict(mc.NOSAMPLE, **{OPT: "true"}), host_only=True)
    assert (A.nrows, A.ncols) == (NR, NC)
    yield A
    sx.options_reset()


def test_host_only_matrix_refuses(host_matrix):
    A = host_matrix
    L = sx.lib()
    assert L.spx_hip_matvec_kernel_f32(1.0, A.handle, 8, 0.0, 1 << 40, None) == sx.SPX_FAILURE
    assert L.spx_hip_matvec_mult_f32(1.0, A.handle, 8, 1 << 40, None) == sx.SPX_FAILURE
    # (the vector handles are looked at first: two that say they are of the right sizes are not needed to be refused)
    assert L.spx_hip_matvec_kernel_f32_vec(1.0, A.handle, None, 0.0, None, None) == sx.SPX_FAILURE
    with pytest.raises(sx.SpxError):
        A.hip_matvec_kernel_f32(1.0, 8, 0.0, 1 << 40)
    assert A.values_f32_bytes() == -1
    assert L.spx_hip_mat_values_f32_bytes(None) == -1


def test_null_arguments():
    L = sx.lib()
    assert L.spx_hip_matvec_kernel_f32(1.0, None, 8, 0.0, 1 << 40, None) == sx.SPX_FAILURE
    assert L.spx_hip_matvec_mult_f32(1.0, None, 8, 1 << 40, None) == sx.SPX_FAILURE
    assert L.spx_hip_matvec_kernel_f32_vec(1.0, None, None, 0.0, None, None) == sx.SPX_FAILURE


def test_null_vectors(host_matrix):
    L = sx.lib()
    A = host_matrix
    assert L.spx_hip_matvec_kernel_f32(1.0, A.handle, None, 0.0, 1 << 40, None) == sx.SPX_FAILURE
    assert L.spx_hip_matvec_kernel_f32(1.0, A.handle, 8, 0.0, None, None) == sx.SPX_FAILURE
    assert L.spx_hip_matvec_mult_f32(1.0, A.handle, 8, None, None) == sx.SPX_FAILURE


def _bad_calls():
    f64 = torch.float64
    return {
        "cpu": (torch.zeros(NC, dtype=f64), torch.zeros(NR, dtype=f64), "device"),
        "float32": (torch.zeros(NC, dtype=torch.float32), torch.zeros(NR, dtype=f64), "float64"),
        "float32 y": (torch.zeros(NC, dtype=f64), torch.zeros(NR, dtype=torch.float32), "float64"),
        "2-D": (torch.zeros(1, NC, dtype=f64), torch.zeros(1, NR, dtype=f64), "shape"),
        "x of nrows": (torch.zeros(NR, dtype=f64), torch.zeros(NR, dtype=f64), "shape"),
        "y of ncols": (torch.zeros(NC, dtype=f64), torch.zeros(NC, dtype=f64), "shape"),
        "transposed lengths": (torch.zeros(NR, dtype=f64), torch.zeros(NC, dtype=f64), "shape"),
        "strided x": (torch.zeros(2 * NC, dtype=f64)[::2], torch.zeros(NR, dtype=f64), "stride"),
        "strided y": (torch.zeros(NC, dtype=f64), torch.zeros(2 * NR, dtype=f64)[::2], "stride"),
        "not a tensor": ([0.0] * NC, torch.zeros(NR, dtype=f64), "tensor"),
    }


@pytest.mark.parametrize("case", list(_bad_calls().keys()))
def test_matvec_f32_rejects_bad_tensors(host_matrix, case):
    x, y, what = _bad_calls()[case]
    y.fill_(7.0)
    y_before = y.clone()
    with pytest.raises(ValueError, match=what):
        host_matrix.matvec_f32(1.0, x, 0.0, y)
    assert torch.equal(y, y_before)


@pytest.mark.parametrize("value", ["true", "false"])
def test_known_option_values_tune(value):
    csr, m = mc.band(NR, 40, 0.2, ncols=NC)
    A = mc.load_rect(sx, csr, NC, dict(mc.NOSAMPLE, **{OPT: value}), host_only=True)
    assert A.values_f32_bytes() == -1
    A.destroy()
    sx.options_reset()


@pytest.mark.parametrize("value", ["yes", "2", ""])
def test_unknown_option_value_fails_the_tune(value):
    csr, m = mc.band(NR, 40, 0.2, ncols=NC)
    try:
        with pytest.raises(sx.SpxError):
            mc.load_rect(sx, csr, NC, dict(mc.NOSAMPLE, **{OPT: value}), host_only=True)
    finally:
        sx.options_reset()


def test_saved_file_does_not_depend_on_the_option(tmp_path):
    csr, m = mc.band(NR, 40, 0.2, ncols=NC)
    blobs = []
    for value in ("false", "true"):
        A = mc.load_rect(sx, csr, NC, dict(mc.NOSAMPLE, **{OPT: value}), host_only=True)
        f = str(tmp_path / (value + ".spx"))
        A.save(f)
        A.destroy()
        blobs.append(open(f, "rb").read())
    sx.options_reset()
    assert len(blobs[0]) > 0 and blobs[0] == blobs[1]
