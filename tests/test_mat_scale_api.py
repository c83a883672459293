"""The interface of the norms and the diagonal scaling without a GPU: the entry points are declared and exported,
the ABI version did not move, the Python names and constants exist, and Matrix.norms / Matrix.scale /
Matrix.norms_host check their arguments, naming the one at fault, before the library is called."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import sparsex_amd as sx
from helpers import ROOT
import matmat_cases as mc

NAMES = ("spx_hip_mat_norms", "spx_hip_mat_norms_host", "spx_hip_mat_scale", "spx_hip_mat_scale_host", "spx_hip_vec_rsqrt")
NR, NC = 300, 800


def _header():
    return open(os.path.join(ROOT, "include", "sparsex_hip.h")).read()


def test_entry_points_declared_and_exported():
    hdr = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", sx.lib_path()], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name + " is not declared in sparsex_hip.h"
        assert name in exported, name + " is not exported by libsparsex.so"


def test_abi_version_and_constants():
    hdr = _header()
    assert re.search(r"#define\s+SPX_HIP_ABI_VERSION\s+5\b", hdr)
    assert sx.lib().spx_hip_abi_version() == 5
    for name, value in (("SUM_ABS", 0), ("SUM_SQ", 1), ("MAX_ABS", 2)):
        assert re.search(r"#define\s+SPX_HIP_NORM_%s\s+%d\b" % (name, value), hdr)
        assert getattr(sx, "NORM_" + name) == value


def test_python_names():
    for name in ("norms", "norms_host", "scale", "hip_mat_norms", "hip_mat_scale"):
        assert callable(getattr(sx.Matrix, name)), name
    assert callable(sx.DeviceVector.rsqrt)


def test_header_states_the_semantics():
    """the promises a caller relies on are written where the functions are declared"""
    hdr = " ".join(_header().split())
    for phrase in ("fl(fl(dr[r] * a) * dc[c])", "leaves the rest alone", "all-reduces", "+0.0", "not bit-reproducible",
                   "The max kind is exact", "legal during stream capture", "exchange plan attached",
                   "tuned as a symmetric one", "spx_hip_mat_export_csx then fails"):
        assert phrase in hdr, phrase


@pytest.fixture(scope="module")
def host_matrix():
    csr, m = mc.band(NR, 40, 0.2, ncols=NC)
    A = mc.load_rect(sx, csr, NC, mc.NOSAMPLE, host_only=True)
    assert (A.nrows, A.ncols) == (NR, NC)
    yield A
    sx.options_reset()


def test_host_only_matrix_refuses_the_device_forms(host_matrix):
    A = host_matrix
    L = sx.lib()
    assert L.spx_hip_mat_norms(A.handle, 0, 8, 1 << 40, None) == sx.SPX_FAILURE
    assert L.spx_hip_mat_scale(A.handle, 8, 1 << 40, None) == sx.SPX_FAILURE
    with pytest.raises(sx.SpxError):
        A.hip_mat_norms(sx.NORM_MAX_ABS, 8, None)
    with pytest.raises(sx.SpxError):
        A.hip_mat_scale(8, None)
    assert L.spx_hip_vec_rsqrt(None, None, 0.0, None) == sx.SPX_FAILURE


def _bad_tensors():
    f64 = torch.float64
    return {
        # name of the operand at fault, (rows | dr, cols | dc), what the message says
        "cpu rows": ("rows|dr", (torch.zeros(NR, dtype=f64), None), "device"),
        "cpu cols": ("cols|dc", (None, torch.zeros(NC, dtype=f64)), "device"),
        "float32 rows": ("rows|dr", (torch.zeros(NR, dtype=torch.float32), None), "float64"),
        "float32 cols": ("cols|dc", (None, torch.zeros(NC, dtype=torch.float32)), "float64"),
        "2-D": ("rows|dr", (torch.zeros(1, NR, dtype=f64), None), "shape"),
        "rows of ncols": ("rows|dr", (torch.zeros(NC, dtype=f64), None), "shape"),
        "cols of nrows": ("cols|dc", (None, torch.zeros(NR, dtype=f64)), "shape"),
        "strided rows": ("rows|dr", (torch.zeros(2 * NR, dtype=f64)[::2], None), "stride"),
        "strided cols": ("cols|dc", (None, torch.zeros(2 * NC, dtype=f64)[::2]), "stride"),
        "a list": ("rows|dr", ([0.0] * NR, None), "DeviceVector or a torch tensor"),
    }


@pytest.mark.parametrize("case", list(_bad_tensors()))
def test_norms_and_scale_reject_bad_tensors(host_matrix, case):
    name, (a, b), what = _bad_tensors()[case]
    for call in (lambda: host_matrix.norms(sx.NORM_MAX_ABS, a, b), lambda: host_matrix.scale(a, b)):
        with pytest.raises(ValueError, match=what) as e:
            call()
        assert re.search(r"\b(%s)\b" % name, str(e.value)), str(e.value)


def test_norms_and_scale_reject_bad_calls(host_matrix):
    A = host_matrix
    with pytest.raises(ValueError, match="kind"):
        A.norms(3, torch.zeros(NR, dtype=torch.float64), None)
    with pytest.raises(ValueError, match="kind"):
        A.norms_host(-1)
    with pytest.raises(ValueError, match="both None"):
        A.norms(sx.NORM_SUM_ABS)
    with pytest.raises(ValueError, match="both None"):
        A.scale()
    with pytest.raises(ValueError, match="both False"):
        A.norms_host(sx.NORM_SUM_ABS, False, False)
    # the host path of scale: numpy arrays, both of them
    ok_r, ok_c = np.ones(NR), np.ones(NC)
    for dr, dc, what in ((np.ones(NR, np.float32), None, "dr must be float64"), (ok_r, np.ones(NR), r"dc must have the shape \(800,\)"),
                         (np.ones((1, NR)), None, r"dr must have the shape \(300,\)"), (np.ones(2 * NR)[::2], None, "dr must be contiguous"),
                         (ok_r, torch.zeros(NC, dtype=torch.float64), "dc must be a numpy array"),
                         (torch.zeros(NR, dtype=torch.float64), ok_c, "dr must be a numpy array")):
        with pytest.raises(ValueError, match=what):
            A.scale(dr, dc)
    for rows, cols, what in ((np.ones(NC), None, "rows must be a contiguous float64 array of 300"),
                             (None, np.ones(NC, np.float32), "cols must be a contiguous float64 array of 800"),
                             ([0.0] * NR, None, "rows must be")):
        with pytest.raises(ValueError, match=what):
            A.norms_host(sx.NORM_SUM_ABS, rows, cols)
    # nothing above reached the matrix
    rows, cols = A.norms_host(sx.NORM_MAX_ABS)
    A.scale(ok_r, ok_c)
    again = A.norms_host(sx.NORM_MAX_ABS)
    assert np.array_equal(rows, again[0]) and np.array_equal(cols, again[1])
