"""The interface of the norms and the scaling D * A * D of a matrix tuned as a symmetric one, without a GPU: the
four entry points are declared and exported, the Python names exist, the header states the semantics, and refusals --
a general tune, a bad kind, bad operands, the device forms on a host-only matrix -- leave the outputs and the saved
stream untouched."""
import os
import re
import subprocess

import numpy as np
import pytest

import sparsex_amd as sx
from sparsex_amd.api import SpxError
from helpers import ROOT

import scale_cases as sc
import values_cases as vc
from diag_cases import matrix, bits

NAMES = ("spx_hip_mat_sym_norms", "spx_hip_mat_sym_norms_host", "spx_hip_mat_sym_scale", "spx_hip_mat_sym_scale_host")


def _header():
    return open(os.path.join(ROOT, "include", "sparsex_hip.h")).read()


def test_entry_points_declared_and_exported():
    hdr = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", sx.lib_path()], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name + " is not declared in sparsex_hip.h"
        assert name in exported, name + " is not exported by libsparsex.so"
    assert re.search(r"#define\s+SPX_HIP_ABI_VERSION\s+5\b", _header()) and sx.lib().spx_hip_abi_version() == 5


def test_python_names():
    for name in ("sym_norms", "sym_norms_host", "sym_scale", "hip_mat_sym_norms", "hip_mat_sym_scale"):
        assert callable(getattr(sx.Matrix, name)), name


def test_header_states_the_semantics():
    hdr = " ".join(_header().split())
    for phrase in ("d[max(r,c)]", "d[min(r,c)]", "all-reduces", "not bit-reproducible", "legal during stream capture",
                   "counts for its row and for its column", "gets the bits of its lower copy", "row == column",
                   "tuned as a general one", "exchange plan attached", "tuned as a symmetric one"):
        assert phrase in hdr, phrase


def test_refusals_leave_everything_alone(tmp_path, capfd):
    csr = matrix("nlpkkt")
    n = csr[3]
    L = sx.lib()
    d = sc.vector(n, 1)
    out = np.full(n, sc.SENTINEL)

    def untouched():
        return (out == sc.SENTINEL).all()

    # a NULL handle
    assert L.spx_hip_mat_sym_norms(None, 0, out.ctypes.data, None) == sx.SPX_FAILURE
    assert L.spx_hip_mat_sym_norms_host(None, 0, out.ctypes.data) == sx.SPX_FAILURE
    assert L.spx_hip_mat_sym_scale(None, d.ctypes.data, None) == sx.SPX_FAILURE
    assert L.spx_hip_mat_sym_scale_host(None, d.ctypes.data) == sx.SPX_FAILURE
    # a general tune, host-only: all four refuse and name the entry points that serve it
    G = vc.tune(csr, host_only=True)
    before = vc.decoded(G, tmp_path, "g0.spx")
    capfd.readouterr()
    with pytest.raises(SpxError):
        G.sym_norms_host(sx.NORM_MAX_ABS, out)
    with pytest.raises(SpxError):
        G.sym_scale(d)
    assert L.spx_hip_mat_sym_norms(G.handle, 0, out.ctypes.data, None) == sx.SPX_FAILURE
    assert L.spx_hip_mat_sym_scale(G.handle, d.ctypes.data, None) == sx.SPX_FAILURE
    err = capfd.readouterr().err
    assert "tuned as a general one" in err and "spx_hip_mat_scale(A, d, d)" in err
    assert untouched()
    assert np.array_equal(bits(vc.decoded(G, tmp_path, "g1.spx").values), bits(before.values))
    G.export_csx(G.info().first_partition)                      # nothing went stale
    G.destroy()
    # a symmetric tune, host-only: bad kinds, NULL vectors, the device forms
    S = vc.tune(csr, sym=True, host_only=True)
    before = vc.decoded(S, tmp_path, "s0.spx")
    capfd.readouterr()
    for kind in (-1, 3):
        assert L.spx_hip_mat_sym_norms_host(S.handle, kind, out.ctypes.data) == sx.SPX_FAILURE
        with pytest.raises(ValueError):
            S.sym_norms_host(kind, out)
    assert "kind" in capfd.readouterr().err
    assert L.spx_hip_mat_sym_norms_host(S.handle, 0, None) == sx.SPX_FAILURE
    assert L.spx_hip_mat_sym_scale_host(S.handle, None) == sx.SPX_FAILURE
    assert "NULL" in capfd.readouterr().err
    # (host addresses: a device form that went on would fault, it must refuse before it looks at them)
    assert L.spx_hip_mat_sym_norms(S.handle, 0, out.ctypes.data, None) == sx.SPX_FAILURE
    assert L.spx_hip_mat_sym_scale(S.handle, d.ctypes.data, None) == sx.SPX_FAILURE
    with pytest.raises(SpxError):
        S.hip_mat_sym_norms(sx.NORM_MAX_ABS, 8)
    with pytest.raises(SpxError):
        S.hip_mat_sym_scale(8)
    assert "host_only" in capfd.readouterr().err
    # operands of the Python methods, named before the library is called
    for bad in (np.zeros(n - 1), np.zeros(n, dtype=np.float32), np.zeros((n, 1)), np.zeros(2 * n)[::2]):
        with pytest.raises(ValueError, match="sym_scale"):
            S.sym_scale(bad)
        with pytest.raises(ValueError, match="sym_norms_host"):
            S.sym_norms_host(sx.NORM_SUM_ABS, bad)
    with pytest.raises(ValueError, match="d is None"):
        S.sym_scale(None)
    with pytest.raises(ValueError, match="DeviceVector or a torch tensor"):
        S.sym_scale([1.0] * n)
    with pytest.raises(ValueError, match="DeviceVector or a torch tensor"):
        S.sym_norms(sx.NORM_SUM_ABS, out)
    with pytest.raises(ValueError, match="kind"):
        S.sym_norms(7)
    assert untouched()
    after = vc.decoded(S, tmp_path, "s1.spx")
    assert np.array_equal(bits(after.values), bits(before.values)) and np.array_equal(bits(after.dvalues), bits(before.dvalues))
    S.export_csx(S.info().first_partition)                      # nothing went stale
    # the old entry points still refuse a symmetric tune, and say where to go
    with pytest.raises(SpxError):
        S.norms_host(sx.NORM_MAX_ABS)
    err = capfd.readouterr().err
    assert "symmetric" in err and "spx_hip_mat_sym_norms" in err
    S.destroy()
    sx.options_reset()
