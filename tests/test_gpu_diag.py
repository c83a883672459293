"""The diagonal of a tuned matrix read in HBM (spx_hip_mat_get_diag / _vec / _host, csx_gather_diag_kernel): bit
for bit the diagonal of the untuned CSR arrays in the tuned numbering, from the values as they are now -- after a
bulk update from a device array, after spx_mat_set_entry, inside a captured graph."""
import numpy as np
import pytest

import sparsex_amd as sx
from sparsex_amd.api import SpxError

import dist_cases as dc
import values_cases as vc
from diag_cases import SENTINEL, NCOLS, matrix, bits, stored_diag, expect, padded

pytestmark = pytest.mark.gpu

W4 = {"spx.gpu.waves": "4"}
# name -> (matrix, symmetric, options, reorder)
CASES = {
    "default": ("cant", False, {}, False),
    "deterministic": ("cant", False, {"spx.gpu.deterministic": "true"}, False),
    "slices-c2": ("cant", False, {"spx.gpu.col_phases": "c2"}, False),
    "unit-windows": ("cant", False, {"spx.gpu.unit_windows": "true"}, False),
    "values-f32": ("cant", False, {"spx.gpu.values_f32": "true"}, False),
    "values-f32-all": ("cant", True, {"spx.gpu.values_f32": "all"}, False),
    "nlpkkt": ("nlpkkt", False, {}, False),
    "webbase": ("webbase", False, {}, False),          # nearly every row without a diagonal entry
    "rect": ("rect", False, {}, False),                # rows >= ncols
    "rect-t": ("rect-t", False, {}, False),
    "symmetric": ("cant", True, {}, False),
    "sym-mirrored": ("cant", True, {"spx.gpu.sym_once": "false"}, False),
    "reorder": ("cant", False, {}, True),
    "sym-reorder": ("cant", True, {}, True),
}


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.float64)).cuda()


def sentinels(n):
    return sx.DeviceVector(host=np.full(n, SENTINEL))


def wanted(csr, A, perm=None, row0=0):
    inf = A.info()
    has, val = padded(*stored_diag(csr, row0=row0), A.nrows)
    return expect(has, val, inf.row_lo, inf.row_hi, perm)[0]


def read_all_ways(A, want):
    """into a vector, into an 8-byte aligned pointer in the middle of a longer vector, and to the host"""
    n = A.nrows
    d = A.get_diag(sentinels(n))
    assert np.array_equal(bits(d.download()), bits(want))
    long = sentinels(n + 3)
    A.hip_get_diag(long.data_ptr() + 8)
    got = long.download()
    assert np.array_equal(bits(got[1:n + 1]), bits(want))
    assert got[0] == SENTINEL and got[n + 1] == SENTINEL and got[n + 2] == SENTINEL
    assert np.array_equal(bits(A.get_diag_host(np.full(n, SENTINEL))), bits(want))


def updates(A, csr, sym, want, perm=None, row0=0):
    """new values from a device array (one diagonal entry -0.0), then one spx_mat_set_entry"""
    inf = A.info()
    lo, hi = inf.row_lo, inf.row_hi
    A.values_plan(csr[0], csr[1])
    v1 = vc.new_values(csr, sym, 13, row0=row0)
    r, c = vc.coords(csr)
    tr = (r + row0) if perm is None else perm[r + row0]
    on = np.flatnonzero((r + row0 == c) & (tr >= lo) & (tr < hi))
    v1[on[on.size // 2]] = -0.0
    A.set_values(dev(v1))
    want1 = wanted(vc.with_values(csr, v1), A, perm, row0)
    assert not np.array_equal(bits(want1), bits(want))
    read_all_ways(A, want1)
    k = on[0]
    cr = int(r[k] + row0)
    A.set_entry(cr, cr, 3.25)
    want1[int(tr[k])] = 3.25
    read_all_ways(A, want1)


@pytest.mark.parametrize("case", list(CASES))
def test_diagonal_of_a_matrix_in_hbm(case):
    name, sym, opts, reorder = CASES[case]
    csr = matrix(name)
    A = vc.tune(csr, dict(W4, **opts), sym=sym, reorder=reorder, ncols=NCOLS.get(name))
    inf = A.info()
    assert inf.on_device
    perm = A.get_perm().astype(np.int64) if reorder else None
    want = wanted(csr, A, perm)
    if sym:
        read_all_ways(A, want)                         # (no plan needed)
    A.diag_plan()
    info = A.diag_plan_info()
    assert info["plan_bytes"] == (0 if sym else 4 * A.nrows) and info["n_rows"] == A.nrows
    if case == "slices-c2":
        assert inf.col_slices == 2
    if case.startswith("values-f32"):
        assert A.values_f32_bytes() > 0
    read_all_ways(A, want)
    updates(A, csr, sym, want, perm)
    A.destroy()


@pytest.mark.parametrize("sym", [False, True])
@pytest.mark.parametrize("how", ["rank", "row-offset"])
def test_slice_one_of_three(how, sym):
    csr = matrix("nlpkkt")
    rp, ci, va, n = csr
    if how == "rank":
        A = dc.tune_rank(csr, 1, 3, dict(dc.NOSAMPLE, **W4), sym)
        part, row0 = csr, 0
    else:
        cuts = dc.cut(csr, 3, "balanced")
        lo, hi = cuts[1], cuts[2]
        A = dc.tune_rows(csr, lo, hi, dict(dc.NOSAMPLE, **W4), sym)
        part = ((rp[lo:hi + 1] - rp[lo]).astype(np.int32), ci[rp[lo]:rp[hi]].copy(), va[rp[lo]:rp[hi]].copy(), n)
        row0 = lo
    inf = A.info()
    assert 0 < inf.row_lo < inf.row_hi < n
    A.diag_plan()
    assert A.diag_plan_info()["plan_bytes"] == (0 if sym else 4 * (inf.row_hi - inf.row_lo))
    want = wanted(part, A, None, row0)
    assert (want[:inf.row_lo] == SENTINEL).all() and (want[inf.row_hi:] == SENTINEL).all()
    read_all_ways(A, want)
    updates(A, part, sym, want, None, row0)
    A.destroy()


@pytest.mark.parametrize("sym", [False, True])
def test_update_and_diagonal_in_one_captured_graph(sym):
    import torch
    csr = matrix("nlpkkt")
    A = vc.tune(csr, W4, sym=sym)
    A.values_plan(csr[0], csr[1])
    A.diag_plan()
    v = [vc.new_values(csr, sym, seed) for seed in (1, 2)]
    src = dev(v[0])
    d = sentinels(A.nrows)
    s = torch.cuda.current_stream().cuda_stream
    A.hip_set_values(src.data_ptr(), s)                    # warm-up outside the capture
    A.hip_get_diag(d.data_ptr(), s)
    torch.cuda.synchronize()
    d.init(SENTINEL)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = torch.cuda.current_stream().cuda_stream       # one stream, one chain: update, then diagonal
        A.hip_set_values(src.data_ptr(), cap)
        A.hip_get_diag(d.data_ptr(), cap)
    assert (d.download() == SENTINEL).all()                # (the capture ran nothing)
    for k in (0, 1, 0):
        src.copy_(dev(v[k]))                                # new numbers where the graph reads them
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(bits(d.download()), bits(wanted(vc.with_values(csr, v[k]), A)))
    A.destroy()


def test_restored_matrix_needs_a_new_plan(tmp_path):
    csr = matrix("nlpkkt")
    A = vc.tune(csr, W4)
    A.diag_plan()
    want = wanted(csr, A)
    f = str(tmp_path / "saved.spx")
    A.save(f)
    A.destroy()
    sx.options_reset()
    B = sx.mat_restore(f)
    assert B.info().on_device
    d = sentinels(B.nrows)
    with pytest.raises(SpxError):
        B.get_diag(d)
    B.diag_plan()
    read_all_ways(B, want)
    B.destroy()


def test_calls_that_must_fail(capfd):
    csr = matrix("nlpkkt")
    A = vc.tune(csr, W4)
    n = A.nrows
    d, short = sentinels(n), sentinels(n - 1)
    L = sx.lib()

    def untouched():
        return (d.download() == SENTINEL).all() and (short.download() == SENTINEL).all()

    with pytest.raises(SpxError):
        A.get_diag(d)                                  # a general matrix without a plan
    with pytest.raises(SpxError):
        A.hip_get_diag(d.data_ptr())
    with pytest.raises(SpxError):
        A.get_diag_host()
    assert "no diagonal plan" in capfd.readouterr().err
    A.diag_plan()
    with pytest.raises(SpxError):
        A.get_diag(short)                              # not nrows elements
    assert L.spx_hip_mat_get_diag(A.handle, None, None) == sx.SPX_FAILURE
    assert L.spx_hip_mat_get_diag(None, d.data_ptr(), None) == sx.SPX_FAILURE
    assert L.spx_hip_mat_get_diag_vec(A.handle, None, None) == sx.SPX_FAILURE
    assert L.spx_hip_mat_get_diag_vec(None, d.handle, None) == sx.SPX_FAILURE
    assert L.spx_hip_mat_get_diag_host(A.handle, None) == sx.SPX_FAILURE
    assert untouched()
    A.get_diag(d)
    assert np.array_equal(bits(d.download()), bits(wanted(csr, A)))
    d.init(SENTINEL)
    A.diag_plan_drop()
    with pytest.raises(SpxError):
        A.get_diag(d)
    assert untouched()
    A.destroy()
    # a host-only matrix: the device entry points refuse, the host one works
    H = vc.tune(csr, W4, host_only=True)
    H.diag_plan()
    with pytest.raises(SpxError):
        H.get_diag(d)
    with pytest.raises(SpxError):
        H.hip_get_diag(d.data_ptr())
    assert untouched()
    assert np.array_equal(bits(H.get_diag_host(np.full(n, SENTINEL))), bits(wanted(csr, H)))
    capfd.readouterr()
    H.destroy()
    sx.options_reset()
