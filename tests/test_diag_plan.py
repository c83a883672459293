"""The diagonal of a tuned matrix on host-only tunes: spx_hip_mat_diag_plan, spx_hip_mat_get_diag_host and
spx_hip_mat_diag_plan_get against scipy's diagonal of the untuned CSR, against the numpy decoder of a saved stream
and against spx_mat_get_entry (stream_locate) -- neither shares code with the plan's walk."""
import numpy as np
import pytest

import sparsex_amd as sx
from sparsex_amd.api import SpxError

import dist_cases as dc
import values_cases as vc

from diag_cases import NONE, SENTINEL, NCOLS, matrix, bits, stored_diag, expect, padded


def check(A, csr, sym, tmp_path, perm=None, row0=0, sample=40, update=True):
    """plan, diagonal, counters, positions; then new values (one diagonal entry -0.0) and one set_entry"""
    inf = A.info()
    lo, hi = inf.row_lo, inf.row_hi
    nrows = A.nrows
    has, val = stored_diag(csr, row0=row0)
    has, val = padded(has, val, nrows)
    A.diag_plan()
    info = A.diag_plan_info()
    want, present = expect(has, val, lo, hi, perm)
    got = A.get_diag_host(np.full(nrows, SENTINEL))
    assert np.array_equal(bits(got), bits(want))
    assert info["n_rows"] == hi - lo and info["row_lo"] == lo and info["plan_bytes"] == 0
    if sym:
        assert info["pos"] is None and info["n_present"] == 0
    else:
        pos = info["pos"]
        assert info["n_present"] == present == int((pos != NONE).sum())
        s = vc.decoded(A, tmp_path, "diag.spx")
        inv = np.argsort(perm) if perm is not None else np.arange(nrows)
        rows = np.flatnonzero(pos != NONE)
        if rows.size > sample:
            rows = np.unique(np.concatenate([rows[[0, -1]], np.random.RandomState(1).choice(rows, sample, replace=False)]))
        for i in rows:
            cr = int(inv[lo + i])
            assert s.values[pos[i]] == A.get_entry(cr, cr) == got[lo + i]
    if not update:
        return
    # new values for the same pattern, one diagonal entry of the own rows -0.0
    A.values_plan(csr[0], csr[1])
    v1 = vc.new_values(csr, sym, 13, row0=row0)
    r, c = vc.coords(csr)
    tr = (r + row0) if perm is None else perm[r + row0]
    on = np.flatnonzero((r + row0 == c) & (tr >= lo) & (tr < hi))
    assert on.size
    v1[on[on.size // 2]] = -0.0
    A.set_values(v1)
    has1, val1 = stored_diag(vc.with_values(csr, v1), row0=row0)
    has1, val1 = padded(has1, val1, nrows)
    want1, _ = expect(has1, val1, lo, hi, perm)
    got1 = A.get_diag_host(np.full(nrows, SENTINEL))
    assert np.array_equal(bits(got1), bits(want1))
    assert (bits(got1[lo:hi]) == bits(np.array([-0.0]))[0]).sum() == 1
    # one entry through spx_mat_set_entry (caller's numbering)
    k = on[0]
    cr = int(r[k] + row0)
    A.set_entry(cr, cr, 3.25)
    got2 = A.get_diag_host(np.full(nrows, SENTINEL))
    want1[int(tr[k])] = 3.25
    assert np.array_equal(bits(got2), bits(want1))


@pytest.mark.parametrize("name", ["cant", "nlpkkt", "webbase", "rect", "rect-t"])
def test_general_matrices(tmp_path, name):
    csr = matrix(name)
    ncols = NCOLS.get(name)
    if name == "webbase":
        has, _ = stored_diag(csr)
        assert csr[3] == 20000 and int((~has).sum()) == 19984      # rows without a stored diagonal entry
    if name == "rect":
        has, _ = stored_diag(csr)
        assert not has[200:].any() and not has[:200].all() and has.any()
    A = vc.tune(csr, {}, host_only=True, ncols=ncols)
    check(A, csr, False, tmp_path)
    A.destroy()


@pytest.mark.parametrize("mode", ["defaults", "mirrored"])
@pytest.mark.parametrize("name", ["cant", "nlpkkt"])
def test_symmetric_matrices(tmp_path, name, mode):
    csr = matrix(name)
    A = vc.tune(csr, {"spx.gpu.sym_once": "false"} if mode == "mirrored" else {}, sym=True, host_only=True)
    # (no plan call needed: the diagonal has an array of its own)
    has, val = stored_diag(csr)
    assert np.array_equal(bits(A.get_diag_host()), bits(np.where(has, val, 0.0)))
    check(A, csr, True, tmp_path)
    A.diag_plan_drop()
    assert np.array_equal(bits(A.get_diag_host()), bits(A.get_diag_host(np.full(A.nrows, SENTINEL))))
    A.destroy()


@pytest.mark.parametrize("phases", ["c2", "2"])
@pytest.mark.parametrize("name", ["cant", "nlpkkt"])
def test_column_slices(tmp_path, name, phases):
    csr = matrix(name)
    A = vc.tune(csr, {"spx.gpu.col_phases": phases}, host_only=True)
    assert abs(A.info().col_slices) == 2
    check(A, csr, False, tmp_path)
    A.destroy()


@pytest.mark.parametrize("sym", [False, True])
def test_reordered_matrix(tmp_path, sym):
    csr = matrix("cant")
    A = vc.tune(csr, {}, sym=sym, host_only=True, reorder=True)
    perm = A.get_perm()
    assert perm is not None and not np.array_equal(perm, np.arange(csr[3]))
    check(A, csr, sym, tmp_path, perm=perm.astype(np.int64))
    A.destroy()


@pytest.mark.parametrize("sym", [False, True])
def test_rank_one_of_three(tmp_path, sym):
    csr = matrix("nlpkkt")
    A = dc.tune_rank(csr, 1, 3, dc.NOSAMPLE, sym, host_only=True)
    inf = A.info()
    assert 0 < inf.row_lo < inf.row_hi < csr[3]
    check(A, csr, sym, tmp_path)
    A.destroy()


@pytest.mark.parametrize("sym", [False, True])
def test_row_offset_slice_one_of_three(tmp_path, sym):
    csr = matrix("nlpkkt")
    rp, ci, va, n = csr
    cuts = dc.cut(csr, 3, "balanced")
    lo, hi = cuts[1], cuts[2]
    A = dc.tune_rows(csr, lo, hi, dc.NOSAMPLE, sym, host_only=True)
    part = ((rp[lo:hi + 1] - rp[lo]).astype(np.int32), ci[rp[lo]:rp[hi]].copy(), va[rp[lo]:rp[hi]].copy(), n)
    inf = A.info()
    assert (inf.row_lo, inf.row_hi) == (lo, hi)
    check(A, part, sym, tmp_path, row0=lo)
    A.destroy()


def test_without_a_plan_and_after_restore(tmp_path):
    csr = matrix("nlpkkt")
    A = vc.tune(csr, {}, host_only=True)
    with pytest.raises(SpxError):
        A.get_diag_host()
    with pytest.raises(SpxError):
        A.diag_plan_info()
    A.diag_plan()
    d = A.get_diag_host()
    A.diag_plan()                                     # a second plan replaces the first
    assert np.array_equal(bits(A.get_diag_host()), bits(d))
    A.diag_plan_drop()
    sent = np.full(A.nrows, SENTINEL)
    with pytest.raises(SpxError):
        A.get_diag_host(sent)
    assert (sent == SENTINEL).all()
    A.diag_plan()
    f = str(tmp_path / "m.spx")
    A.save(f)
    B = sx.mat_restore(f)                             # (spx.rt.host_only is still set)
    with pytest.raises(SpxError):
        B.get_diag_host()
    B.diag_plan()
    assert np.array_equal(bits(B.get_diag_host()), bits(d))
    # a host-only matrix has no HIP executor: the device entry points say so, whatever the pointer
    with pytest.raises(SpxError):
        B.hip_get_diag(8)
    A.destroy()
    B.destroy()


def test_null_arguments():
    L = sx.lib()
    csr = matrix("nlpkkt")
    A = vc.tune(csr, {}, host_only=True)
    A.diag_plan()
    buf = np.zeros(A.nrows)
    assert L.spx_hip_mat_diag_plan(None) == sx.SPX_FAILURE
    assert L.spx_hip_mat_diag_plan_drop(None) == sx.SPX_FAILURE
    assert L.spx_hip_mat_get_diag_host(None, buf.ctypes.data) == sx.SPX_FAILURE
    assert L.spx_hip_mat_get_diag_host(A.handle, None) == sx.SPX_FAILURE
    assert L.spx_hip_mat_get_diag(None, 8, None) == sx.SPX_FAILURE
    assert L.spx_hip_mat_get_diag(A.handle, None, None) == sx.SPX_FAILURE
    assert L.spx_hip_mat_get_diag_vec(A.handle, None, None) == sx.SPX_FAILURE
    assert L.spx_hip_mat_get_diag_vec(None, None, None) == sx.SPX_FAILURE
    assert L.spx_hip_mat_diag_plan_get(A.handle, None) == sx.SPX_FAILURE
    assert L.spx_hip_mat_diag_plan_get(None, None) == sx.SPX_FAILURE
    assert (buf == 0.0).all()
    A.destroy()


@pytest.mark.parametrize("sym,name", [(False, "nlpkkt"), (True, "cant")])
def test_values_plan_walk_names_every_position(tmp_path, sym, name):
    """The walk the two plans share, through the values plan: every position it gives a source holds, in the saved
    stream, the value of exactly that CSR entry (the values are distinct hashes of (row, column))."""
    csr = matrix(name)
    v0 = vc.new_values(csr, sym, 21)
    csr = vc.with_values(csr, v0)
    A = vc.tune(csr, {}, sym=sym, host_only=True)
    A.values_plan(csr[0], csr[1])
    info = A.values_plan_info()
    s = vc.decoded(A, tmp_path, "walk.spx")
    src = info["src_values"]
    assert src.size == s.values.size
    at = np.flatnonzero(src != NONE)
    assert at.size and np.array_equal(bits(s.values[at]), bits(v0[src[at].astype(np.int64)]))
    # (positions without a source hold what the tune put there: zeros)
    assert not s.values[src == NONE].any()
    A.destroy()
