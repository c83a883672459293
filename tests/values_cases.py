"""What the tests of the bulk value update (spx_hip_mat_values_plan / spx_hip_mat_set_values) share: new value
arrays for a pattern, and the two independent checks of a matrix after an update -- the numpy decoder of a saved
stream (stream_decode.py: every stored copy, whatever found it) and spx_mat_get_entry (stream_locate)."""
import numpy as np
import scipy.sparse as sp

import sparsex_amd as sx
from stream_decode import Stream

NOSAMPLE = {"spx.preproc.sampling": "none"}
NONE = 0xFFFFFFFF


def tune(csr, opts=None, sym=False, host_only=False, reorder=False, ncols=None, indexing=None):
    """helpers.tune with a reordering, a column count and an indexing of its own"""
    rp, ci, va, n = csr
    sx.options_reset()
    if host_only:
        sx.option_set("spx.rt.host_only", "true")
    for k, v in dict(NOSAMPLE, **(opts or {})).items():
        sx.option_set(k, str(v))
    if sym:
        sx.option_set("spx.matrix.symmetric", "true")
    args = () if indexing is None else (indexing,)
    inp = sx.input_load_csr(rp, ci, va, n, n if ncols is None else ncols, *args)
    A = sx.mat_tune(inp, reorder=reorder)
    A._input = inp
    return A


def coords(csr, base=0):
    """(row, column) of every CSR entry, 0-based"""
    rp, ci = csr[0], csr[1]
    return np.repeat(np.arange(rp.size - 1), np.diff(rp)), ci.astype(np.int64) - base


def new_values(csr, sym, seed, row0=0, base=0):
    """A value array for the pattern of `csr`, uniform in (-2, -1) u (1, 2) (no zero, nothing near one); `sym`: the
    same value at (r, c) and (c, r), whatever the order of the entries (`row0`: the first row of a slice)."""
    # a hash of (row, column, seed): the slices of one matrix give the same entry the same value
    r, c = coords(csr, base)
    r = r + row0
    if sym:
        r, c = np.minimum(r, c), np.maximum(r, c)
    with np.errstate(over="ignore"):
        x = (r.astype(np.uint64) << np.uint64(32)) + c.astype(np.uint64) + np.uint64(seed) * np.uint64(0x9E3779B97F4A7C15)
        for mul in (0xBF58476D1CE4E5B9, 0x94D049BB133111EB):
            x = (x ^ (x >> np.uint64(30))) * np.uint64(mul)
        x = x ^ (x >> np.uint64(31))
    mag = 1.0 + (x >> np.uint64(12)).astype(np.float64) / float(1 << 52)
    return np.where((x & np.uint64(1)) == 1, -mag, mag)


def with_values(csr, v):
    return (csr[0], csr[1], v, csr[3])


def to_scipy(csr, ncols=None, base=0, row0=0, nrows=None):
    """the CSR arrays as a scipy matrix in global rows (a slice: its rows at row0)"""
    rp, ci, va, n = csr
    r, c = coords(csr, base)
    nr = rp.size - 1 + row0 if nrows is None else nrows
    return sp.csr_matrix((va, (r + row0, c)), shape=(nr, n if ncols is None else ncols))


def decoded(A, tmp_path, name="m.spx"):
    f = str(tmp_path / name)
    A.save(f)
    return Stream(f)


def check_stream(A, m, tmp_path, sym=False, perm=None):
    """Every stored copy of every nonzero of the saved stream -- lower triangle, mirror image, tiles, read-once
    segments, thin mirror list, diagonal -- holds the value of the scipy matrix `m` (caller's numbering) there,
    bit for bit.  Returns the decoded stream."""
    s = decoded(A, tmp_path, "check.spx")
    r, c, v, _ = s.triplets()
    if perm is not None:
        inv = np.argsort(perm)
        r, c = inv[r], inv[c]
    want = np.asarray(m[r, c]).ravel() if r.size else np.zeros(0)
    if sym:
        # (the diagonal lives in dvalues; a cell on it inside a dense block is a zero that must stay one)
        want = np.where(r == c, 0.0, want)
    bad = np.flatnonzero(want != v)
    assert bad.size == 0, "stored copy of (%d, %d) holds %r, not %r (%d differ)" % (
        r[bad[0]], c[bad[0]], v[bad[0]], want[bad[0]], bad.size)
    if sym:
        d = np.asarray(m.diagonal())
        rows = np.arange(s.own_lo, s.own_hi)
        got = s.dvalues[rows]
        want = d[np.argsort(perm)[rows]] if perm is not None else d[rows]
        assert np.array_equal(got, want), "diagonal"
    return s


def check_entries(A, m, rows=None, limit=1500, seed=3, sym=False):
    """spx_mat_get_entry returns the value of `m` for its entries (all of them up to `limit`, else a random sample
    that always holds the first and the last); `rows`: (lo, hi) of a general slice."""
    coo = m.tocoo()
    r, c, v = coo.row, coo.col, coo.data
    if rows is not None:
        keep = (r >= rows[0]) & (r < rows[1])
        if sym:
            keep = (np.maximum(r, c) >= rows[0]) & (np.maximum(r, c) < rows[1])
        r, c, v = r[keep], c[keep], v[keep]
    idx = np.arange(r.size)
    if r.size > limit:
        idx = np.unique(np.concatenate([[0, r.size - 1], np.random.RandomState(seed).choice(r.size, limit, replace=False)]))
    for k in idx:
        got = A.get_entry(int(r[k]), int(c[k]))
        assert got == v[k], "get_entry(%d, %d) = %r, not %r" % (r[k], c[k], got, v[k])
    return idx.size


def destinations(info, nnz):
    """destinations per CSR index over the three arrays of a plan"""
    cnt = np.zeros(nnz, dtype=np.int64)
    for name in ("src_values", "src_mirror", "src_diag"):
        a = info[name]
        a = a[a != NONE].astype(np.int64)
        assert a.size == 0 or a.max() < nnz
        cnt += np.bincount(a, minlength=nnz)
    return cnt
