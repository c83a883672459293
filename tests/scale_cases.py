"""What the tests of the norms and the diagonal scaling of a tuned matrix (spx_hip_mat_norms / spx_hip_mat_scale)
share: scale vectors from a hash of the index, the expected scaled matrix -- (dr[r] * a) * dc[c], formed by numpy
in exactly that order -- and the expected norms from the untuned CSR arrays with their bounds.  Vectors are in the
numbering of the products' vectors (the tuned one of a reordered matrix), matrices in the caller's.  No pytest code
in here."""
import numpy as np

import sparsex_amd as sx

import dist_cases as dc
import values_cases as vc
from diag_cases import NCOLS, matrix, bits

SENTINEL = -7.5
KINDS = (sx.NORM_SUM_ABS, sx.NORM_SUM_SQ, sx.NORM_MAX_ABS)


def _hash(n, seed):
    with np.errstate(over="ignore"):
        x = np.arange(n, dtype=np.uint64) + np.uint64(seed) * np.uint64(0x9E3779B97F4A7C15)
        for mul in (0xBF58476D1CE4E5B9, 0x94D049BB133111EB):
            x = (x ^ (x >> np.uint64(30))) * np.uint64(mul)
        return x ^ (x >> np.uint64(31))


def vector(n, seed, period=None):
    """n doubles with magnitudes in (0.5, 2) and mixed signs (`period`: of a long vector, which repeats)"""
    if period is not None and n > period:
        return np.tile(vector(period, seed), n // period + 1)[:n].copy()
    x = _hash(n, seed)
    mag = 0.5 * 4.0 ** ((x >> np.uint64(12)).astype(np.float64) / float(1 << 52))
    mag = np.clip(mag, np.nextafter(0.5, 1.0), np.nextafter(2.0, 1.0))
    return np.where((x & np.uint64(1)) == 1, -mag, mag)


def pow2_vector(n, seed):
    """n powers of two 2^k, k in -3 .. 3: scaling by them and then by their reciprocals is exact"""
    k = (_hash(n, seed) % np.uint64(7)).astype(np.int64) - 3
    return 2.0 ** k.astype(np.float64)


def tuned_coords(csr, perm=None, row0=0):
    """(row, column) of every CSR entry in the numbering of the products' vectors"""
    r, c = vc.coords(csr)
    r = r + row0
    if perm is not None:
        r, c = perm[r], perm[c]
    return r, c


def scaled_values(csr, dr=None, dc=None, perm=None, row0=0):
    """the CSR value array after A.scale(dr, dc): (dr[r] * a) * dc[c], a missing vector's product not formed"""
    r, c = tuned_coords(csr, perm, row0)
    v = csr[2].copy()
    if dr is not None:
        v = dr[r] * v
    if dc is not None:
        v = v * dc[c]
    return v


def expected_norms(csr, kind, nrows, ncols, lo, hi, perm=None, row0=0):
    """(rows, cols, entries per row, entries per column) of the entries whose tuned row lies in [lo, hi): rows is
    SENTINEL outside [lo, hi), +0.0 where nothing is stored"""
    r, c = tuned_coords(csr, perm, row0)
    own = (r >= lo) & (r < hi)
    r, c, v = r[own], c[own], np.abs(csr[2][own])
    t = v * v if kind == sx.NORM_SUM_SQ else v
    rows, cols = np.zeros(nrows), np.zeros(ncols)
    if kind == sx.NORM_MAX_ABS:
        np.maximum.at(rows, r, t)
        np.maximum.at(cols, c, t)
    else:
        np.add.at(rows, r, t)
        np.add.at(cols, c, t)
    rows[:lo] = SENTINEL
    rows[hi:] = SENTINEL
    return rows, cols, np.bincount(r, minlength=nrows), np.bincount(c, minlength=ncols)


def check_norms(kind, got, want, count, what):
    """The max kind bit for bit; a sum within n * 2^-52 * want, n the entries of that row or column: the worst case
    of two sums of n non-negative terms in any order (n * 2^-53 relative each)."""
    assert got.shape == want.shape, what
    if kind == sx.NORM_MAX_ABS:
        bad = np.flatnonzero(bits(got) != bits(want))
        assert bad.size == 0, "%s: element %d is %r, not %r (%d differ)" % (what, bad[0], got[bad[0]], want[bad[0]], bad.size)
        return
    fixed = (count == 0) | (want == SENTINEL)               # nothing stored, or not this process' row: exact
    assert np.array_equal(bits(got[fixed]), bits(want[fixed])), "%s: an empty or foreign element was touched" % what
    err = np.abs(got - want)
    bound = count * 2.0 ** -52 * np.abs(want)
    bad = np.flatnonzero(~fixed & ~(err <= bound))
    assert bad.size == 0, "%s: element %d is %r, not %r: off by %.3g bounds" % (
        what, bad[0], got[bad[0]], want[bad[0]], err[bad[0]] / bound[bad[0]])


def check_all_norms(norms_of, csr, nrows, ncols, lo, hi, perm=None, row0=0):
    """`norms_of(kind)` -> (rows, cols) as numpy arrays (rows started as SENTINELs), for the three kinds"""
    for kind in KINDS:
        want_r, want_c, nr, nc = expected_norms(csr, kind, nrows, ncols, lo, hi, perm, row0)
        rows, cols = norms_of(kind)
        if rows is not None:
            check_norms(kind, rows, want_r, nr, "kind %d rows" % kind)
        if cols is not None:
            check_norms(kind, cols, want_c, nc, "kind %d cols" % kind)


def tuned_matrix(t, values):
    """what the handle of the Tuned `t` multiplies by when its CSR arrays hold `values`: the entries of its own rows
    as a scipy matrix in the numbering of the products' vectors, and its transpose, each with its CSR tuple"""
    import scipy.sparse as sp
    r, c = tuned_coords(t.csr, t.perm, t.row0)
    own = (r >= t.lo) & (r < t.hi)
    m = sp.csr_matrix((values[own], (r[own], c[own])), shape=(t.nrows, t.ncols))
    mt = sp.csr_matrix(m.T)
    out = []
    for a in (m, mt):
        a.sort_indices()
        out += [a, (a.indptr.astype(np.int32), a.indices.astype(np.int32), a.data, a.shape[0])]
    return out


def untouched_positions(before, after, src_values):
    """the positions of the decoded value array without a source in the values plan hold the bits they held"""
    none = src_values == vc.NONE
    assert before.values.size == after.values.size == src_values.size
    assert np.array_equal(bits(before.values[none]), bits(after.values[none])), "padding was written"
    return int(none.sum())


class Tuned:
    """A tune with what the checks need: the handle `A`, the CSR arrays of the rows this process was handed (`csr`,
    the first of them `row0`), the column count, the permutation of a reordered matrix, the own rows [lo, hi)."""

    def __init__(self, A, csr, ncols=None, perm=None, row0=0):
        self.A, self.csr, self.row0, self.perm = A, csr, row0, perm
        self.ncols = csr[3] if ncols is None else ncols
        self.nrows = A.nrows
        inf = A.info()
        self.lo, self.hi = inf.row_lo, inf.row_hi
        assert A.ncols == self.ncols

    def scipy(self, values):
        """the matrix with these CSR values, caller's numbering, global rows"""
        return vc.to_scipy(vc.with_values(self.csr, values), ncols=self.ncols, row0=self.row0, nrows=self.nrows)

    def scaled(self, values, dr=None, dc=None):
        return scaled_values(vc.with_values(self.csr, values), dr, dc, self.perm, self.row0)

    def check_norms(self, norms_of, values):
        check_all_norms(norms_of, vc.with_values(self.csr, values), self.nrows, self.ncols, self.lo, self.hi, self.perm,
                        self.row0)


def tune_matrix(name, opts=None, reorder=False, host_only=False):
    """one of the matrices of diag_cases, whole"""
    csr = matrix(name)
    A = vc.tune(csr, opts, host_only=host_only, reorder=reorder, ncols=NCOLS.get(name))
    return Tuned(A, csr, NCOLS.get(name), A.get_perm().astype(np.int64) if reorder else None)


def tune_slice(how, opts=None, host_only=False):
    """slice 1 of 3 of nlpkkt: "rank" (the whole matrix handed over, spx.rt.gpu_rank/world) or "row-offset" (its
    rows only, spx.rt.row_offset)"""
    whole = matrix("nlpkkt")
    rp, ci, va, n = whole
    opts = dict(dc.NOSAMPLE, **(opts or {}))
    if how == "rank":
        t = Tuned(dc.tune_rank(whole, 1, 3, opts, host_only=host_only), whole)
    else:
        lo, hi = dc.cut(whole, 3, "balanced")[1:3]
        part = ((rp[lo:hi + 1] - rp[lo]).astype(np.int32), ci[rp[lo]:rp[hi]].copy(), va[rp[lo]:rp[hi]].copy(), n)
        t = Tuned(dc.tune_rows(whole, lo, hi, opts, host_only=host_only), part, row0=lo)
    assert 0 < t.lo < t.hi < t.nrows
    return t
