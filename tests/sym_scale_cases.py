"""What the tests of the norms and the scaling D * A * D of a matrix tuned as a symmetric one (spx_hip_mat_sym_norms /
spx_hip_mat_sym_scale) share: the expected scaled values from the full symmetric CSR arrays -- (d[max(r,c)] * a) *
d[min(r,c)], formed by numpy in exactly that order -- and the expected norms with the entry counts that
scale_cases.check_norms takes its bounds from.  Vectors are in the numbering of the products' vectors (the tuned one
of a reordered matrix), matrices in the caller's; they come from scale_cases.vector (mixed signs) and pow2_vector.
No pytest code in here."""
import numpy as np
import scipy.sparse as sp

import sparsex_amd as sx

import scale_cases as sc
import values_cases as vc
from diag_cases import bits

SENTINEL = sc.SENTINEL
KINDS = sc.KINDS
vector, pow2_vector = sc.vector, sc.pow2_vector


def scaled_values(csr, d, perm=None):
    """the value array of the full symmetric CSR after A.sym_scale(d): the factor of the larger tuned index first"""
    r, c = sc.tuned_coords(csr, perm)
    return (d[np.maximum(r, c)] * csr[2]) * d[np.minimum(r, c)]


def scaled_matrix(csr, d, perm=None):
    """... as (value array, scipy matrix in the caller's numbering)"""
    v = scaled_values(csr, d, perm)
    return v, vc.to_scipy(vc.with_values(csr, v))


def expected_norms(csr, kind, lo=0, hi=None, perm=None):
    """(norms, entries per element) of a whole matrix from its full CSR arrays (lo = 0, hi = n), or the partial
    result of the slice that owns the tuned rows [lo, hi): the entries {r own, c <= r}, counted for r and, off the
    diagonal, for c.  +0.0 where the process holds nothing."""
    n = csr[3]
    hi = n if hi is None else hi
    r, c = sc.tuned_coords(csr, perm)
    t = np.abs(csr[2])
    t = t * t if kind == sx.NORM_SUM_SQ else t
    if lo == 0 and hi == n:
        idx, val = r, t
    else:
        low = (r >= lo) & (r < hi) & (c <= r)
        off = low & (c < r)
        idx, val = np.concatenate([r[low], c[off]]), np.concatenate([t[low], t[off]])
    out = np.zeros(n)
    if kind == sx.NORM_MAX_ABS:
        np.maximum.at(out, idx, val)
    else:
        np.add.at(out, idx, val)
    return out, np.bincount(idx, minlength=n)


def check_all_norms(norms_of, csr, lo=0, hi=None, perm=None):
    """`norms_of(kind)` -> numpy array of n doubles (which started as SENTINELs), for the three kinds: the max kind
    bit for bit, the sums within count * 2^-52 relative (scale_cases.check_norms)"""
    for kind in KINDS:
        want, count = expected_norms(csr, kind, lo, hi, perm)
        got = norms_of(kind)
        sc.check_norms(kind, got, want, count, "kind %d" % kind)


def join_partials(kind, parts):
    """what the caller's all-reduce makes of the slices' partial results"""
    parts = np.array(parts)
    return parts.max(axis=0) if kind == sx.NORM_MAX_ABS else parts.sum(axis=0)


def check_joined(kind, parts, counts, csr, perm=None):
    """the joined partial results of all the slices against the whole matrix' norms.  Bound of a sum: every slice's
    partial is within its count * 2^-52, their sum adds one rounding per slice."""
    want, count = expected_norms(csr, kind, perm=perm)
    got = join_partials(kind, parts)
    assert np.array_equal(np.sum(counts, axis=0), count), "the slices' entries are not the matrix'"
    sc.check_norms(kind, got, want, count + len(parts), "kind %d joined" % kind)


def rounded_csr(csr, values):
    """the CSR arrays with `values` rounded to float, as the float copy holds them"""
    return vc.with_values(csr, values.astype(np.float32).astype(np.float64))


def lds_doubles(stream):
    """the most transposed-sum slots + rows of a row-block of a decoded stream: the dynamic LDS of a norms launch"""
    rbs = stream.rbs
    return int((rbs["n_slots"].astype(np.int64) + rbs["n_rows"].astype(np.int64)).max()) if rbs.size else 0
