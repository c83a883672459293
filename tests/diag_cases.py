"""What the tests of the diagonal of a tuned matrix (spx_hip_mat_diag_plan / spx_hip_mat_get_diag*) share: the small
matrices, and the expected diagonal from the untuned CSR arrays -- tuned numbering, +0.0 where nothing is stored, a
sentinel outside the own rows."""
import numpy as np
import scipy.sparse as sp

from sparsex_amd import synth

import values_cases as vc

NONE = 0xFFFFFFFF
SENTINEL = -7.5
_cache = {}


def _csr_of(m):
    m = sp.csr_matrix(m)
    m.sort_indices()
    return (m.indptr.astype(np.int32), m.indices.astype(np.int32), m.data.copy(), m.shape[0])


def _rect():
    m = sp.random(300, 200, density=0.03, random_state=np.random.RandomState(7), format="lil")
    for i in range(0, 200, 3):          # some diagonal entries, some rows without, rows >= ncols without any
        m[i, i] = 1.0 + i
    return sp.csr_matrix(m)


GENERATORS = {
    "cant": lambda: synth.syn_cant(0.05),
    "nlpkkt": lambda: synth.syn_nlpkkt(6),
    "webbase": lambda: synth.syn_webbase(0.02),
    "rect": lambda: _csr_of(_rect()),
    "rect-t": lambda: _csr_of(_rect().T),
}
NCOLS = {"rect": 200, "rect-t": 300}


def matrix(name):
    if name not in _cache:
        _cache[name] = GENERATORS[name]()
    return _cache[name]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def stored_diag(csr, ncols=None, row0=0):
    """(has, value) per global row of the rows the CSR arrays hold: whether a(i, i) is stored, and its value"""
    r, c = vc.coords(csr)
    r = r + row0
    n = csr[3] if row0 == 0 else None
    nrows = (csr[0].size - 1 + row0) if n is None else n
    has = np.zeros(nrows, dtype=bool)
    val = np.zeros(nrows)
    on = r == c
    has[r[on]] = True
    val[r[on]] = csr[2][on]
    return has, val


def expect(has, val, lo, hi, perm=None):
    """what get_diag_host leaves in an array of SENTINELs: tuned numbering, +0.0 where nothing is stored"""
    n = has.size
    d = np.where(has, val, 0.0)
    h = has
    if perm is not None:
        t = np.empty(n)
        t[perm] = d
        th = np.empty(n, dtype=bool)
        th[perm] = h
        d, h = t, th
    out = np.full(n, SENTINEL)
    out[lo:hi] = d[lo:hi]
    return out, int(h[lo:hi].sum())


def padded(has, val, nrows):
    """(a slice's arrays end with its last row)"""
    if has.size < nrows:
        return np.pad(has, (0, nrows - has.size)), np.pad(val, (0, nrows - val.size))
    return has, val
