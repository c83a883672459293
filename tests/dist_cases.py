"""Cases for the row-partitioned path: matrices, cuts into the row ranges of 2 and 3 processes, the two ways of
making a process' slice (its rows only: spx.rt.row_offset / global_rows; the whole matrix: spx.rt.gpu_rank /
gpu_world), the kernel families, and float64 references of what a slice computes -- rows [lo, hi) of the product
on the general path, the partial vector of an unattached slice on the symmetric one.  test_dist_cases.py tunes
every case host-only and asserts, on the decoded stream, that it reaches what it is named for;
test_gpu_slices.py runs the slices in one process, dist_worker.py (started by test_gpu_dist_step.py) runs the
attached step on several ranks.  No pytest code in here.

Every matrix is seeded (sparsex_amd.synth) and the smallest of its generator that still reaches what the case
is for."""
import numpy as np
import scipy.sparse as sp

import sparsex_amd as sx
from sparsex_amd import synth
from helpers import FP64_BOUND_FACTOR, abs_bound
import limit_cases as lc
from test_row_slices import nnz_balanced_bounds

NOSAMPLE = lc.NOSAMPLE
ALPHA_BETA = lc.ALPHA_BETA
WAVES = "4"                   # pinned, as limit_cases does: the launch tuner may emit the stream again

# name -> generator of the whole matrix as (rowptr, colind, values, n); all symmetric with a positive diagonal
MATRICES = {
    "nlpkkt": lambda: synth.syn_nlpkkt_rows(12),
    "kkt2f": lambda: synth.syn_kkt2f_rows(12),
    "nd24k": lambda: synth.syn_nd24k(0.02),                # dense 8x8 tiles
    # runs long enough for passes of their own on a slice: csx_spmv_sx_kernel (test_dist_cases.py: SX passes > 0)
    "pipeline": lambda: synth.syn_nlpkkt_rows(PIPELINE_EDGE),
    # the last of three symmetric slices couples into rows all over the grid: a thin mirror list
    "thin-mirror": lambda: synth.syn_kkt2f_rows(THIN_EDGE),
}
PIPELINE_EDGE = 42             # (41: no run of the stencil is long enough for a pass of its own)
THIN_EDGE = 24                 # (23: the last slice of three has no list yet)

CUT_KINDS = ("balanced", "shifted", "one-row")


def cut(csr, world, kind):
    """The first rows of `world` slices, and n: balanced by nonzeros; the same shifted by three rows (on nd24k a
    boundary that is no multiple of 8 runs through a block row); the last rank holds exactly one row."""
    rp, n = csr[0], csr[3]
    counts = np.diff(rp)
    if kind == "balanced":
        return nnz_balanced_bounds(counts, world)
    if kind == "shifted":
        b = nnz_balanced_bounds(counts, world)
        return [0] + [c + 3 for c in b[1:-1]] + [n]
    if kind == "one-row":
        return nnz_balanced_bounds(counts[:n - 1], world - 1)[:-1] + [n - 1, n]
    raise KeyError(kind)


# name -> (matrix, world, cut kind, options on top of the family's, general families, symmetric families)
# The three generators meet every cut and both worlds once; the last three cases are
# there for one kernel each.
GENERAL_ALL = tuple(lc.OFF_FAMILIES)
SYM_ALL = tuple(lc.SYM_FAMILIES)
# at least 64 row-blocks per rank for device_plan_chunks: smaller row-blocks, not a larger matrix
SMALL_RB = {"spx.gpu.rowblock_elems": "256", "spx.gpu.rowblock_rows": "16"}
CASES = {
    "nlpkkt-w2-balanced": ("nlpkkt", 2, "balanced", {}, GENERAL_ALL, SYM_ALL),
    "nlpkkt-w3-shifted": ("nlpkkt", 3, "shifted", {}, GENERAL_ALL, SYM_ALL),
    "nlpkkt-w2-one-row": ("nlpkkt", 2, "one-row", {}, GENERAL_ALL, SYM_ALL),
    "kkt2f-w3-balanced": ("kkt2f", 3, "balanced", {}, GENERAL_ALL, SYM_ALL),
    "kkt2f-w2-shifted": ("kkt2f", 2, "shifted", {}, GENERAL_ALL, SYM_ALL),
    "kkt2f-w3-one-row": ("kkt2f", 3, "one-row", {}, GENERAL_ALL, SYM_ALL),
    # (the balanced cut in two lies five rows behind a multiple of 8: shifted by three it is ON a block row)
    "nd24k-w2-balanced": ("nd24k", 2, "balanced", {}, GENERAL_ALL, SYM_ALL),
    "nd24k-w2-shifted": ("nd24k", 2, "shifted", {}, GENERAL_ALL, SYM_ALL),
    "nd24k-w3-shifted": ("nd24k", 3, "shifted", {}, GENERAL_ALL, SYM_ALL),
    "nd24k-w2-one-row": ("nd24k", 2, "one-row", {}, GENERAL_ALL, SYM_ALL),
    "pipeline-w2-balanced": ("pipeline", 2, "balanced", {}, (), ("segments", "pipeline")),
    "thin-mirror-w3-balanced": ("thin-mirror", 3, "balanced", {}, (), SYM_ALL),
    "overlap-w2-balanced": ("nlpkkt", 2, "balanced", SMALL_RB, ("plain", "det", "unit-windows"), ()),
    "overlap-w3-shifted": ("nlpkkt", 3, "shifted", SMALL_RB, ("plain", "det", "unit-windows"), ()),
}
MISALIGNED = ("nd24k-w2-balanced", "nd24k-w3-shifted")      # no boundary is a multiple of 8
OVERLAP = ("overlap-w2-balanced", "overlap-w3-shifted")
PIPELINED = ("pipeline-w2-balanced",)          # csx_spmv_sx_kernel takes passes of a slice (family "pipeline")
THIN_MIRROR = "thin-mirror-w3-balanced"


def thin_mirror_entry(csr, lo, mirror_rows):
    """(row, column) of a stored nonzero of the slice that starts at row lo whose mirror image lives in the thin
    mirror list: the first column of the last row that has one there (a grid row far in front of the slice)."""
    rp, ci, _, n = csr
    listed = set(int(v) for v in mirror_rows)
    r = next(q for q in range(n - 1, lo, -1) if int(ci[rp[q]]) in listed)
    return r, int(ci[rp[r]])


def pairs(symmetric):
    """(case, family) of one path, in the table's order"""
    return [(c, f) for c, v in CASES.items() for f in v[5 if symmetric else 4]]


def matrix(case):
    return MATRICES[CASES[case][0]]()


def bounds(case, csr):
    _, world, kind, _, _, _ = CASES[case]
    return cut(csr, world, kind)


def family_options(case, family, symmetric):
    """The options of a tune of `case` under `family`: no sampling, four wavefronts, the family's switches (the
    general ones without the row-block settings of the offset cases) and the case's own."""
    extra = dict(CASES[case][3], **{"spx.gpu.waves": WAVES})
    if symmetric:
        return lc.sym_options(family, extra)
    return dict(NOSAMPLE, **dict(lc.OFF_FAMILIES[family], **extra))


# ---- the two ways of making a slice --------------------------------------------------------------------------

def _set(opts, symmetric, host_only):
    sx.options_reset()
    if host_only:
        sx.option_set("spx.rt.host_only", "true")
    for k, v in opts.items():
        sx.option_set(k, str(v))
    if symmetric:
        sx.option_set("spx.matrix.symmetric", "true")


def tune_rows(csr, lo, hi, opts, symmetric=False, host_only=False, threads=2):
    """The process is handed rows [lo, hi) only (a symmetric slice: the full rows)."""
    rp, ci, va, n = csr
    rl = (rp[lo:hi + 1] - rp[lo]).astype(np.int32)
    cl, vl = ci[rp[lo]:rp[hi]].copy(), va[rp[lo]:rp[hi]].copy()
    _set(dict(opts, **{"spx.rt.row_offset": lo, "spx.rt.global_rows": n, "spx.rt.nr_threads": threads}), symmetric,
         host_only)
    inp = sx.input_load_csr(rl, cl, vl, hi - lo, n)
    A = sx.mat_tune(inp)
    A._input = inp
    return A


def tune_rank(csr, rank, world, opts, symmetric=False, host_only=False):
    """The process is handed the whole matrix and owns the partition of `rank`: the library cuts (by nonzeros,
    one partition per rank); info().row_lo / row_hi say where."""
    rp, ci, va, n = csr
    _set(dict(opts, **{"spx.rt.gpu_rank": rank, "spx.rt.gpu_world": world, "spx.rt.nr_threads": world}),
         symmetric, host_only)
    inp = sx.input_load_csr(rp, ci, va, n, n)
    A = sx.mat_tune(inp)
    A._input = inp
    return A


# ---- references: float64 scipy on the untuned CSR --------------------------------------------------------------

def to_scipy(csr):
    rp, ci, va, n = csr
    return sp.csr_matrix((va, ci, rp), shape=(n, n))


def _rows_only(m, lo, hi):
    """m with every row outside [lo, hi) emptied (n x n)"""
    n = m.shape[0]
    keep = sp.diags(((np.arange(n) >= lo) & (np.arange(n) < hi)).astype(np.float64))
    out = sp.csr_matrix(keep @ m)
    out.eliminate_zeros()
    return out


def general_part(m, lo, hi):
    """The matrix a general slice multiplies by: rows [lo, hi) of m"""
    return _rows_only(m, lo, hi)


def symmetric_part(m, lo, hi):
    """The matrix an unattached symmetric slice multiplies by: the strictly lower part L of its rows and their
    diagonal, and L's mirror image (which lands on rows in front of hi).  Over all ranks these sum to m."""
    low = _rows_only(sp.tril(m, k=-1).tocsr(), lo, hi)
    d = np.zeros(m.shape[0])
    d[lo:hi] = m.diagonal()[lo:hi]
    return sp.csr_matrix(low + low.T + sp.diags(d))


def reference(part, lo, hi, x, alpha, beta=0.0, y0=None):
    """(value, bound) of alpha * part * x + beta * y0 with the beta term on the rows [lo, hi) only: every other
    row of `part` gets its sum alone, every row `part` does not reach is 0.  The bound is helpers.abs_bound of
    |part| (the fp64 tolerance of this build) plus, as in helpers.check_y, 4 * 2^-53 * |beta * y0|.  y0 may hold
    NaN outside [lo, hi): it is not read there."""
    n = part.shape[0]
    ref = alpha * (part @ x)
    bound = abs_bound((part.indptr, part.indices, part.data, n), x, alpha)
    if beta != 0.0:
        ref[lo:hi] += beta * y0[lo:hi]
        bound[lo:hi] += 4 * 2.0 ** -53 * np.abs(beta * y0[lo:hi])
    return ref, bound


def max_ratio(y, ref, bound, rows=slice(None)):
    """max |y - ref| / bound over `rows` (inf where y is not finite; 0 over no rows)"""
    err = np.abs(y[rows] - ref[rows])
    if err.size == 0:
        return 0.0
    r = err / bound[rows]
    return float(np.where(np.isfinite(r), r, np.inf).max())


def bits(a):
    """the bit patterns of a float64 array (NaN sentinels compare equal to themselves)"""
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def nan_outside(n, lo, hi, seed):
    """y0 of a rank: random values on its own rows, NaN everywhere else"""
    y0 = np.full(n, np.nan)
    y0[lo:hi] = synth.random_x(n, seed=seed)[lo:hi]
    return y0
