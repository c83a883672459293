"""Cases and helpers shared by the tests of the multi-vector product (test_matmat_cases.py on the CPU,
test_gpu_matmat_streams.py on the GPU): band matrices whose leftovers land in dense x windows, the census of
a saved stream, padded blocks of vectors and a run that checks every column against the CSR product."""
import numpy as np
import scipy.sparse as sp

from sparsex_amd import synth
from helpers import check_y
from stream_decode import Stream

NOSAMPLE = {"spx.preproc.sampling": "none"}

# MV_LDS_BUDGET of sparsex_amd/csrc/device_runtime.cpp (80 KB), in doubles: launch_rowblocks_mv stages the K x
# windows of a call in LDS where K * (copies * rows + window) doubles fit it, and gathers through L2 otherwise.
# Whoever moves that budget moves this constant, and with it the preconditions of BANDS below.
MV_LDS_BUDGET_DOUBLES = 10240
# ... so that K = 8 windows of more than this many doubles are never staged, whatever the rows
NEVER_STAGED_AT_8 = MV_LDS_BUDGET_DOUBLES // 8
PASS_GATHER_LDS = 4
ALPHA_BETA = ((0.5, 0.0), (2.0, -0.5), (0.0, 0.75))


def band(n, hw, dens, ncols=None, seed=1):
    """n x ncols CSR with int(n * (2 hw + 1) * dens) draws around the (scaled) diagonal: row uniform, column
    row * ncols // n + U[-hw, hw]; out-of-range draws dropped, duplicates summed, values uniform in (-1, 1).
    Returns ((rowptr, colind, values, n), scipy matrix); the tuple is helpers.tune's where ncols == n."""
    ncols = n if ncols is None else ncols
    rng = np.random.RandomState(seed)
    k = int(n * (2 * hw + 1) * dens)
    r = rng.randint(0, n, k)
    c = r * ncols // n + rng.randint(-hw, hw + 1, k)
    keep = (c >= 0) & (c < ncols)
    m = sp.coo_matrix((np.ones(int(keep.sum())), (r[keep], c[keep])), shape=(n, ncols)).tocsr()
    m.sum_duplicates()
    m.sort_indices()
    m.data = rng.uniform(-1, 1, m.nnz)
    return (m.indptr.astype(np.int32), m.indices.astype(np.int32), m.data.copy(), n), m


def long_rows():
    """40000 x 40000 with two rows of 30000 and 9000 nonzeros: rows split over several row-blocks, which go
    through the carry slots and the fix-up kernel."""
    rng = np.random.RandomState(3)
    n = 40000
    rows = np.concatenate([np.full(30000, 5), np.full(9000, 17), rng.randint(0, n, 50000)])
    cols = np.concatenate([rng.choice(n, 30000, replace=False),
                           rng.choice(n, 9000, replace=False), rng.randint(0, n, 50000)])
    a = sp.coo_matrix((np.ones(rows.size), (rows, cols)), shape=(n, n)).tocsr()
    a.sum_duplicates()
    a.sort_indices()
    a.data = rng.uniform(-1, 1, a.nnz)
    return (a.indptr.astype(np.int32), a.indices.astype(np.int32), a.data, n)


# name -> (band arguments, what launch_rowblocks_mv does with the windows at K = 8:
#          "staged": at every K, even with a tile per wavefront (8 copies); "unstaged": never at K = 8)
BANDS = {
    "band-400": (dict(n=6000, hw=400, dens=0.10), "staged"),
    "band-1500": (dict(n=6000, hw=1500, dens=0.10), "unstaged"),
    "band-wide": (dict(n=3000, hw=1500, dens=0.10, ncols=8000), "unstaged"),
    "band-tall": (dict(n=7000, hw=300, dens=0.20, ncols=3000), "staged"),
}

# The two runs of every band case.  Both pin the wavefront count: left to itself the launch tuner emits the
# stream again with smaller row-blocks where that is faster (autotune_launch of api.cpp), and the stream on the
# GPU would no longer be the one test_matmat_cases.py decoded.  "pinned" keeps one tile per workgroup as well,
# so that the plain family runs; "deterministic" runs the det family.
BAND_MODES = {
    "pinned": {"spx.gpu.waves": "4", "spx.gpu.wave_tiles": "false"},
    "deterministic": {"spx.gpu.waves": "4", "spx.gpu.deterministic": "true"},
}


def band_options(mode):
    return dict(NOSAMPLE, **BAND_MODES[mode])


# the general-path matrices of test_gpu_matmat.py: no precondition, their census line is printed
GENERAL = {
    "cant": (lambda: synth.syn_cant(0.05), NOSAMPLE),
    "webbase": (lambda: synth.syn_webbase(0.02), NOSAMPLE),
    "nlpkkt": (lambda: synth.syn_nlpkkt(20), NOSAMPLE),
    "phases-c2": (lambda: synth.syn_nlpkkt(20), dict(NOSAMPLE, **{"spx.gpu.col_phases": "c2"})),
}


# The 27 instantiations of spmv_mv_kernels.hip: K in {2, 4, 8} x waves in {2, 4, 8} x family.  The options that
# pin a family (launch_rowblocks_mv: det where a tile per wavefront is kept and the column slices do not run in
# one launch, accum where they do, else plain).  spx.gpu.rowblock_rows keeps the row-blocks of the det family
# small enough that a group of 8 fits MV_LDS_BUDGET with eight copies of the tiles (8 * 8 * rows <= 10240).
# Column slices lift that limit to 2048 rows (emit_and_upload of api.cpp: "a slice of a row is short") and a run of
# rows that hold nothing in a slice never closes a row-block (emit_gpu), so a banded matrix cut in two slices holds
# a row-block of up to 2048 rows and its group is 4 (8 * 2048 > 10240); the accum family reaches K = 8 on a matrix
# whose every row has nonzeros in both halves of the columns, with few enough of them per row-block.
FAMILIES = {
    "plain": {"spx.gpu.wave_tiles": "false", "spx.gpu.col_phases": "1"},
    "accum": {"spx.gpu.wave_tiles": "false", "spx.gpu.col_phases": "c2", "spx.gpu.rowblock_elems": "1000"},
    "det": {"spx.gpu.deterministic": "true", "spx.gpu.col_phases": "1", "spx.gpu.rowblock_rows": "16"},
}


def band_twice():
    """3000 x 6000: band(3000, 400, 0.10) next to a copy of itself, a band in each half of the columns."""
    _, m = band(3000, 400, 0.10)
    m = sp.hstack([m, m]).tocsr()
    m.sort_indices()
    return (m.indptr.astype(np.int32), m.indices.astype(np.int32), m.data.copy(), 3000), m


# name -> generator of (csr tuple, scipy matrix)
KERNEL_MATRICES = {
    "cant": lambda: (synth.syn_cant(0.05), to_scipy(synth.syn_cant(0.05))),
    "band-400": lambda: band(**BANDS["band-400"][0]),
    "band-twice": band_twice,
}
# (matrix, family) -> the group device_mv_group must return
KERNEL_TUNES = {
    ("cant", "plain"): 8, ("band-400", "plain"): 8,
    ("cant", "det"): 8, ("band-400", "det"): 8,
    ("band-twice", "accum"): 8, ("cant", "accum"): 4,
}
KERNEL_WAVES = (2, 4, 8)


def kernel_options(family, waves):
    return dict(NOSAMPLE, **dict(FAMILIES[family], **{"spx.gpu.waves": str(waves)}))


def expected_group(rows, copies):
    """device_mv_group of device_runtime.cpp for row-blocks of up to `rows` rows."""
    for K in (8, 4, 2):
        if K * copies * rows <= MV_LDS_BUDGET_DOUBLES:
            return K
    return 1


def census(path):
    """(kind-4 passes, largest x window in doubles, largest row-block in rows) of a saved stream; the windows
    counted are those of row-blocks that hold a kind-4 pass."""
    s = Stream(path)
    n4, xwin = 0, 0
    for rb in s.rbs:
        k = int((s.passes[int(rb["pass_off"]):int(rb["pass_off"]) + int(rb["n_pass"])]["kind"] == PASS_GATHER_LDS).sum())
        n4 += k
        if k:
            xwin = max(xwin, int(rb["xwin_len"]))
    return n4, xwin, int(s.rbs["n_rows"].max()) if len(s.rbs) else 0


def load_rect(sx, csr, ncols, opts=None, host_only=False):
    """helpers.tune for a matrix of csr[3] x ncols."""
    rp, ci, va, n = csr
    sx.options_reset()
    if host_only:
        sx.option_set("spx.rt.host_only", "true")
    for k, v in (opts or {}).items():
        sx.option_set(k, v)
    inp = sx.input_load_csr(rp, ci, va, n, ncols)
    A = sx.mat_tune(inp)
    A._input = inp
    return A


def block(torch, n, nvec, pad, seed0, fill=None):
    """(nvec, n) float64 view into an (nvec, n + pad) tensor whose padding holds NaN."""
    full = torch.full((nvec, n + pad), float("nan"), dtype=torch.float64, device="cuda")
    view = full[:, :n]
    if fill is None:
        for j in range(nvec):
            view[j] = torch.from_numpy(synth.random_x(n, seed=seed0 + j))
    else:
        view.fill_(fill)
    return full, view


def check_columns(a, Xh, Yh, alpha, beta, y0):
    """helpers.check_y on every column; `a` is the scipy CSR matrix (any shape)."""
    csr = (a.indptr, a.indices, a.data, a.shape[0])
    for j in range(Xh.shape[0]):
        check_y_rect(a, csr, Xh[j], Yh[j], alpha, beta, y0[j] if beta != 0.0 else None)


def check_y_rect(a, csr, x, y, alpha, beta, y0):
    """helpers.check_y, whose bound multiplies with a square |A|: a rectangular matrix is padded with empty
    rows or columns to a square one (x and y with zeros), which changes neither the product nor the bound."""
    nr, nc = a.shape
    if nr == nc:
        return check_y(csr, x, y, alpha, beta, y0)
    n = max(nr, nc)
    rp = np.concatenate([a.indptr, np.full(n - nr, a.indptr[-1], dtype=a.indptr.dtype)])
    pad = lambda v, k: None if v is None else np.concatenate([v, np.zeros(n - k)])
    return check_y((rp, a.indices, a.data, n), pad(x, nc), pad(y, nr), alpha, beta, pad(y0, nr))


def run(torch, A, a, nvec, alpha, beta, padx=0, pady=0, ref=None):
    """A.matmat on nvec random vectors (NaN behind every vector; beta == 0: Y starts as NaN), every column
    against the CSR product of the scipy matrix `a`.  ref: a function (X, y0 tensor, alpha, beta) -> Y1 that
    every column must equal bit for bit.  Returns Y on the host."""
    nr, nc = a.shape
    xf, X = block(torch, nc, nvec, padx, 11)
    yf, Y = block(torch, nr, nvec, pady, 101, None if beta != 0.0 else float("nan"))
    y0d = Y.clone()
    y0 = y0d.cpu().numpy()
    A.matmat(alpha, X, beta, Y)
    torch.cuda.synchronize()
    Xh, Yh = X.cpu().numpy(), Y.cpu().numpy()
    check_columns(a, Xh, Yh, alpha, beta, y0)
    if pady:
        assert torch.isnan(yf[:, nr:]).all(), "the padding of Y was written"
    if padx:
        assert torch.isnan(xf[:, nc:]).all()
    if ref is not None:
        Y1 = ref(X, y0d, alpha, beta)
        torch.cuda.synchronize()
        assert torch.equal(Y, Y1), "column differs from the single-vector product"
    return Yh


def single_vector_columns(torch, A):
    """run()'s `ref`: hip_matvec_kernel column by column."""
    def ref(X, y0d, alpha, beta):
        s = torch.cuda.current_stream().cuda_stream
        Y1 = y0d.clone()
        for j in range(X.shape[0]):
            A.hip_matvec_kernel(alpha, X[j].data_ptr(), beta, Y1[j].data_ptr(), s)
        return Y1
    return ref


def to_scipy(csr, ncols=None):
    rp, ci, va, n = csr
    return sp.csr_matrix((va, ci, rp), shape=(n, n if ncols is None else ncols))
