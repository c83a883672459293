"""The multi-vector product on row-major (interleaved) blocks, spx_hip_matmat_rm_kernel / Matrix.matmat_rm, on the
GPU: entry (i, j) of X at X[i * ldx + j], of Y at Y[i * ldy + j].  Every column against the CSR product
(helpers.check_y) on the general streams of test_gpu_matmat.py -- unit, inline, gather and window passes, over-long
rows, column phases, column slices in one launch -- over every group width and remainder chain, with and without
padding behind the rows; the padding and beta = 0 over NaN; bases 8 bytes off a 16-byte boundary; the 36 kernel
instances (matmat_cases.FAMILIES x K x waves); band matrices with staged and unstaged windows; bit-identity with
the single-vector product under spx.gpu.deterministic; a row slice; the refusals; nvec = 0; a captured graph.

The LDS formula is the column-major product's (mv_lds_bytes of device_runtime.cpp: K * (copies * rows + window)
doubles against 80 KB), so the staging preconditions of matmat_cases.BANDS, which test_matmat_cases.py proves on the
CPU, hold here unchanged and matmat_rm_group() must equal matmat_group() on every general tune."""
import numpy as np
import pytest
import scipy.sparse as sp

import sparsex_amd as sx
from sparsex_amd import synth
from helpers import check_y, tune
from test_gpu_matmat import CASES as MATMAT_CASES
import matmat_cases as mc

pytestmark = pytest.mark.gpu

NVECS = (1, 2, 3, 5, 8, 11)
GENERAL_CASES = ("demopatt", "cant", "webbase", "nlpkkt", "long-rows", "waves2", "waves8", "phases-c2", "phases-c4",
                 "phases-2", "unit-windows", "no-x-window")
NAN = float("nan")


@pytest.fixture(scope="module")
def tuned():
    cache = {}

    def get(name):
        if name not in cache:
            gen, opts, sym, _ = MATMAT_CASES[name]
            assert not sym
            csr = gen()
            cache[name] = (csr, tune(csr, opts))
        return cache[name]
    yield get
    cache.clear()
    sx.options_reset()


def rm_block(torch, n, nvec, ld, seed0, fill=None, offset=0):
    """(n, nvec) float64 view with stride(0) == ld into a flat NaN buffer, starting at element `offset` of it;
    column j holds random_x(n, seed0 + j), or `fill`.  Returns (flat buffer, view)."""
    flat = torch.full((offset + max(n, 1) * ld,), NAN, dtype=torch.float64, device="cuda")
    view = flat[offset:offset + n * ld].view(n, ld)[:, :nvec]
    if fill is None:
        cols = np.stack([synth.random_x(n, seed=seed0 + j) for j in range(nvec)], axis=1) if nvec else np.zeros((n, 0))
        view.copy_(torch.from_numpy(cols))
    else:
        view.fill_(fill)
    return flat, view


def padding_bits(torch, flat, view, n, nvec, ld, offset=0):
    """the bit patterns of every position of the flat buffer outside the view"""
    mask = torch.ones(flat.shape, dtype=torch.bool, device=flat.device)
    mask[offset:offset + n * ld].view(n, ld)[:, :nvec] = False
    return flat.view(torch.int64)[mask].clone()


def run_rm(torch, A, a, nvec, alpha, beta, ldx=None, ldy=None, ref=None, offset=0):
    """A.matmat_rm on nvec random vectors (NaN in every padding position of X and Y; beta == 0: all of Y starts as
    NaN), every column against the CSR product of the scipy matrix `a`; the padding of Y keeps its bits and no
    result is NaN.  ref: a function (X, y0 tensor, alpha, beta) -> Y1 of shape (nvec, nrows) that every column
    must equal bit for bit."""
    nr, nc = a.shape
    ldx = nvec if ldx is None else ldx
    ldy = nvec if ldy is None else ldy
    xf, X = rm_block(torch, nc, nvec, ldx, 11, offset=offset)
    yf, Y = rm_block(torch, nr, nvec, ldy, 101, None if beta != 0.0 else NAN, offset=offset)
    assert X.stride(0) == ldx and Y.stride(0) == ldy and X.data_ptr() % 16 == (8 * offset) % 16
    y0d = Y.clone()
    y0 = y0d.cpu().numpy()
    pad_before = padding_bits(torch, yf, Y, nr, nvec, ldy, offset)
    xf_before = xf.view(torch.int64).clone()
    A.matmat_rm(alpha, X, beta, Y)
    torch.cuda.synchronize()
    Xh, Yh = X.cpu().numpy(), Y.cpu().numpy()
    assert not np.isnan(Yh).any(), "a result is NaN"
    mc.check_columns(a, np.ascontiguousarray(Xh.T), np.ascontiguousarray(Yh.T), alpha, beta,
                     np.ascontiguousarray(y0.T))
    assert torch.equal(padding_bits(torch, yf, Y, nr, nvec, ldy, offset), pad_before), "the padding of Y was written"
    assert torch.equal(xf.view(torch.int64), xf_before), "X was written"
    if ref is not None:
        Y1 = ref(X, y0d, alpha, beta)
        torch.cuda.synchronize()
        assert torch.equal(Y.t(), Y1), "column differs from the single-vector product"
    return Yh


def single_vector_columns(torch, A):
    """run_rm()'s `ref`: hip_matvec_kernel on a contiguous copy of every column."""
    def ref(X, y0d, alpha, beta):
        s = torch.cuda.current_stream().cuda_stream
        Xc = X.t().contiguous()
        Y1 = y0d.t().contiguous()
        for j in range(Xc.shape[0]):
            A.hip_matvec_kernel(alpha, Xc[j].data_ptr(), beta, Y1[j].data_ptr(), s)
        return Y1
    return ref


# ---- 1. columns against CSR -------------------------------------------------------------------------------

@pytest.mark.parametrize("name", GENERAL_CASES)
def test_columns_match_the_csr_product(tuned, name):
    """nvec 1 .. 11: every group width (8, 4, 2, 1), every remainder chain (3 = 2 + 1, 5 = 4 + 1, 11 = 8 + 2 + 1)
    and odd column offsets j0; ld == nvec and ld == nvec + 3: with an odd ld every other row is 8- but not 16-byte
    aligned, and the 8-byte loads run."""
    import torch
    csr, A = tuned(name)
    a = mc.to_scipy(csr)
    g = A.matmat_rm_group()
    assert g >= 2 and g == A.matmat_group(), "%s: group %d (column-major: %d)" % (name, g, A.matmat_group())
    for k, nvec in enumerate(NVECS):
        alpha, beta = mc.ALPHA_BETA[k % 3]
        run_rm(torch, A, a, nvec, alpha, beta)
        alpha, beta = mc.ALPHA_BETA[(k + 1) % 3]
        run_rm(torch, A, a, nvec, alpha, beta, ldx=nvec + 3, ldy=nvec + 3)


# ---- 2. padding and NaN -----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["cant", "webbase", "long-rows", "phases-c2"])
def test_padding_and_beta_zero_over_nan(tuned, name):
    """(run_rm fills the padding of X and of Y with NaN, for beta == 0 all of Y, and compares the bits of Y's
    padding; here with leading dimensions that differ between X and Y)"""
    import torch
    csr, A = tuned(name)
    a = mc.to_scipy(csr)
    run_rm(torch, A, a, 5, 0.5, 0.0, ldx=12, ldy=14)
    run_rm(torch, A, a, 8, 1.0, 0.0, ldx=9, ldy=9)
    run_rm(torch, A, a, 8, 1.0, 0.0, ldx=8, ldy=16)


# ---- 3. misaligned base -----------------------------------------------------------------------------------

@pytest.mark.parametrize("nvec", [2, 4, 8])
@pytest.mark.parametrize("name", ["cant", "webbase"])
def test_base_eight_bytes_off_a_16_byte_boundary(tuned, name, nvec):
    import torch
    csr, A = tuned(name)
    run_rm(torch, A, mc.to_scipy(csr), nvec, 2.0, -0.5, offset=1)
    run_rm(torch, A, mc.to_scipy(csr), nvec, 0.5, 0.0, ldx=nvec + 2, ldy=nvec + 2, offset=1)


# ---- 4. the 36 kernel instances ---------------------------------------------------------------------------

ALL_KERNELS = {(f, K, w) for f in mc.FAMILIES for K in (1, 2, 4, 8) for w in mc.KERNEL_WAVES}


@pytest.fixture(scope="module")
def kernel_runs():
    """(matrix, family, waves) -> the (family, K, waves) instances that ran, each run checked."""
    import torch
    done, mats = {}, {}

    def ensure(matrix, family, waves):
        key = (matrix, family, waves)
        if key in done:
            return done[key]
        if matrix not in mats:
            mats[matrix] = mc.KERNEL_MATRICES[matrix]()
        csr, a = mats[matrix]
        A = mc.load_rect(sx, csr, a.shape[1], mc.kernel_options(family, waves))
        inf, g = A.info(), A.matmat_rm_group()
        assert g == mc.KERNEL_TUNES[(matrix, family)]
        # launch_rowblocks_mv: accum where the column slices run in one launch, else det where a tile per
        # wavefront is kept, else plain; launch_spmv_mvr: the matrix' wavefront count
        ran_family = "accum" if inf.col_slices > 1 else "det" if inf.wave_tiles else "plain"
        ran = set()
        for k, nvec in enumerate((1, 2, 4, 8)):
            alpha, beta = mc.ALPHA_BETA[k % 3]
            run_rm(torch, A, a, nvec, alpha, beta, ldx=nvec + (k % 2), ldy=nvec + 2 * (k % 2),
                   ref=single_vector_columns(torch, A) if ran_family == "det" else None)
            ran.add((ran_family, min(g, nvec), int(inf.waves)))
        done[key] = ran
        return ran
    yield ensure
    done.clear()
    mats.clear()
    sx.options_reset()


@pytest.mark.parametrize("waves", mc.KERNEL_WAVES)
@pytest.mark.parametrize("matrix,family", list(mc.KERNEL_TUNES))
def test_pinned_family_and_waves_run(kernel_runs, matrix, family, waves):
    g = mc.KERNEL_TUNES[(matrix, family)]
    assert kernel_runs(matrix, family, waves) == {(family, K, waves) for K in (1, 2, 4, 8) if K <= g}


def test_all_36_instances_ran(kernel_runs):
    seen = set()
    for (matrix, family) in mc.KERNEL_TUNES:
        for waves in mc.KERNEL_WAVES:
            seen |= kernel_runs(matrix, family, waves)
    assert len(ALL_KERNELS) == 36
    missing = ALL_KERNELS - seen
    assert not missing, "instances that never ran: %s" % sorted(missing)


@pytest.mark.parametrize("mode", list(mc.BAND_MODES))
@pytest.mark.parametrize("name", list(mc.BANDS))
def test_band_windows_staged_and_gathered(name, mode):
    """nvec 13 = 8 + 4 + 1 and 7 = 4 + 2 + 1: the windows of the "unstaged" cases go through L2 at K = 8 and through
    LDS at narrower groups within one call (the same LDS formula as the column-major product, so the preconditions
    of matmat_cases.BANDS carry over).  band-wide and band-tall are rectangular."""
    import torch
    kw, _ = mc.BANDS[name]
    csr, a = mc.band(**kw)
    det = mode == "deterministic"
    A = mc.load_rect(sx, csr, a.shape[1], mc.band_options(mode))
    assert A.matmat_rm_group() == 8
    assert bool(A.info().wave_tiles) == det
    ref = single_vector_columns(torch, A) if det else None
    k = 0
    for nvec in (13, 7):
        for alpha, beta in mc.ALPHA_BETA:
            run_rm(torch, A, a, nvec, alpha, beta, ldx=nvec + k % 2, ldy=nvec + 3 - k % 2, ref=ref)
            k += 1


# ---- 5. bit-identity under determinism --------------------------------------------------------------------

@pytest.mark.parametrize("gen", [lambda: synth.syn_cant(0.05), lambda: synth.syn_webbase(0.02)], ids=["cant", "webbase"])
def test_deterministic_columns_are_bit_identical(gen):
    import torch
    csr = gen()
    A = tune(csr, dict(mc.NOSAMPLE, **{"spx.gpu.deterministic": "true"}))
    assert A.matmat_rm_group() >= 2
    a = mc.to_scipy(csr)
    ref = single_vector_columns(torch, A)
    for nvec in (1, 3, 8):
        run_rm(torch, A, a, nvec, 0.5, 0.25, ldx=nvec + 3, ldy=nvec + 1, ref=ref)
        run_rm(torch, A, a, nvec, 0.5, 0.0, ldx=nvec + 2, ldy=nvec + 2, ref=ref)


# ---- 6. row slice -----------------------------------------------------------------------------------------

def test_row_slice_writes_the_rows_of_the_single_product():
    import torch
    N = 12
    n = synth.nlpkkt_nrows(N)
    lo, hi = n // 4, (3 * n) // 4
    rl, cl, vl, _ = synth.syn_nlpkkt_rows(N, lo, hi)
    sx.options_reset()
    opts = dict(mc.NOSAMPLE, **{"spx.rt.row_offset": str(lo), "spx.rt.global_rows": str(n)})
    for k, v in opts.items():
        sx.option_set(k, v)
    inp = sx.input_load_csr(rl, cl, vl, hi - lo, n)
    A = sx.mat_tune(inp)
    assert A.nrows == n
    s = torch.cuda.current_stream().cuda_stream
    for nvec, beta in ((3, 0.0), (5, 0.5)):
        _, X = rm_block(torch, A.ncols, nvec, nvec + 1, 7)
        yf, Y = rm_block(torch, A.nrows, nvec, nvec + 2, 0, 123.0)
        Xc = X.t().contiguous()
        Y1 = Y.t().contiguous()
        A.matmat_rm(0.5, X, beta, Y)
        for j in range(nvec):
            A.hip_matvec_kernel(0.5, Xc[j].data_ptr(), beta, Y1[j].data_ptr(), s)
        torch.cuda.synchronize()
        y, y1 = Y.t().cpu().numpy(), Y1.cpu().numpy()
        assert np.array_equal(y == 123.0, y1 == 123.0), "not the rows the single-vector product writes"
        assert (y1 != 123.0).any() and (y1 == 123.0).any()
        assert np.allclose(y, y1, rtol=1e-13, atol=1e-13)
        assert torch.isnan(yf.view(A.nrows, nvec + 2)[:, nvec:]).all(), "the padding of Y was written"
    del A
    inp.destroy()
    sx.options_reset()


# ---- 7. refusals ------------------------------------------------------------------------------------------

def test_symmetric_handle_is_refused():
    import torch
    csr = synth.syn_nlpkkt(12)
    n = csr[3]
    for opts in ({}, {"spx.gpu.sym_once": "false", "spx.gpu.sym_segments": "false"}):
        A = tune(csr, dict(mc.NOSAMPLE, **opts), sym=True)
        assert A.matmat_rm_group() == 0
        X = torch.ones((n, 2), dtype=torch.float64, device="cuda")
        Y = torch.full((n, 2), 7.0, dtype=torch.float64, device="cuda")
        with pytest.raises(sx.SpxError):
            A.matmat_rm(1.0, X, 0.0, Y)
        with pytest.raises(sx.SpxError):
            A.hip_matmat_rm_kernel(1.0, X.data_ptr(), 2, 1, 0.5, Y.data_ptr(), 2, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert (Y == 7.0).all() and (X == 1.0).all()
    sx.options_reset()


def test_matrix_with_an_exchange_plan_is_refused():
    """(a communicator of one rank, as in test_gpu_multirank.py::test_rccl_transport_single_rank)"""
    import torch
    csr = synth.syn_cant(0.05)
    n = csr[3]
    t = sx.RcclTransport(sx.rccl_unique_id(), 0, 1)
    A = tune(csr, mc.NOSAMPLE)
    assert A.matmat_rm_group() >= 2
    A.dist_attach(t)
    X = torch.ones((n, 2), dtype=torch.float64, device="cuda")
    Y = torch.full((n, 2), 7.0, dtype=torch.float64, device="cuda")
    with pytest.raises(sx.SpxError):
        A.matmat_rm(1.0, X, 0.0, Y)
    torch.cuda.synchronize()
    assert (Y == 7.0).all() and (X == 1.0).all()
    A.destroy()
    t.destroy()
    sx.options_reset()


def test_bad_arguments_fail(tuned):
    import torch
    csr, A = tuned("cant")
    n = csr[3]
    s = torch.cuda.current_stream().cuda_stream
    buf = torch.zeros((4 * n,), dtype=torch.float64, device="cuda")
    base = buf.data_ptr()
    with pytest.raises(sx.SpxError):                      # X and Y overlap: Y starts inside X
        A.hip_matmat_rm_kernel(1.0, base, 2, 2, 0.0, base + 8 * n, 2, s)
    with pytest.raises(sx.SpxError):                      # the same block
        A.hip_matmat_rm_kernel(1.0, base, 2, 1, 0.0, base, 2, s)
    with pytest.raises(sx.SpxError):                      # interleaved with each other: ranges meet
        A.hip_matmat_rm_kernel(1.0, base, 4, 2, 0.0, base + 16, 4, s)
    with pytest.raises(sx.SpxError):                      # ldx < nvec
        A.hip_matmat_rm_kernel(1.0, base, 1, 2, 0.0, base + 16 * n, 2, s)
    with pytest.raises(sx.SpxError):                      # ldy < nvec
        A.hip_matmat_rm_kernel(1.0, base, 2, 2, 0.0, base + 16 * n, 1, s)
    with pytest.raises(sx.SpxError):                      # NULL X
        A.hip_matmat_rm_kernel(1.0, 0, 2, 2, 0.0, base + 16 * n, 2, s)
    with pytest.raises(sx.SpxError):                      # NULL Y
        A.hip_matmat_rm_kernel(1.0, base, 2, 2, 0.0, 0, 2, s)
    with pytest.raises(sx.SpxError):                      # rows 2^62 doubles apart: past the address space
        A.hip_matmat_rm_kernel(1.0, base, 1 << 62, 2, 0.0, base + 16 * n, 2, s)
    with pytest.raises(sx.SpxError):                      # ... of Y
        A.hip_matmat_rm_kernel(1.0, base, 2, 2, 0.0, base + 16 * n, 1 << 62, s)
    torch.cuda.synchronize()
    assert not buf.any()
    # (adjacent, not overlapping: fine)
    X = buf[:2 * n].view(n, 2)
    X.copy_(torch.from_numpy(np.stack([synth.random_x(n, seed=j) for j in range(2)], axis=1)))
    A.hip_matmat_rm_kernel(1.0, base, 2, 2, 0.0, base + 16 * n, 2, s)
    torch.cuda.synchronize()
    Y = buf[2 * n:].view(n, 2)
    for j in range(2):
        check_y(csr, X[:, j].cpu().numpy(), Y[:, j].cpu().numpy(), 1.0)


# ---- 8. no-op and capture ---------------------------------------------------------------------------------

def test_zero_vectors_is_a_no_op(tuned):
    import torch
    csr, A = tuned("cant")
    n = csr[3]
    X = torch.zeros((n, 0), dtype=torch.float64, device="cuda")
    Y = torch.zeros((n, 0), dtype=torch.float64, device="cuda")
    A.matmat_rm(1.0, X, 0.0, Y)
    A.hip_matmat_rm_kernel(1.0, 0, 0, 0, 0.0, 0, 0, torch.cuda.current_stream().cuda_stream)
    # (and nothing is touched where the pointers are real)
    Z = torch.full((n, 3), 5.0, dtype=torch.float64, device="cuda")
    A.hip_matmat_rm_kernel(1.0, Z.data_ptr(), 3, 0, 0.0, Z.data_ptr(), 3, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert (Z == 5.0).all()


def test_captured_matmat_rm_replays(tuned):
    import torch
    csr, A = tuned("nlpkkt")
    rp, ci, va, n = csr
    nvec = 5
    _, X = rm_block(torch, n, nvec, nvec + 2, 51)
    Y = torch.zeros((n, nvec), dtype=torch.float64, device="cuda")
    A.matmat_rm(0.5, X, 0.0, Y)                                     # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(4):                                          # Y <- 0.5 A X + 0.25 Y, four times
            A.matmat_rm(0.5, X, 0.25, Y)
    a = sp.csr_matrix((va, ci, rp), shape=(n, n))
    for rep in range(3):                                            # new inputs, same graph
        X.copy_(torch.from_numpy(np.stack([synth.random_x(n, seed=500 + 10 * rep + j) for j in range(nvec)], axis=1)))
        Y.fill_(float(rep))
        g.replay()
        torch.cuda.synchronize()
        Xh, Yh = X.cpu().numpy(), Y.cpu().numpy()
        ref = np.full((n, nvec), float(rep))
        for _ in range(4):
            ref = 0.5 * (a @ Xh) + 0.25 * ref
        assert np.allclose(Yh, ref, rtol=1e-12, atol=1e-13)
