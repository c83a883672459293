"""The multi-vector product with the float copy of the values on column-major blocks, spx_hip_matmat_kernel_f32 /
Matrix.matmat_f32, on the GPU: the plain, accum and det families of csx_spmv_mv_kernel<MvArgs, float, ...>
(spmv_mv_f32_kernels.hip) on handles tuned with spx.gpu.values_f32.

The reference of every result is matmat_cases.check_y_rect -- the project's fp64 bound and its relative 1e-6
criterion -- on the CSR arrays with values.astype(float32).astype(float64), as in test_gpu_values_f32.py, whose
helpers this file uses.  That the floats are really read (and no fp64 kernel stands in) shows per column with
assert_reads_floats: the result lies beyond the fp64 bound of the product with A itself on at least half the
non-empty rows.  Column j of X is synth.random_x with seed 5 + j, column j of a Y that is read with seed 100 + j; on
the matrices used here (matmat_cases.KERNEL_MATRICES, long_rows, BANDS) the CSR product of the rounded values lies
beyond A's bound on every non-empty row or all but one (checked on the CPU for the seeds 5, 8 and 15), so the
condition holds for the reference with a wide margin.  Matrices, vectors and handles are shared per module."""
import numpy as np
import pytest
import scipy.sparse as sp

import sparsex_amd as sx
from sparsex_amd import synth
from helpers import check_y
import dist_cases as dc
import matmat_cases as mc
import values_cases as vc
import test_gpu_transpose as tt
from test_gpu_values_f32 import ON, OPT, Shared, assert_reads_floats, rounded

pytestmark = pytest.mark.gpu

NVECS = (2, 3, 5, 8, 11)             # K = 8, 4, 2 and the single-vector remainder (3 = 2 + 1, 11 = 8 + 2 + 1)
ALL = {OPT: "all"}
NAN = float("nan")
X_SEED, Y_SEED = 5, 100


@pytest.fixture(scope="module")
def shared():
    import torch
    s = Shared(torch)
    yield s
    for A in s.tuned.values():
        A.destroy()
    s.tuned.clear()
    s.mats.clear()
    s.xs.clear()
    sx.options_reset()
    torch.cuda.empty_cache()


def cm_block(torch, n, nvec, pad, offset=0):
    """(nvec, n) view with stride(0) == n + pad into a flat buffer of NaN, starting at its element `offset`"""
    ld = n + pad
    flat = torch.full((offset + max(nvec, 1) * ld,), NAN, dtype=torch.float64, device="cuda")
    return flat, flat[offset:offset + nvec * ld].view(nvec, ld)[:, :n]


def outside(torch, flat, n, nvec, pad, offset=0):
    """the positions of the flat buffer that are not the view's"""
    mask = torch.ones(flat.shape, dtype=torch.bool, device=flat.device)
    mask[offset:offset + nvec * (n + pad)].view(nvec, n + pad)[:, :n] = False
    return flat[mask]


def columns(shared, n, nvec, seed0):
    return np.stack([shared.x(n, seed=seed0 + j)[0] for j in range(nvec)]) if nvec else np.zeros((0, n))


def float_columns(torch, A):
    """run_f32()'s `ref`: hip_matvec_kernel_f32 column by column"""
    def ref(X, Y0, alpha, beta):
        s = torch.cuda.current_stream().cuda_stream
        Y1 = Y0.clone()
        for j in range(X.shape[0]):
            A.hip_matvec_kernel_f32(alpha, X[j].data_ptr(), beta, Y1[j].data_ptr(), s)
        return Y1
    return ref


def run_f32(shared, A, mat, nvec, alpha, beta, padx=3, pady=5, offset=0, ref=None, beyond=True, what=""):
    """A.matmat_f32 on nvec columns inside NaN-padded blocks (ldx = ncols + padx, ldy = nrows + pady; beta == 0:
    all of Y starts as NaN): every column against the CSR product of the ROUNDED values and (alpha != 0) beyond the
    bound of the unrounded one; the padding stays NaN, X keeps its bits.  ref: a function (X, Y0, alpha, beta) -> Y1
    that Y must equal bit for bit.  Returns Y (device)."""
    torch = shared.torch
    csr, m, m32, csr32 = mat
    nr, nc = m.shape
    Xh = columns(shared, nc, nvec, X_SEED)
    y0h = columns(shared, nr, nvec, Y_SEED)
    xf, X = cm_block(torch, nc, nvec, padx, offset)
    yf, Y = cm_block(torch, nr, nvec, pady, offset)
    X.copy_(torch.from_numpy(Xh))
    if beta != 0.0:
        Y.copy_(torch.from_numpy(y0h))
    assert X.data_ptr() % 16 == (8 * offset) % 16 and Y.data_ptr() % 16 == (8 * offset) % 16
    assert nvec < 2 or (X.stride(0) == nc + padx and Y.stride(0) == nr + pady)
    Y0 = Y.clone()
    x_bits = xf.view(torch.int64).clone()
    out = A.matmat_f32(alpha, X, beta, Y)
    torch.cuda.synchronize()
    assert out is Y
    Yh = Y.cpu().numpy()
    assert not np.isnan(Yh).any(), "a result is NaN"
    assert torch.isnan(outside(torch, yf, nr, nvec, pady, offset)).all(), "the padding of Y was written"
    assert torch.equal(xf.view(torch.int64), x_bits), "X was written"
    for j in range(nvec):
        mc.check_y_rect(m32, csr32, Xh[j], Yh[j], alpha, beta, y0h[j] if beta != 0.0 else None)
        if beyond and alpha != 0.0:
            assert_reads_floats(mat, Xh[j], Yh[j], alpha, beta, y0h[j], "%s nvec %d column %d alpha %g beta %g" % (
                what, nvec, j, alpha, beta))
    if ref is not None:
        Y1 = ref(X, Y0, alpha, beta)
        torch.cuda.synchronize()
        assert torch.equal(Y, Y1), "a column differs from the single float product"
    return Y


def groups_of(g, nvec):
    """the group widths device_spmm_f32 serves nvec vectors with"""
    ks, j = [], 0
    while j < nvec:
        K = g
        while K > 1 and K > nvec - j:
            K //= 2
        ks.append(K)
        j += K
    return ks


# ---- 1. the 27 instances -------------------------------------------------------------------------------------------

ALL_KERNELS = {(f, K, w) for f in mc.FAMILIES for K in (2, 4, 8) for w in mc.KERNEL_WAVES}


@pytest.fixture(scope="module")
def kernel_runs(shared):
    """(matrix, family, waves) -> the (family, K, waves) instances that ran, each run checked"""
    done = {}

    def ensure(matrix, family, waves):
        key = (matrix, family, waves)
        if key in done:
            return done[key]
        torch = shared.torch
        mat = shared.matrix("k-" + matrix, mc.KERNEL_MATRICES[matrix])
        A = shared.load(("kernel",) + key, mat[0], mat[1], dict(mc.kernel_options(family, waves), **ON))
        inf, g = A.info(), A.matmat_group_f32()
        assert g == mc.KERNEL_TUNES[(matrix, family)] == A.matmat_group()
        assert A.values_f32_bytes() == 4 * (inf.value_bytes // 8) > 0
        # launch_rowblocks_mv: accum where the column slices run in one launch, else det where a tile per
        # wavefront is kept, else plain; launch_spmv_mv_f32: the matrix' wavefront count
        ran_family = "accum" if inf.col_slices > 1 else "det" if inf.wave_tiles else "plain"
        ref = float_columns(torch, A) if ran_family == "det" else None
        what = "%s %s waves %d" % key
        ran = set()
        for nvec in NVECS:
            for alpha, beta in mc.ALPHA_BETA:
                run_f32(shared, A, mat, nvec, alpha, beta, ref=ref, what=what)
            ran |= {(ran_family, K, int(inf.waves)) for K in groups_of(g, nvec) if K > 1}
        # every column 8 bytes off a 16-byte boundary (an even leading dimension behind an odd offset)
        nr, nc = mat[1].shape
        run_f32(shared, A, mat, 11, 2.0, -0.5, padx=2 + nc % 2, pady=4 + nr % 2, offset=1, ref=ref, what=what + " at 8 mod 16")
        shared.drop(("kernel",) + key)
        done[key] = ran
        return ran
    yield ensure
    done.clear()


@pytest.mark.parametrize("waves", mc.KERNEL_WAVES)
@pytest.mark.parametrize("matrix,family", list(mc.KERNEL_TUNES))
def test_pinned_family_and_waves_run(kernel_runs, matrix, family, waves):
    g = mc.KERNEL_TUNES[(matrix, family)]
    assert kernel_runs(matrix, family, waves) == {(family, K, waves) for K in (2, 4, 8) if K <= g}


def test_all_27_instances_ran(kernel_runs):
    seen = set()
    for (matrix, family) in mc.KERNEL_TUNES:
        for waves in mc.KERNEL_WAVES:
            seen |= kernel_runs(matrix, family, waves)
    assert len(ALL_KERNELS) == 27
    missing = ALL_KERNELS - seen
    assert not missing, "instances that never ran: %s" % sorted(missing)


# ---- 2. carry slots, windows, a rectangular matrix -------------------------------------------------------------------

def test_long_rows_through_carry_slots_and_fixup(shared):
    mat = shared.matrix("long-rows", lambda: (mc.long_rows(), None))
    A = shared.load(("long-rows",), mat[0], mat[1], dict(mc.NOSAMPLE, **ON))
    assert A.matmat_group_f32() == A.matmat_group() >= 2
    for k, nvec in enumerate(NVECS):
        alpha, beta = mc.ALPHA_BETA[k % 3]
        run_f32(shared, A, mat, nvec, alpha, beta, what="long-rows")
    shared.drop(("long-rows",))


@pytest.mark.parametrize("mode", list(mc.BAND_MODES))
@pytest.mark.parametrize("name", ["band-400", "band-1500", "band-wide"])
def test_band_windows_staged_and_gathered(shared, name, mode):
    """band-400: the x windows staged in LDS at every K; band-1500 and the rectangular band-wide: never staged at
    K = 8, staged at narrower groups within one call (13 = 8 + 4 + 1, 7 = 4 + 2 + 1) -- the staging rule of the fp64
    product, whose preconditions test_matmat_cases.py proves on the CPU"""
    torch = shared.torch
    kw, _ = mc.BANDS[name]
    mat = shared.matrix(name, lambda: mc.band(**kw))
    det = mode == "deterministic"
    key = ("band", name, mode)
    A = shared.load(key, mat[0], mat[1], dict(mc.band_options(mode), **ON))
    assert A.matmat_group_f32() == 8 and bool(A.info().wave_tiles) == det
    ref = float_columns(torch, A) if det else None
    k = 0
    for nvec in (13, 7):
        for alpha, beta in mc.ALPHA_BETA:
            run_f32(shared, A, mat, nvec, alpha, beta, padx=1 + k % 2, pady=4 - k % 2, ref=ref, what="%s %s" % (name, mode))
            k += 1
    shared.drop(key)


# ---- 3. determinism ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["cant", "long-rows"])
def test_deterministic_columns_are_bit_identical(shared, name):
    """spx.gpu.deterministic=true: every column is A.matvec_f32 of that column bit for bit, and two block calls are
    bit-identical"""
    torch = shared.torch
    mat = shared.matrix(*{"cant": ("k-cant", mc.KERNEL_MATRICES["cant"]), "long-rows": ("long-rows", lambda: (mc.long_rows(), None))}[name])
    key = ("det", name)
    A = shared.load(key, mat[0], mat[1], dict(mc.NOSAMPLE, **dict({"spx.gpu.deterministic": "true"}, **ON)))
    assert A.matmat_group_f32() >= 2
    n = mat[0][3]
    nvec = 11
    X = torch.from_numpy(columns(shared, n, nvec, X_SEED)).cuda()
    Y0 = torch.from_numpy(columns(shared, n, nvec, Y_SEED)).cuda()
    for alpha, beta in ((0.5, 0.25), (0.5, 0.0)):
        Ys = [Y0.clone(), Y0.clone()]
        for Y in Ys:
            A.matmat_f32(alpha, X, beta, Y)
        Y1 = Y0.clone()
        for j in range(nvec):
            assert A.matvec_f32(alpha, X[j], beta, Y1[j]) is not None
        torch.cuda.synchronize()
        assert torch.equal(Ys[0], Ys[1]), "two block calls differ"
        assert torch.equal(Ys[0], Y1), "a column differs from matvec_f32"
    run_f32(shared, A, mat, 5, 0.5, 0.0, ref=float_columns(torch, A), what=name + " deterministic")
    shared.drop(key)


# ---- 4. symmetric streams (spx.gpu.values_f32=all) ----------------------------------------------------------------------

SYM_MATMAT = {"spx.gpu.sym_matmat": "true", "spx.gpu.wave_tiles": "false", "spx.gpu.waves": "4"}
# name -> (matrix name, generator, options, whether the K-vector kernels run)
SYM = {
    # no tiles, no read-once segments: the mirror image is stored, the mv kernels run and round the diagonal
    "no-once": ("kkt20", tt.SYM_CASES["no-once"][0], tt.SYM_CASES["no-once"][1], True),
    # the default symmetric tune: tiles and read-once segments, one float product per column
    "default": ("nd24k", tt.SYM_CASES["tiles"][0], tt.SYM_CASES["tiles"][1], False),
    # read-once passes for K vectors in fp64: csx_spmv_mvsym_kernel has no float form, and must not run
    "sym-matmat": ("nd24k", tt.SYM_CASES["tiles"][0], dict(tt.SYM_CASES["tiles"][1], **SYM_MATMAT), False),
}


@pytest.mark.parametrize("name", list(SYM))
def test_symmetric_streams(shared, name):
    """(syn_nlpkkt and syn_nd24k: the rounded product lies beyond A's own bound on every row,
    test_gpu_values_f32_sym.py)"""
    mname, gen, opts, native = SYM[name]
    mat = shared.matrix("sym-" + mname, lambda: (gen(), None))
    key = ("sym", name)
    A = shared.load(key, mat[0], mat[1], dict(opts, **ALL), sym=True)
    inf = A.info()
    assert inf.symmetric and A.values_f32_bytes() == 4 * (inf.value_bytes // 8) > 0
    g, g64 = A.matmat_group_f32(), A.matmat_group()
    print("%s: float group %d, fp64 group %d, sym_tiles %d, sym_segments %d" % (name, g, g64, inf.sym_tiles, inf.sym_segments))
    if native:
        assert g == g64 >= 2
    else:
        assert g == 1
        assert (g64 >= 2) == (name == "sym-matmat"), "the fp64 product of this tune should%s run groups" % (
            "" if name == "sym-matmat" else " not")
    for nvec in ((2, 5, 11) if native else (3,)):
        for alpha, beta in mc.ALPHA_BETA:
            run_f32(shared, A, mat, nvec, alpha, beta, what="symmetric " + name)
    shared.drop(key)


# ---- 5. a row slice -----------------------------------------------------------------------------------------------------

def test_row_slices_write_the_rows_of_the_single_float_product(shared):
    """Ranks 0 and 1 of 2 in one process: each writes the rows matvec_f32 writes and no others, right against
    fl32(A)."""
    torch = shared.torch
    csr, m, m32, csr32 = shared.matrix("dist-nlpkkt", lambda: (dc.MATRICES["nlpkkt"](), None))
    n = csr[3]
    nvec = 5
    Xh = columns(shared, n, nvec, X_SEED)
    y0h = columns(shared, n, nvec, Y_SEED)
    opts = dict(dc.NOSAMPLE, **dict({"spx.gpu.waves": dc.WAVES, "spx.gpu.wave_tiles": "false"}, **ON))
    covered = 0
    for rank in range(2):
        A = dc.tune_rank(csr, rank, 2, opts)
        inf = A.info()
        lo, hi = inf.row_lo, inf.row_hi
        assert not inf.symmetric and 0 <= lo < hi <= n and hi - lo < n
        assert A.matmat_group_f32() == A.matmat_group() >= 2
        part32 = dc.general_part(m32, lo, hi)
        part = (None, sp.csr_matrix(dc.general_part(m, lo, hi)), sp.csr_matrix(part32), None)
        X = torch.from_numpy(Xh).cuda()
        for alpha, beta in mc.ALPHA_BETA:
            Y = torch.full((nvec, n), NAN, dtype=torch.float64, device="cuda")
            if beta != 0.0:
                Y[:, lo:hi] = torch.from_numpy(y0h[:, lo:hi].copy())
            Y1 = Y.clone()
            A.matmat_f32(alpha, X, beta, Y)
            for j in range(nvec):
                A.matvec_f32(alpha, X[j], beta, Y1[j])
            torch.cuda.synchronize()
            Yh, Y1h = Y.cpu().numpy(), Y1.cpu().numpy()
            assert np.array_equal(np.isnan(Yh), np.isnan(Y1h)), "not the rows the single float product writes"
            assert np.isnan(Yh[:, :lo]).all() and np.isnan(Yh[:, hi:]).all() and not np.isnan(Yh[:, lo:hi]).any()
            for j in range(nvec):
                own, y0 = np.zeros(n), np.zeros(n)
                own[lo:hi] = Yh[j, lo:hi]
                y0[lo:hi] = y0h[j, lo:hi]
                check_y((part32.indptr, part32.indices, part32.data, n), Xh[j], own, alpha, beta, y0 if beta != 0.0 else None)
                if alpha != 0.0:
                    assert_reads_floats(part, Xh[j], own, alpha, beta, y0, "rank %d column %d alpha %g" % (rank, j, alpha))
        covered += hi - lo
        A.destroy()
    assert covered == n


# ---- 6. refusals and the no-op ---------------------------------------------------------------------------------------------

def _assert_refused(torch, A, nvec=3):
    """both forms of the call fail, and Y keeps its 7s"""
    X = torch.ones((nvec, A.ncols), dtype=torch.float64, device="cuda")
    Y = torch.full((nvec, A.nrows), 7.0, dtype=torch.float64, device="cuda")
    with pytest.raises(sx.SpxError):
        A.matmat_f32(1.0, X, 0.0, Y)
    with pytest.raises(sx.SpxError):
        A.hip_matmat_kernel_f32(1.0, X.data_ptr(), A.ncols, nvec, 0.5, Y.data_ptr(), A.nrows, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert bool((Y == 7.0).all()) and bool((X == 1.0).all()), "a refused call wrote"


def test_handles_without_a_copy_are_refused(shared):
    """a general tune without the option, and a symmetric tune with =true (which symmetric tunes ignore): group 0,
    SPX_FAILURE, nothing written -- never the fp64 product"""
    torch = shared.torch
    mat = shared.matrix("k-cant", mc.KERNEL_MATRICES["cant"])
    A = shared.load(("no-copy", "general"), mat[0], mat[1], dict(mc.NOSAMPLE))
    assert A.values_f32_bytes() == 0 and A.matmat_group_f32() == 0 and A.matmat_group() >= 2
    _assert_refused(torch, A)
    shared.drop(("no-copy", "general"))
    smat = shared.matrix("sym-kkt20", lambda: (tt.SYM_CASES["no-once"][0](), None))
    for opts in (tt.SYM_CASES["no-once"][1], dict(mc.NOSAMPLE)):
        S = shared.load(("no-copy", "symmetric"), smat[0], smat[1], dict(opts, **ON), sym=True)
        assert S.info().symmetric and S.values_f32_bytes() == 0 and S.matmat_group_f32() == 0
        _assert_refused(torch, S)
        shared.drop(("no-copy", "symmetric"))


def test_bad_arguments_fail_and_zero_vectors_is_a_no_op(shared):
    torch = shared.torch
    mat = shared.matrix("k-cant", mc.KERNEL_MATRICES["cant"])
    A = shared.load(("args",), mat[0], mat[1], dict(mc.NOSAMPLE, **ON))
    n = mat[0][3]
    s = torch.cuda.current_stream().cuda_stream
    buf = torch.full((4, n), 7.0, dtype=torch.float64, device="cuda")
    base = buf.data_ptr()
    with pytest.raises(sx.SpxError):                      # X and Y overlap
        A.hip_matmat_kernel_f32(1.0, base, n, 2, 0.0, base + 8 * n, n, s)
    with pytest.raises(sx.SpxError):                      # the same block
        A.hip_matmat_kernel_f32(1.0, base, n, 1, 0.0, base, n, s)
    with pytest.raises(sx.SpxError):                      # ldx < ncols
        A.hip_matmat_kernel_f32(1.0, base, n - 1, 2, 0.0, base + 16 * n, n, s)
    with pytest.raises(sx.SpxError):                      # ldy < nrows
        A.hip_matmat_kernel_f32(1.0, base, n, 2, 0.0, base + 16 * n, n - 1, s)
    with pytest.raises(sx.SpxError):                      # NULL X, NULL Y
        A.hip_matmat_kernel_f32(1.0, 0, n, 2, 0.0, base + 16 * n, n, s)
    with pytest.raises(sx.SpxError):
        A.hip_matmat_kernel_f32(1.0, base, n, 2, 0.0, 0, n, s)
    # nvec == 0: nothing happens, whatever the pointers
    A.hip_matmat_kernel_f32(1.0, 0, n, 0, 0.0, 0, n, s)
    A.hip_matmat_kernel_f32(1.0, base, n, 0, 0.0, base, n, s)
    A.matmat_f32(1.0, buf[:0], 0.0, buf[:0])
    torch.cuda.synchronize()
    assert bool((buf == 7.0).all()), "a refused call or a call with no vectors wrote"
    # (adjacent, not overlapping: fine)
    Xh = columns(shared, n, 2, X_SEED)
    buf[:2] = torch.from_numpy(Xh).cuda()
    A.hip_matmat_kernel_f32(1.0, base, n, 2, 0.0, base + 16 * n, n, s)
    torch.cuda.synchronize()
    for j in range(2):
        check_y(mat[3], Xh[j], buf[2 + j].cpu().numpy(), 1.0)
    shared.drop(("args",))


# ---- 7. the doubles stay what they were; new values ---------------------------------------------------------------------------

def test_fp64_matmat_on_the_same_handle_does_not_see_the_copy(shared):
    """the fp64 block product of a handle with the copy lies within A's own bound, before and after a float one"""
    torch = shared.torch
    mat = shared.matrix("k-cant", mc.KERNEL_MATRICES["cant"])
    A = shared.load(("both",), mat[0], mat[1], dict(mc.NOSAMPLE, **ON))
    mc.run(torch, A, mat[1], 11, 2.0, -0.5, padx=3, pady=5)
    run_f32(shared, A, mat, 11, 2.0, -0.5, what="cant, between two fp64 products")
    mc.run(torch, A, mat[1], 8, 0.5, 0.0, padx=3, pady=5)
    shared.drop(("both",))


def test_set_values_reaches_the_float_block_product(shared):
    torch = shared.torch
    csr, m, m32, csr32 = shared.matrix("cant-small", lambda: (synth.syn_cant(0.02), None))
    A = vc.tune(csr, dict(mc.NOSAMPLE, **ON))
    assert A.matmat_group_f32() >= 2
    A.values_plan(csr[0], csr[1])
    for seed in (1, 2):
        v = vc.new_values(csr, False, seed)
        A.set_values(torch.from_numpy(v.copy()).cuda())
        new = shared.matrix(("cant-small", seed), lambda: (vc.with_values(csr, v), None))
        assert np.abs(rounded(v) - rounded(csr[2])).max() > 0.0
        run_f32(shared, A, new, 5, 0.5, 0.0, what="cant after set_values %d" % seed)
        run_f32(shared, A, new, 8, 2.0, -0.5, what="cant after set_values %d" % seed)
    A.destroy()


# ---- 8. a captured graph --------------------------------------------------------------------------------------------------------

def test_captured_matmat_f32_replays(shared):
    torch = shared.torch
    mat = shared.matrix("k-cant", mc.KERNEL_MATRICES["cant"])
    csr, m, m32, csr32 = mat
    A = shared.load(("capture",), csr, m, dict(mc.NOSAMPLE, **ON))
    n = csr[3]
    nvec = 5
    _, X = cm_block(torch, n, nvec, 2)
    X.copy_(torch.from_numpy(columns(shared, n, nvec, X_SEED)))
    Y = torch.zeros((nvec, n), dtype=torch.float64, device="cuda")
    A.matmat_f32(0.5, X, 0.0, Y)                                    # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        A.matmat_f32(0.5, X, 0.0, Y)
    for rep in range(2):                                            # new inputs, the same graph
        Xh = columns(shared, n, nvec, 40 + 10 * rep)
        X.copy_(torch.from_numpy(Xh))
        Y.fill_(NAN)
        g.replay()
        torch.cuda.synchronize()
        Yh = Y.cpu().numpy()
        for j in range(nvec):
            check_y(csr32, Xh[j], Yh[j], 0.5)
            assert_reads_floats(mat, Xh[j], Yh[j], 0.5, 0.0, None, "replay %d column %d" % (rep, j))
    shared.drop(("capture",))
