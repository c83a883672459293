"""The multi-vector product with the float copy of the values on row-major (interleaved) blocks,
spx_hip_matmat_rm_kernel_f32 / Matrix.matmat_rm_f32, on the GPU: the plain, accum and det
families of csx_spmv_mv_kernel<MvrArgs, float, ...> (spmv_mvr_f32_kernels.hip) on general handles tuned
with spx.gpu.values_f32=true.  Entry (i, j) of X at X[i * ldx + j], of Y at Y[i * ldy + j].

The reference of every column is matmat_cases.check_y_rect on the CSR arrays with
values.astype(float32).astype(float64), and every column must lie beyond the fp64 bound of the product with A itself
(assert_reads_floats), as in test_gpu_matmat_f32.py: column j of X is synth.random_x with seed 5 + j.  The 36
instances run by the scheme of test_gpu_matmat_rm.py::test_all_36_instances_ran."""
import numpy as np
import pytest

import sparsex_amd as sx
from helpers import check_y
import matmat_cases as mc
import test_gpu_transpose as tt
from test_gpu_values_f32 import ON, Shared, assert_reads_floats
from test_gpu_matmat_f32 import X_SEED, Y_SEED, columns, groups_of

pytestmark = pytest.mark.gpu

NVECS = (1, 2, 3, 5, 8, 11)
NAN = float("nan")


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


def rm_block(torch, n, nvec, ld, offset=0):
    """(n, nvec) view with stride(0) == ld into a flat buffer of NaN, starting at its element `offset`"""
    flat = torch.full((offset + max(n, 1) * ld,), NAN, dtype=torch.float64, device="cuda")
    return flat, flat[offset:offset + n * ld].view(n, ld)[:, :nvec]


def outside(torch, flat, n, nvec, ld, offset=0):
    """the positions of the flat buffer that are not the view's: j >= nvec of every row, and what lies in front"""
    mask = torch.ones(flat.shape, dtype=torch.bool, device=flat.device)
    mask[offset:offset + n * ld].view(n, ld)[:, :nvec] = False
    return flat[mask]


def float_columns(torch, A):
    """run_rm_f32()'s `ref`: hip_matvec_kernel_f32 on a contiguous copy of every column -> (nvec, nrows)"""
    def ref(X, Y0, alpha, beta):
        s = torch.cuda.current_stream().cuda_stream
        Xc = X.t().contiguous()
        Y1 = Y0.t().contiguous()
        for j in range(Xc.shape[0]):
            A.hip_matvec_kernel_f32(alpha, Xc[j].data_ptr(), beta, Y1[j].data_ptr(), s)
        return Y1
    return ref


def run_rm_f32(shared, A, mat, nvec, alpha, beta, ldx=None, ldy=None, offset=0, ref=None, what=""):
    """A.matmat_rm_f32 on nvec columns (NaN in every padding position of X and Y; beta == 0: all of Y starts as
    NaN): every column against the CSR product of the ROUNDED values and (alpha != 0) beyond the bound of the
    unrounded one; the positions j >= nvec stay NaN, X keeps its bits.  ref: a function (X, Y0, alpha, beta) -> Y1
    of shape (nvec, nrows) that every column must equal bit for bit."""
    torch = shared.torch
    csr, m, m32, csr32 = mat
    nr, nc = m.shape
    ldx = nvec if ldx is None else ldx
    ldy = nvec if ldy is None else ldy
    Xh = columns(shared, nc, nvec, X_SEED)
    y0h = columns(shared, nr, nvec, Y_SEED)
    xf, X = rm_block(torch, nc, nvec, ldx, offset)
    yf, Y = rm_block(torch, nr, nvec, ldy, offset)
    X.copy_(torch.from_numpy(np.ascontiguousarray(Xh.T)))
    if beta != 0.0:
        Y.copy_(torch.from_numpy(np.ascontiguousarray(y0h.T)))
    assert X.stride(0) == ldx and Y.stride(0) == ldy and X.data_ptr() % 16 == (8 * offset) % 16
    Y0 = Y.clone()
    x_bits = xf.view(torch.int64).clone()
    out = A.matmat_rm_f32(alpha, X, beta, Y)
    torch.cuda.synchronize()
    assert out is Y
    Yh = np.ascontiguousarray(Y.cpu().numpy().T)
    assert not np.isnan(Yh).any(), "a result is NaN"
    assert torch.isnan(outside(torch, yf, nr, nvec, ldy, offset)).all(), "the padding of Y was written"
    assert torch.equal(xf.view(torch.int64), x_bits), "X was written"
    for j in range(nvec):
        mc.check_y_rect(m32, csr32, Xh[j], Yh[j], alpha, beta, y0h[j] if beta != 0.0 else None)
        if alpha != 0.0:
            assert_reads_floats(mat, Xh[j], Yh[j], alpha, beta, y0h[j], "%s nvec %d column %d alpha %g beta %g" % (
                what, nvec, j, alpha, beta))
    if ref is not None:
        Y1 = ref(X, Y0, alpha, beta)
        torch.cuda.synchronize()
        assert torch.equal(Y.t(), Y1), "a column differs from the single float product"


# ---- 1. the 36 instances ---------------------------------------------------------------------------------------------

ALL_KERNELS = {(f, K, w) for f in mc.FAMILIES for K in (1, 2, 4, 8) for w in mc.KERNEL_WAVES}


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
        inf, g = A.info(), A.matmat_rm_group()
        assert g == mc.KERNEL_TUNES[(matrix, family)] == A.matmat_group_f32()
        ran_family = "accum" if inf.col_slices > 1 else "det" if inf.wave_tiles else "plain"
        ref = float_columns(torch, A) if ran_family == "det" else None
        ran = set()
        for k, nvec in enumerate(NVECS):
            alpha, beta = mc.ALPHA_BETA[k % 3]
            # (an odd leading dimension every other time: every other row 8 but not 16 bytes aligned)
            run_rm_f32(shared, A, mat, nvec, alpha, beta, ldx=nvec + (k % 2), ldy=nvec + 2 * (k % 2), ref=ref,
                       what="%s %s waves %d" % key)
            ran |= {(ran_family, K, int(inf.waves)) for K in groups_of(g, nvec)}
        shared.drop(("kernel",) + key)
        done[key] = ran
        return ran
    yield ensure
    done.clear()


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


# ---- 2. padding, alignment, windows --------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cant(shared):
    mat = shared.matrix("k-cant", mc.KERNEL_MATRICES["cant"])
    return shared.load(("cant",), mat[0], mat[1], dict(mc.NOSAMPLE, **ON)), mat


def test_padding_positions_stay_nan(shared, cant):
    """leading dimensions that differ between X and Y; beta == 0 over a Y of NaN and a Y that is read"""
    A, mat = cant
    assert A.matmat_rm_group() >= 2
    run_rm_f32(shared, A, mat, 5, 0.5, 0.0, ldx=12, ldy=14, what="cant")
    run_rm_f32(shared, A, mat, 8, 2.0, -0.5, ldx=9, ldy=9, what="cant")
    run_rm_f32(shared, A, mat, 8, 0.5, 0.0, ldx=8, ldy=16, what="cant")


@pytest.mark.parametrize("nvec", [2, 4, 8])
def test_base_eight_bytes_off_and_an_odd_ldx(shared, cant, nvec):
    """the 8-byte loads of X: the base 8 bytes off a 16-byte boundary with an even leading dimension (every row
    misaligned), and an odd leading dimension (every other row)"""
    A, mat = cant
    run_rm_f32(shared, A, mat, nvec, 2.0, -0.5, offset=1, what="cant at 8 mod 16")
    run_rm_f32(shared, A, mat, nvec, 0.5, 0.0, ldx=nvec + 2, ldy=nvec + 2, offset=1, what="cant at 8 mod 16, padded")
    run_rm_f32(shared, A, mat, nvec, 0.5, 0.0, ldx=nvec + 1, ldy=nvec + 3, what="cant, odd ldx")


@pytest.mark.parametrize("name", ["long-rows", "band-1500", "band-wide"])
def test_long_rows_and_band_windows(shared, name):
    """carry slots and the fix-up (long-rows); windows gathered through L2 at K = 8 and staged at narrower groups
    within one call, 13 = 8 + 4 + 1 (band-1500, and the rectangular band-wide)"""
    if name == "long-rows":
        mat = shared.matrix(name, lambda: (mc.long_rows(), None))
        opts = mc.NOSAMPLE
    else:
        mat = shared.matrix(name, lambda: mc.band(**mc.BANDS[name][0]))
        opts = mc.band_options("pinned")
    A = shared.load(("windows", name), mat[0], mat[1], dict(opts, **ON))
    assert A.matmat_rm_group() >= 2
    for k, nvec in enumerate((13, 7)):
        for alpha, beta in mc.ALPHA_BETA:
            run_rm_f32(shared, A, mat, nvec, alpha, beta, ldx=nvec + k, ldy=nvec + 3 - k, what=name)
    shared.drop(("windows", name))


# ---- 3. determinism -----------------------------------------------------------------------------------------------------------

def test_deterministic_columns_are_bit_identical(shared):
    """spx.gpu.deterministic=true: every column is matvec_f32 of that column, bit for bit"""
    torch = shared.torch
    mat = shared.matrix("k-cant", mc.KERNEL_MATRICES["cant"])
    A = shared.load(("det",), mat[0], mat[1], dict(mc.NOSAMPLE, **dict({"spx.gpu.deterministic": "true"}, **ON)))
    assert A.matmat_rm_group() >= 2
    ref = float_columns(torch, A)
    for nvec in (1, 3, 8):
        run_rm_f32(shared, A, mat, nvec, 0.5, 0.25, ldx=nvec + 3, ldy=nvec + 1, ref=ref, what="cant deterministic")
        run_rm_f32(shared, A, mat, nvec, 0.5, 0.0, ldx=nvec + 2, ldy=nvec + 2, ref=ref, what="cant deterministic")
    shared.drop(("det",))


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------------

def _assert_refused(torch, A, nvec=2):
    X = torch.ones((A.ncols, nvec), dtype=torch.float64, device="cuda")
    Y = torch.full((A.nrows, nvec), 7.0, dtype=torch.float64, device="cuda")
    with pytest.raises(sx.SpxError):
        A.matmat_rm_f32(1.0, X, 0.0, Y)
    with pytest.raises(sx.SpxError):
        A.hip_matmat_rm_kernel_f32(1.0, X.data_ptr(), nvec, 1, 0.5, Y.data_ptr(), nvec, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert bool((Y == 7.0).all()) and bool((X == 1.0).all()), "a refused call wrote"


def test_symmetric_handle_is_refused(shared):
    """with a float copy (spx.gpu.values_f32=all), so that the layout is what refuses it"""
    torch = shared.torch
    gen, opts = tt.SYM_CASES["no-once"]
    mat = shared.matrix("sym-kkt20", lambda: (gen(), None))
    A = shared.load(("sym",), mat[0], mat[1], dict(opts, **{"spx.gpu.values_f32": "all"}), sym=True)
    assert A.info().symmetric and A.values_f32_bytes() > 0 and A.matmat_rm_group() == 0
    _assert_refused(torch, A)
    shared.drop(("sym",))


def test_matrix_with_an_exchange_plan_is_refused(shared):
    """(a communicator of one rank, as in test_gpu_matmat_rm.py)"""
    torch = shared.torch
    mat = shared.matrix("k-cant", mc.KERNEL_MATRICES["cant"])
    t = sx.RcclTransport(sx.rccl_unique_id(), 0, 1)
    A = shared.load(("attached",), mat[0], mat[1], dict(mc.NOSAMPLE, **ON))
    assert A.matmat_rm_group() >= 2 and A.values_f32_bytes() > 0
    A.dist_attach(t)
    _assert_refused(torch, A)
    shared.drop(("attached",))
    t.destroy()


def test_handle_without_a_copy_is_refused(shared):
    torch = shared.torch
    mat = shared.matrix("k-cant", mc.KERNEL_MATRICES["cant"])
    A = shared.load(("no-copy",), mat[0], mat[1], dict(mc.NOSAMPLE))
    assert A.values_f32_bytes() == 0 and A.matmat_group_f32() == 0 and A.matmat_rm_group() >= 2
    _assert_refused(torch, A)
    shared.drop(("no-copy",))


def test_bad_leading_dimensions_fail(shared, cant):
    torch = shared.torch
    A, mat = cant
    n = mat[0][3]
    s = torch.cuda.current_stream().cuda_stream
    buf = torch.full((4 * n,), 7.0, dtype=torch.float64, device="cuda")
    base = buf.data_ptr()
    with pytest.raises(sx.SpxError):                      # ldx < nvec
        A.hip_matmat_rm_kernel_f32(1.0, base, 1, 2, 0.0, base + 16 * n, 2, s)
    with pytest.raises(sx.SpxError):                      # ldy < nvec
        A.hip_matmat_rm_kernel_f32(1.0, base, 2, 2, 0.0, base + 16 * n, 1, s)
    with pytest.raises(sx.SpxError):                      # X and Y overlap
        A.hip_matmat_rm_kernel_f32(1.0, base, 2, 2, 0.0, base + 8 * n, 2, s)
    with pytest.raises(sx.SpxError):                      # NULL X
        A.hip_matmat_rm_kernel_f32(1.0, 0, 2, 2, 0.0, base + 16 * n, 2, s)
    A.hip_matmat_rm_kernel_f32(1.0, base, 3, 0, 0.0, base, 3, s)           # nvec == 0: nothing happens
    torch.cuda.synchronize()
    assert bool((buf == 7.0).all()), "a refused call or a call with no vectors wrote"
    # (adjacent, not overlapping: fine)
    Xh = columns(shared, n, 2, X_SEED)
    buf[:2 * n].view(n, 2).copy_(torch.from_numpy(np.ascontiguousarray(Xh.T)))
    A.hip_matmat_rm_kernel_f32(1.0, base, 2, 2, 0.0, base + 16 * n, 2, s)
    torch.cuda.synchronize()
    Y = buf[2 * n:].view(n, 2)
    for j in range(2):
        check_y(mat[3], Xh[j], Y[:, j].cpu().numpy(), 1.0)
