"""Row / column norms and in-place diagonal scaling of a tuned matrix in HBM (spx_hip_mat_norms, spx_hip_mat_scale:
csx_norms_kernel and csx_scale_values_kernel of scale_kernels.hip): the norms against numpy over the untuned CSR
arrays (the max kind bit for bit, the sums within n * 2^-52), the scaled values bit for bit in every stored copy of
the stream, the products, the diagonal and the float copy of the values after a scaling, the walker at the limits of
the stream's fields, a captured graph, and the calls that must fail."""
import numpy as np
import pytest

import sparsex_amd as sx
from sparsex_amd.api import SpxError

import limit_cases as lc
import matmat_cases as mc
import scale_cases as sc
import values_cases as vc
from diag_cases import bits, matrix

pytestmark = pytest.mark.gpu

W4 = {"spx.gpu.waves": "4"}
# the general cases of test_gpu_diag.py: name -> (matrix, options, reorder)
CASES = {
    "default": ("cant", {}, False),
    "deterministic": ("cant", {"spx.gpu.deterministic": "true"}, False),
    "slices-c2": ("cant", {"spx.gpu.col_phases": "c2"}, False),
    "unit-windows": ("cant", {"spx.gpu.unit_windows": "true"}, False),
    "values-f32": ("cant", {"spx.gpu.values_f32": "true"}, False),
    "nlpkkt": ("nlpkkt", {}, False),
    "webbase": ("webbase", {}, False),
    "rect": ("rect", {}, False),
    "rect-t": ("rect-t", {}, False),
    "reorder": ("cant", {}, True),
}
SLICES = ("rank", "row-offset")
PERIOD = 65537             # of the scale vectors of the matrices with 2^24 columns and more


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.float64)).cuda()


def sentinels(n):
    return sx.DeviceVector(host=np.full(n, sc.SENTINEL))


def load(name):
    if name in SLICES:
        t = sc.tune_slice(name, W4)
    else:
        mat, opts, reorder = CASES[name]
        t = sc.tune_matrix(mat, dict(W4, **opts), reorder)
    assert t.A.info().on_device
    t.name = name
    return t


@pytest.fixture(params=list(CASES) + list(SLICES))
def tuned(request):
    t = load(request.param)
    yield t
    t.A.destroy()
    sx.options_reset()


# ---- norms -------------------------------------------------------------------------------------------------------

def norms_by(t, how):
    """kind -> (rows, cols) on the host, read in one of four ways into vectors of sentinels"""
    import torch
    A, nr, nc = t.A, t.nrows, t.ncols

    def norms_of(kind):
        if how == "both":
            r, c = A.norms(kind, sentinels(nr), sentinels(nc))
            return r.download(), c.download()
        if how == "rows":
            r, c = A.norms(kind, rows=sentinels(nr))
            assert c is None
            return r.download(), None
        if how == "cols":
            r, c = A.norms(kind, cols=dev(np.full(nc, sc.SENTINEL)))          # (a torch tensor: the current stream)
            assert r is None and isinstance(c, torch.Tensor)
            torch.cuda.synchronize()
            return None, c.cpu().numpy()
        # pointers 8 bytes into longer vectors, whose neighbours survive
        lr, lcv = sentinels(nr + 3), sentinels(nc + 3)
        A.hip_mat_norms(kind, lr.data_ptr() + 8, lcv.data_ptr() + 8)
        gr, gc = lr.download(), lcv.download()
        for g, n in ((gr, nr), (gc, nc)):
            assert g[0] == sc.SENTINEL and g[n + 1] == sc.SENTINEL and g[n + 2] == sc.SENTINEL
        return gr[1:nr + 1], gc[1:nc + 1]
    return norms_of


def test_norms_against_numpy(tuned):
    t = tuned
    if t.name == "slices-c2":
        assert t.A.info().col_slices == 2
    for how in ("both", "rows", "cols", "offset"):
        t.check_norms(norms_by(t, how), t.csr[2])
    r, c = t.A.norms(sx.NORM_SUM_ABS, rows=True, cols=True)                   # vectors made on request
    assert isinstance(r, sx.DeviceVector) and r.size == t.nrows and isinstance(c, sx.DeviceVector) and c.size == t.ncols
    want = sc.expected_norms(t.csr, sx.NORM_SUM_ABS, t.nrows, t.ncols, t.lo, t.hi, t.perm, t.row0)
    sc.check_norms(sx.NORM_SUM_ABS, c.download(), want[1], want[3], "cols of a new vector")
    # the host form of a matrix in HBM
    rows, cols = np.full(t.nrows, sc.SENTINEL), np.full(t.ncols, sc.SENTINEL)
    t.A.norms_host(sx.NORM_MAX_ABS, rows, cols)
    want = sc.expected_norms(t.csr, sx.NORM_MAX_ABS, t.nrows, t.ncols, t.lo, t.hi, t.perm, t.row0)
    sc.check_norms(sx.NORM_MAX_ABS, rows, want[0], want[2], "host form, rows")
    sc.check_norms(sx.NORM_MAX_ABS, cols, want[1], want[3], "host form, cols")


# ---- scaling -----------------------------------------------------------------------------------------------------

def products_and_diagonal(t, values):
    """the forward and the transposed product and the diagonal of the handle against the matrix with these CSR values"""
    import torch
    A = t.A
    m, csr, mt, csr_t = sc.tuned_matrix(t, values)
    x = np.random.RandomState(5).uniform(-1, 1, t.ncols)
    y = dev(np.zeros(t.nrows))
    A.hip_matvec_kernel(1.0, dev(x).data_ptr(), 0.0, y.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    yh = y.cpu().numpy()
    yh[:t.lo] = 0.0
    yh[t.hi:] = 0.0
    mc.check_y_rect(m, csr, x, yh, 1.0, 0.0, None)                         # helpers.check_y
    z = np.random.RandomState(6).uniform(-1, 1, t.nrows)
    w = dev(np.full(t.ncols, np.nan))
    A.matvec_trans(1.0, dev(z), 0.0, w)
    torch.cuda.synchronize()
    mc.check_y_rect(mt, csr_t, z, w.cpu().numpy(), 1.0, 0.0, None)         # (the bound of test_gpu_transpose.py)
    d = A.get_diag(sentinels(t.nrows)).download()
    want = np.zeros(t.nrows)
    k = min(t.nrows, t.ncols)
    want[:k] = m.diagonal()
    assert np.array_equal(bits(d[t.lo:t.hi]), bits(want[t.lo:t.hi]))
    assert (d[:t.lo] == sc.SENTINEL).all() and (d[t.hi:] == sc.SENTINEL).all()


def test_scaled_values_products_and_diagonal(tuned, tmp_path):
    t = tuned
    A = t.A
    A.values_plan(t.csr[0], t.csr[1])
    A.diag_plan()
    plan = A.values_plan_info()["src_values"]
    before = vc.decoded(A, tmp_path, "before.spx")
    dr, dcv = sc.vector(t.nrows, 1), sc.vector(t.ncols, 2)
    A.scale(sx.DeviceVector(host=dr), dev(dcv))                              # a device vector and a tensor
    v1 = t.scaled(t.csr[2], dr, dcv)
    after = vc.check_stream(A, t.scipy(v1), tmp_path, perm=t.perm)
    sc.untouched_positions(before, after, plan)
    products_and_diagonal(t, v1)
    t.check_norms(norms_by(t, "both"), v1)
    with pytest.raises(SpxError):
        A.export_csx(A.info().first_partition)                               # stale, as after set_values
    # each vector alone, through the raw pointers and through the host form
    drd = sx.DeviceVector(host=dr)
    A.hip_mat_scale(drd.data_ptr(), None)
    v2 = t.scaled(v1, dr, None)
    vc.check_stream(A, t.scipy(v2), tmp_path, perm=t.perm)
    A.scale(dc=dcv)                                                          # numpy: temporary buffers, synchronous
    v3 = t.scaled(v2, None, dcv)
    after3 = vc.check_stream(A, t.scipy(v3), tmp_path, perm=t.perm)
    sc.untouched_positions(before, after3, plan)
    assert vc.check_entries(A, t.scipy(v3), rows=(t.lo, t.hi) if t.name in SLICES else None, limit=60) > 0
    # a refresh overwrites with what the caller hands over
    A.set_values(dev(t.csr[2]))
    back = vc.check_stream(A, t.scipy(t.csr[2]), tmp_path, perm=t.perm)
    assert np.array_equal(bits(back.values), bits(before.values))
    products_and_diagonal(t, t.csr[2])


def test_float_copy_follows_the_scaling():
    """The twin after a scaling holds what the refresh kernel narrows from the same doubles: the float product (and
    the fp64 one) of the two states agree bit for bit.  (spx.gpu.deterministic on top of the values-f32 case: only a
    product that repeats its own bits can show that two value arrays are the same.)"""
    import torch
    mat, opts, reorder = CASES["values-f32"]
    t = sc.tune_matrix(mat, dict(W4, **dict(opts, **{"spx.gpu.deterministic": "true"})), reorder)
    A = t.A
    assert A.values_f32_bytes() > 0
    A.values_plan(t.csr[0], t.csr[1])
    dr, dcv = sc.vector(t.nrows, 1), sc.vector(t.ncols, 2)
    x = dev(np.random.RandomState(5).uniform(-1, 1, t.ncols))
    s = torch.cuda.current_stream().cuda_stream

    def both_products():
        y32, y64 = dev(np.zeros(t.nrows)), dev(np.zeros(t.nrows))
        A.matvec_f32(1.0, x, 0.0, y32)
        A.hip_matvec_kernel(1.0, x.data_ptr(), 0.0, y64.data_ptr(), s)
        torch.cuda.synchronize()
        return y32.cpu().numpy(), y64.cpu().numpy()

    y0 = both_products()
    A.scale(dev(dr), dev(dcv))
    y1 = both_products()
    assert not np.array_equal(bits(y0[0]), bits(y1[0]))
    v1 = t.scaled(t.csr[2], dr, dcv)
    A.set_values(dev(v1))
    y2 = both_products()
    assert np.array_equal(bits(y1[0]), bits(y2[0])), "the float copy after a scaling is not the narrowed doubles"
    assert np.array_equal(bits(y1[1]), bits(y2[1]))
    # and it is the FLOAT values the float product reads
    m32 = sc.tuned_matrix(t, v1.astype(np.float32).astype(np.float64))
    mc.check_y_rect(m32[0], m32[1], x.cpu().numpy(), y1[0], 1.0, 0.0, None)
    A.destroy()
    sx.options_reset()


def test_row_maxima_become_one():
    """dr = 1 / rowmax by the existing reciprocal: every non-empty row's largest |a| is then within 2^-52 of 1 (one
    rounding of the reciprocal, one of the product)."""
    t = load("webbase")
    A = t.A
    rmax, _ = A.norms(sx.NORM_MAX_ABS, rows=True)
    dr = sx.DeviceVector(t.nrows)
    rmax.reciprocal_into(dr, 0.0)
    A.scale(dr=dr)
    after = A.norms(sx.NORM_MAX_ABS, rows=True)[0].download()
    nonempty = rmax.download() > 0
    assert nonempty.sum() > 100 and (~nonempty).sum() == (np.diff(t.csr[0]) == 0).sum()
    assert (np.abs(after[nonempty] - 1.0) <= 2.0 ** -52).all()
    assert not after[~nonempty].any()
    A.destroy()
    sx.options_reset()


# ---- the walker at the limits of the stream's fields (limit_cases.py) -------------------------------------------------

def scale_and_max(csr, m, opts, tmp_path):
    """one scaling with check_stream and one norms(MAX_ABS) of the scaled matrix"""
    ncols = m.shape[1]
    A = vc.tune(csr, opts, ncols=ncols)
    t = sc.Tuned(A, csr, ncols)
    dr, dcv = sc.vector(t.nrows, 1, PERIOD), sc.vector(ncols, 2, PERIOD)
    A.scale(sx.DeviceVector(host=dr), sx.DeviceVector(host=dcv))
    v1 = t.scaled(csr[2], dr, dcv)
    vc.check_stream(A, t.scipy(v1), tmp_path)
    want = sc.expected_norms(vc.with_values(csr, v1), sx.NORM_MAX_ABS, t.nrows, ncols, 0, t.nrows)
    r, c = A.norms(sx.NORM_MAX_ABS, sentinels(t.nrows), sentinels(ncols))
    sc.check_norms(sx.NORM_MAX_ABS, r.download(), want[0], want[2], "rows")
    sc.check_norms(sx.NORM_MAX_ABS, c.download(), want[1], want[3], "cols")
    A.destroy()
    sx.options_reset()


_wide = {}


@pytest.mark.parametrize("case,family", sorted(lc.OFF_WIDTHS))
def test_column_offsets_of_16_24_and_32_bits(case, family, tmp_path):
    if case not in _wide:
        _wide.clear()                                   # (one matrix at a time: the widest has 2^25 columns)
        _wide[case] = lc.wide_offsets(lc.OFFSETS[case][0])
    csr, m = _wide[case]
    scale_and_max(csr, m, lc.off_options(family), tmp_path)


@pytest.mark.parametrize("case", [k for k, v in lc.STEPS.items() if not v[2]])
def test_steps_of_127(case, tmp_path):
    gen, opts, sym, _ = lc.STEPS[case]
    csr, m = gen()
    scale_and_max(csr, m, dict(opts, **W4), tmp_path)


@pytest.mark.parametrize("waves", lc.PASS_WAVES)
def test_pass_counts_at_the_edges_of_the_wavefronts_turns(waves, tmp_path):
    csr, m = lc.pass_edges()
    scale_and_max(csr, m, dict(lc.PASS_OPTS, **{"spx.gpu.waves": str(waves)}), tmp_path)


# ---- a captured graph ----------------------------------------------------------------------------------------------

def test_one_ruiz_sweep_in_a_captured_graph(tmp_path):
    """norms(MAX_ABS, rows) -> rsqrt -> scale(dr) -> product as one linear chain on one stream: a replay equals the
    eager sequence on a second, identically tuned handle bit for bit (deterministic tunes: the product repeats its
    own bits).  Every call ran once before the capture; that first sweep scaled both handles alike."""
    import torch
    opts = dict(W4, **{"spx.gpu.deterministic": "true"})
    ta, tb = sc.tune_matrix("nlpkkt", opts), sc.tune_matrix("nlpkkt", opts)
    n = ta.nrows
    x = dev(np.random.RandomState(5).uniform(-1, 1, n))
    out = []
    for t in (ta, tb):
        t.rows, t.dr, t.y = sentinels(n), sentinels(n), dev(np.zeros(n))

    def sweep(t, s):
        t.A.norms(sx.NORM_MAX_ABS, rows=t.rows, stream=s)
        t.rows.rsqrt(t.dr, 0.0, stream=s)
        t.A.scale(dr=t.dr, stream=s)
        t.A.hip_matvec_kernel(1.0, x.data_ptr(), 0.0, t.y.data_ptr(), s)

    s = torch.cuda.current_stream().cuda_stream
    sweep(ta, s)                                          # warm-up outside the capture
    sweep(tb, s)
    torch.cuda.synchronize()
    first = ta.y.cpu().numpy()
    assert np.array_equal(bits(first), bits(tb.y.cpu().numpy()))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        sweep(ta, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(bits(ta.y.cpu().numpy()), bits(first))             # (the capture ran nothing)
    g.replay()
    sweep(tb, s)
    torch.cuda.synchronize()
    ya, yb = ta.y.cpu().numpy(), tb.y.cpu().numpy()
    assert not np.array_equal(bits(ya), bits(first))
    assert np.array_equal(bits(ya), bits(yb))
    assert np.array_equal(bits(ta.dr.download()), bits(tb.dr.download()))
    sa, sb = vc.decoded(ta.A, tmp_path, "a.spx"), vc.decoded(tb.A, tmp_path, "b.spx")
    assert np.array_equal(bits(sa.values), bits(sb.values))
    # ... and it is the sweep: two of them by numpy
    v = ta.csr[2]
    for _ in range(2):
        rmax = sc.expected_norms(vc.with_values(ta.csr, v), sx.NORM_MAX_ABS, n, n, 0, n)[0]
        v = ta.scaled(v, 1.0 / np.sqrt(rmax), None)
    vc.check_stream(ta.A, ta.scipy(v), tmp_path)
    for t in (ta, tb):
        t.A.destroy()
    sx.options_reset()


# ---- calls that must fail ------------------------------------------------------------------------------------------

def test_calls_that_must_fail(tmp_path, capfd):
    import torch
    csr = matrix("nlpkkt")
    n = csr[3]
    rows, cols, dr = sentinels(n), sentinels(n), sx.DeviceVector(host=sc.vector(n, 1))

    def refused(A, what):
        capfd.readouterr()
        before = vc.decoded(A, tmp_path, "r0.spx")
        for call in (lambda: A.norms(sx.NORM_MAX_ABS, rows, cols), lambda: A.hip_mat_norms(sx.NORM_SUM_SQ, rows.data_ptr(), None),
                     lambda: A.scale(dr, dr), lambda: A.hip_mat_scale(None, dr.data_ptr())):
            with pytest.raises(SpxError):
                call()
        assert what in capfd.readouterr().err
        torch.cuda.synchronize()
        assert (rows.download() == sc.SENTINEL).all() and (cols.download() == sc.SENTINEL).all()
        after = vc.decoded(A, tmp_path, "r1.spx")
        assert np.array_equal(bits(after.values), bits(before.values)) and np.array_equal(bits(after.dvalues), bits(before.dvalues))

    # a symmetric tune (the host forms too)
    S = vc.tune(csr, W4, sym=True)
    refused(S, "symmetric")
    with pytest.raises(SpxError):
        S.norms_host(sx.NORM_MAX_ABS)
    with pytest.raises(SpxError):
        S.scale(np.ones(n), None)
    S.destroy()
    # a matrix with an exchange plan attached (a communicator of one rank)
    tr = sx.RcclTransport(sx.rccl_unique_id(), 0, 1)
    D = vc.tune(csr, W4)
    D.dist_attach(tr)
    refused(D, "exchange plan")
    D.destroy()
    tr.destroy()
    # the device forms on a host-only matrix; the arguments of a good handle
    H = vc.tune(csr, W4, host_only=True)
    refused(H, "host_only")
    H.destroy()
    A = vc.tune(csr, W4)
    L = sx.lib()
    assert L.spx_hip_mat_norms(A.handle, 3, rows.data_ptr(), cols.data_ptr(), None) == sx.SPX_FAILURE
    assert L.spx_hip_mat_norms(A.handle, 0, None, None, None) == sx.SPX_FAILURE
    assert L.spx_hip_mat_scale(A.handle, None, None, None) == sx.SPX_FAILURE
    assert L.spx_hip_mat_norms(None, 0, rows.data_ptr(), None, None) == sx.SPX_FAILURE
    assert L.spx_hip_mat_scale(None, dr.data_ptr(), None, None) == sx.SPX_FAILURE
    torch.cuda.synchronize()
    assert (rows.download() == sc.SENTINEL).all() and (cols.download() == sc.SENTINEL).all()
    A.export_csx(A.info().first_partition)                 # nothing went stale
    A.destroy()
    capfd.readouterr()
    sx.options_reset()


def test_wrong_current_device_is_refused():
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("one HIP device")
    csr = matrix("nlpkkt")
    n = csr[3]
    torch.cuda.set_device(0)
    A = vc.tune(csr, W4)
    rows, dr = sentinels(n), sx.DeviceVector(host=sc.vector(n, 1))
    try:
        torch.cuda.set_device(1)
        with pytest.raises(SpxError):
            A.hip_mat_norms(sx.NORM_MAX_ABS, rows.data_ptr(), None)
        with pytest.raises(SpxError):
            A.hip_mat_scale(dr.data_ptr(), None)
        with pytest.raises(SpxError):
            A.norms_host(sx.NORM_MAX_ABS)
    finally:
        torch.cuda.set_device(0)
    assert (rows.download() == sc.SENTINEL).all()
    A.destroy()
    sx.options_reset()
