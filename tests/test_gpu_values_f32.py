"""The product with the float copy of the values on the GPU: spx_hip_matvec_kernel_f32 / Matrix.matvec_f32 on handles
tuned with spx.gpu.values_f32=true (csx_narrow_values_kernel builds the copy; csx_spmv_f32_kernel,
csx_spmv_accum_f32_kernel, csx_spmv_det_f32_kernel and csx_spmv_xw_f32_kernel read it).

The reference of every result is helpers.check_y / matmat_cases.check_y_rect -- the project's fp64 bound and its
relative 1e-6 criterion -- on the CSR arrays with values.astype(float32).astype(float64): the product is an fp64
product of fl32(A).  That a kernel really reads the floats shows where the result lies BEYOND the fp64 bound of the
product with A itself: on at least half the non-empty rows of every matrix whose values are not floats already.
(tests/golden's demopatt holds 32 floats among its 38 values, 1.0 .. 10.0 and the like: there the CSR product of the
rounded values itself lies beyond A's bound on a few rows only, and the result must lie beyond it on at least half
of THOSE.)  Tuned handles, matrices and vectors are shared per module."""
import numpy as np
import pytest
import scipy.sparse as sp

import sparsex_amd as sx
from sparsex_amd import synth
from helpers import FP64_BOUND_FACTOR, check_y, tune
import dist_cases as dc
import limit_cases as lc
import matmat_cases as mc
import values_cases as vc
import test_gpu_transpose as tt

pytestmark = pytest.mark.gpu

PAD = 3
OPT = "spx.gpu.values_f32"
ON = {OPT: "true"}
CASES = tt.CASES
MATRIX_OF = tt.MATRIX_OF
U = 2.0 ** -53


def rounded(v):
    return np.asarray(v).astype(np.float32).astype(np.float64)


class Shared:
    """Matrices (with their float-rounded twins), tuned handles and vectors, made once and shared."""

    def __init__(self, torch):
        self.torch = torch
        self.mats, self.tuned, self.xs = {}, {}, {}

    def matrix(self, name, gen):
        """(csr tuple, scipy matrix, scipy matrix of the rounded values, its csr tuple)"""
        if name not in self.mats:
            csr, m = gen()
            if m is None:
                m = mc.to_scipy(csr)
            m = sp.csr_matrix(m)
            m32 = sp.csr_matrix((rounded(m.data), m.indices, m.indptr), shape=m.shape)
            self.mats[name] = (csr, m, m32, (m32.indptr, m32.indices, m32.data, m32.shape[0]))
        return self.mats[name]

    def load(self, key, csr, m, opts, sym=False):
        if key not in self.tuned:
            if m.shape[0] != m.shape[1]:
                self.tuned[key] = mc.load_rect(sx, csr, m.shape[1], opts)
            else:
                self.tuned[key] = tune(csr, opts, sym=sym)
        return self.tuned[key]

    def drop(self, key):
        self.tuned.pop(key).destroy()

    def case(self, name, more=None):
        gen, opts, _ = CASES[name]
        mat = self.matrix(MATRIX_OF.get(name, name), gen)
        o = dict(dict(opts, **ON), **(more or {}))
        return self.load((name, tuple(sorted((more or {}).items()))), mat[0], mat[1], o), mat

    def x(self, n, seed=5):
        if (n, seed) not in self.xs:
            xh = synth.random_x(n, seed=seed)
            xh.setflags(write=False)
            xf = self.torch.full((n + PAD + 2,), float("nan"), dtype=self.torch.float64, device="cuda")
            xf[2:2 + n] = self.torch.from_numpy(xh.copy())
            self.xs[(n, seed)] = (xh, xf)
        return self.xs[(n, seed)]


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


def beyond_rows(m, xh, yh, alpha, beta, y0h):
    """(rows on which yh lies beyond the fp64 bound of alpha * m * x + beta * y0, the non-empty rows)"""
    yc = alpha * (m @ xh)
    bound = abs(alpha) * FP64_BOUND_FACTOR * U * (abs(m) @ np.abs(xh)) + 1e-300
    if beta != 0.0:
        yc = yc + beta * y0h
        bound = bound + 4 * U * np.abs(beta * y0h)
    return np.abs(yh - yc) > bound, np.diff(m.indptr) > 0


def assert_reads_floats(mat, xh, yh, alpha, beta, y0h, what=""):
    """The result is the product of ANOTHER matrix than A: beyond A's fp64 bound on at least half the non-empty
    rows -- or, where A's values are mostly floats already (demopatt), on at least half the rows on which the CSR
    product of the rounded values lies beyond it."""
    csr, m, m32, csr32 = mat
    got, nonempty = beyond_rows(m, xh, yh, alpha, beta, y0h)
    y32 = alpha * (m32 @ xh) + (beta * y0h if beta != 0.0 else 0.0)
    ref, _ = beyond_rows(m, xh, y32, alpha, beta, y0h)
    n_ne, n_ref, n_got = int(nonempty.sum()), int((ref & nonempty).sum()), int((got & nonempty).sum())
    print("%s: beyond A's fp64 bound on %d of %d non-empty rows (the CSR product of the rounded values: %d)" % (
        what, n_got, n_ne, n_ref))
    assert n_ref > 0
    if 2 * n_ref >= n_ne:
        assert 2 * n_got >= n_ne, "the result is A's own product on most rows: were the doubles read?"
    else:
        assert 2 * int((got & ref & nonempty).sum()) >= n_ref


def f32_runs(shared, A, mat, pairs=mc.ALPHA_BETA, shift=2, what="", beyond=True):
    """A.matvec_f32 for every (alpha, beta) on vectors inside NaN-padded tensors (`shift`: where they start, in
    doubles: 2 = 16-byte aligned, 1 = not), beta == 0 over a y of NaN; each result against the CSR product of the
    rounded values, and (alpha != 0) beyond the bound of the unrounded one."""
    torch = shared.torch
    csr, m, m32, csr32 = mat
    nr, nc = m.shape
    xh, xf = shared.x(nc)
    if shift != 2:
        xf = torch.full((nc + PAD + 2,), float("nan"), dtype=torch.float64, device="cuda")
        xf[shift:shift + nc] = torch.from_numpy(xh.copy())
    xv = xf[shift:shift + nc]
    assert xv.data_ptr() % 16 == (0 if shift == 2 else 8)
    y0h = shared.x(nr, seed=9)[0]
    for alpha, beta in pairs:
        yf = torch.full((nr + PAD + 2,), float("nan"), dtype=torch.float64, device="cuda")
        yv = yf[shift:shift + nr]
        if beta != 0.0:
            yv.copy_(torch.from_numpy(y0h.copy()))
        out = A.matvec_f32(alpha, xv, beta, yv)
        torch.cuda.synchronize()
        assert out is yv
        yh = yv.cpu().numpy()
        assert torch.isnan(yf[:shift]).all() and torch.isnan(yf[shift + nr:]).all(), "the padding of y was written"
        assert torch.isnan(xf[:shift]).all() and torch.isnan(xf[shift + nc:]).all()
        assert torch.equal(xv.cpu(), torch.from_numpy(xh.copy())), "x was written"
        mc.check_y_rect(m32, csr32, xh, yh, alpha, beta, y0h if beta != 0.0 else None)
        if beyond and alpha != 0.0:
            assert_reads_floats(mat, xh, yh, alpha, beta, y0h, "%s alpha %g beta %g" % (what, alpha, beta))


def f64_product(shared, A, n_x, n_y, alpha=0.5):
    torch = shared.torch
    xh, xf = shared.x(n_x)
    y = torch.full((n_y,), float("nan"), dtype=torch.float64, device="cuda")
    A.hip_matvec_kernel(alpha, xf[2:2 + n_x].data_ptr(), 0.0, y.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return y


def stream_values(A):
    return A.info().value_bytes // 8


def assert_no_copy(shared, A, bytes_expected=0):
    """bytes as stated, and the three entry points fail without writing"""
    torch = shared.torch
    L = sx.lib()
    assert A.values_f32_bytes() == bytes_expected
    x = torch.zeros(A.ncols, dtype=torch.float64, device="cuda")
    y = torch.full((A.nrows,), 7.0, dtype=torch.float64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    assert L.spx_hip_matvec_kernel_f32(1.0, A.handle, x.data_ptr(), 0.0, y.data_ptr(), st) == sx.SPX_FAILURE
    assert L.spx_hip_matvec_mult_f32(1.0, A.handle, x.data_ptr(), y.data_ptr(), st) == sx.SPX_FAILURE
    with pytest.raises(sx.SpxError):
        sx.matvec_kernel_f32_vec(A, 1.0, sx.DeviceVector(A.ncols), 0.0, sx.DeviceVector(A.nrows))
    with pytest.raises(sx.SpxError):
        A.matvec_f32(1.0, x, 0.0, y)
    torch.cuda.synchronize()
    assert bool((y == 7.0).all()), "a refused call wrote"


# ---- 1. the result against the CSR product of the rounded values ---------------------------------------------------

@pytest.mark.parametrize("name", list(CASES))
def test_result_matches_csr_of_the_rounded_values(shared, name):
    A, mat = shared.case(name)
    inf = A.info()
    print("%s: %d row-blocks, waves %d, wave tiles %d, unit windows %d, column slices %d" % (
        name, inf.n_rowblocks, inf.waves, inf.wave_tiles, inf.unit_windows, inf.col_slices))
    assert not inf.symmetric
    assert A.values_f32_bytes() == 4 * stream_values(A) > 0
    f32_runs(shared, A, mat, what=name)


# ---- 2. every instance ---------------------------------------------------------------------------------------------

FAMILY_RUNS = [(mx, fam, w) for (mx, fam) in (("cant", "plain"), ("cant", "det"), ("cant", "accum"), ("band-twice", "accum"))
               for w in mc.KERNEL_WAVES]


@pytest.mark.parametrize("matrix,family,waves", FAMILY_RUNS)
def test_general_families_and_wavefront_counts(shared, matrix, family, waves):
    """csx_spmv_f32_kernel, csx_spmv_det_f32_kernel and csx_spmv_accum_f32_kernel for 2, 4 and 8 wavefronts"""
    assert (matrix, family) in mc.KERNEL_TUNES
    mat = shared.matrix("k-" + matrix, mc.KERNEL_MATRICES[matrix])
    key = ("family", matrix, family, waves)
    # (the plain family without the unit windows, which the launch tuner may otherwise turn on: they have a test of
    # their own below)
    A = shared.load(key, mat[0], mat[1], dict(dict(mc.kernel_options(family, waves), **ON), **{"spx.gpu.unit_windows": "false"}))
    inf = A.info()
    assert inf.waves == waves
    assert (inf.col_slices == 2) == (family == "accum")
    assert (inf.wave_tiles == 1) == (family == "det")
    assert inf.unit_windows == 0
    assert A.values_f32_bytes() == 4 * stream_values(A)
    f32_runs(shared, A, mat, what="%s %s waves %d" % (matrix, family, waves))
    shared.drop(key)


XW_RUNS = [(name, w) for name in ("cant", "nlpkkt") for w in (2, 4, 8)]
XW_OPTS = {"spx.gpu.unit_windows": "true", "spx.gpu.wave_tiles": "false", "spx.gpu.col_phases": "1"}


@pytest.mark.parametrize("name,waves", XW_RUNS)
def test_unit_window_family(shared, name, waves):
    """csx_spmv_xw_f32_kernel<2 | 4 | 8>"""
    A, mat = shared.case(name, dict(XW_OPTS, **{"spx.gpu.waves": str(waves)}))
    assert A.info().unit_windows == 1 and A.info().waves == waves
    f32_runs(shared, A, mat, what="%s unit windows, waves %d" % (name, waves))


@pytest.mark.parametrize("family", ["plain", "xw"])
def test_misaligned_pointers(shared, family):
    """x and y at addresses that are 8 but not 16 bytes aligned"""
    if family == "xw":
        A, mat = shared.case("cant", dict(XW_OPTS, **{"spx.gpu.waves": "4"}))
        assert A.info().unit_windows == 1
    else:
        A, mat = shared.case("cant", dict(lc.OFF_FAMILIES["plain"], **{"spx.gpu.waves": "4"}))
        assert A.info().unit_windows == 0 and A.info().wave_tiles == 0
    f32_runs(shared, A, mat, pairs=mc.ALPHA_BETA[:2], shift=1, what="cant " + family + " at 8 mod 16")


# ---- 3. the limits of the stream's fields (limit_cases.py) -----------------------------------------------------------

OFF_RUNS = [(c, f) for c in ("off-65536", "off-2p24") for f in ("plain", "unit-windows")]


@pytest.mark.parametrize("case,family", OFF_RUNS)
def test_offsets_of_24_and_32_bits(shared, case, family):
    assert case in lc.OFFSETS and min(lc.OFF_WIDTHS[(case, family)]) >= 3
    mat = shared.matrix(case, lambda: lc.wide_offsets(lc.OFFSETS[case][0]))
    key = (case, family)
    A = shared.load(key, mat[0], mat[1], dict(lc.off_options(family), **ON))
    # (spx.gpu.unit_windows=true turns the pipelined kernel on where a window plan exists: these matrices of
    # leftovers may leave it none, and the plain kernel then runs under both families)
    print("%s %s: unit windows %d" % (case, family, A.info().unit_windows))
    assert family == "unit-windows" or A.info().unit_windows == 0
    f32_runs(shared, A, mat, pairs=(lc.ALPHA_BETA, (0.5, 0.0)), what="%s %s" % (case, family))
    shared.drop(key)


LINEAR_F32_MODES = ("waves-2", "waves-4", "waves-8", "det-2", "det-4", "det-8", "unit-windows")


@pytest.mark.parametrize("mode", LINEAR_F32_MODES)
@pytest.mark.parametrize("case", list(lc.LINEAR))
def test_steps_segments_and_pass_counts(shared, case, mode):
    """steps of 127 and 128, 8188 segments in front, joined row-blocks (SpxPass::elem0), the pass counts at the
    edges of the wavefronts' turns (limit_cases.pass_edges)"""
    gen, _ = lc.LINEAR[case]
    mat = shared.matrix("diagonals" if case.startswith("segs") else case, gen)
    key = (case, mode)
    A = shared.load(key, mat[0], mat[1], dict(lc.linear_options(case, mode), **ON))
    assert not A.info().symmetric and A.values_f32_bytes() == 4 * stream_values(A)
    f32_runs(shared, A, mat, pairs=(lc.ALPHA_BETA, (0.5, 0.0)), what="%s %s" % (case, mode))
    shared.drop(key)


# ---- 4. same handle, both precisions ---------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["long-rows", "cant"])
def test_deterministic_products_are_bit_identical(shared, name):
    """spx.gpu.deterministic: the fp64 product of a handle with the copy is that of a handle without it, bit for
    bit, and two float products are bit-identical"""
    torch = shared.torch
    gen, opts, _ = CASES[name]
    mat = shared.matrix(name, gen)
    csr, m = mat[0], mat[1]
    n = csr[3]
    det = dict(opts, **{"spx.gpu.deterministic": "true", "spx.gpu.waves": "4"})
    A0 = shared.load((name, "det-off"), csr, m, det)
    y0 = f64_product(shared, A0, n, n)
    assert_no_copy(shared, A0)
    shared.drop((name, "det-off"))
    A1 = shared.load((name, "det-on"), csr, m, dict(det, **ON))
    assert A1.values_f32_bytes() == 4 * stream_values(A1)
    y1 = f64_product(shared, A1, n, n)
    xh, xf = shared.x(n)
    ys = []
    for _ in range(2):
        y = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
        A1.matvec_f32(0.5, xf[2:2 + n], 0.0, y)
        ys.append(y)
    y2 = f64_product(shared, A1, n, n)
    torch.cuda.synchronize()
    assert torch.equal(y0, y1) and torch.equal(y1, y2), "the fp64 product changed with the copy"
    assert torch.equal(ys[0], ys[1])
    check_y(csr, xh, y1.cpu().numpy(), 0.5)
    check_y(mat[3], xh, ys[0].cpu().numpy(), 0.5)
    assert_reads_floats(mat, xh, ys[0].cpu().numpy(), 0.5, 0.0, None, name + " deterministic")


@pytest.mark.parametrize("name", ["cant", "band-wide", "phases-c2"])
def test_other_products_still_read_the_doubles(shared, name):
    """the fp64, the multi-vector and the transposed product of a handle with the copy, against A"""
    torch = shared.torch
    A, mat = shared.case(name)
    csr, m, m32, csr32 = mat
    nr, nc = m.shape
    assert A.values_f32_bytes() > 0
    xh, _ = shared.x(nc)
    mc.check_y_rect(m, (m.indptr, m.indices, m.data, nr), xh, f64_product(shared, A, nc, nr).cpu().numpy(), 0.5, 0.0, None)
    mc.run(torch, A, m, 3, 2.0, -0.5, padx=PAD, pady=PAD)
    mt = m.T.tocsr()
    mt.sort_indices()
    zh, zf = shared.x(nr, seed=7)
    y = torch.full((nc,), float("nan"), dtype=torch.float64, device="cuda")
    A.matvec_trans(0.5, zf[2:2 + nr], 0.0, y)
    torch.cuda.synchronize()
    mc.check_y_rect(mt, (mt.indptr, mt.indices, mt.data, nc), zh, y.cpu().numpy(), 0.5, 0.0, None)


# ---- 5. keeping the copy true ------------------------------------------------------------------------------------------

UPDATE_RUNS = {
    "plain": dict(lc.OFF_FAMILIES["plain"], **{"spx.gpu.waves": "4"}),
    "phases-c2": dict(lc.OFF_FAMILIES["slices-c2"], **{"spx.gpu.waves": "4"}),
    "xw": dict(lc.OFF_FAMILIES["unit-windows"], **{"spx.gpu.waves": "4"}),
}


def _cant_small(shared):
    return shared.matrix("cant-small", lambda: (synth.syn_cant(0.02), None))


@pytest.mark.parametrize("family", list(UPDATE_RUNS))
def test_set_values_writes_both_arrays(shared, family):
    torch = shared.torch
    csr, m, m32, csr32 = _cant_small(shared)
    n = csr[3]
    A = vc.tune(csr, dict(UPDATE_RUNS[family], **ON))
    inf = A.info()
    assert inf.unit_windows == (1 if family == "xw" else 0) and inf.col_slices == (2 if family == "phases-c2" else 1)
    A.values_plan(csr[0], csr[1])
    xh, xf = shared.x(n)
    for seed in (1, 2):
        v = vc.new_values(csr, False, seed)
        A.set_values(torch.from_numpy(v.copy()).cuda())
        new = shared.matrix(("cant-small", seed), lambda: (vc.with_values(csr, v), None))
        f32_runs(shared, A, new, pairs=mc.ALPHA_BETA[:2], what="cant %s after set_values %d" % (family, seed))
        # ... and the doubles hold the new values unrounded
        check_y(new[0], xh, f64_product(shared, A, n, n).cpu().numpy(), 0.5)
    # the host variant, back to the values of the tune
    A.set_values(np.array(csr[2]))
    f32_runs(shared, A, (csr, m, m32, csr32), pairs=mc.ALPHA_BETA[:1], what="cant %s, the first values again" % family)
    A.destroy()


@pytest.mark.parametrize("family", ["plain", "xw"])
def test_set_entry_patches_the_float(shared, family):
    torch = shared.torch
    csr, m, m32, csr32 = _cant_small(shared)
    n = csr[3]
    A = vc.tune(csr, dict(UPDATE_RUNS[family], **ON))
    xh, xf = shared.x(n)
    y = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    A.matvec_f32(1.0, xf[2:2 + n], 0.0, y)                          # a product is in flight before the edit
    r = n // 2
    c = int(m.indices[m.indptr[r]])
    new_value = 1000.0 + 1.0 / 3.0                                  # (not a float)
    assert A.get_entry(r, c) == m[r, c]
    A.set_entry(r, c, new_value)
    assert A.get_entry(r, c) == new_value                            # the double
    m2 = m.copy()
    m2[r, c] = new_value
    m2 = sp.csr_matrix(m2)
    m2.sort_indices()
    new = shared.matrix(("cant-small", "entry"), lambda: ((m2.indptr, m2.indices, m2.data, n), m2))
    f32_runs(shared, A, new, pairs=mc.ALPHA_BETA[:2], what="cant %s after set_entry" % family)
    y.fill_(float("nan"))
    A.matvec_f32(1.0, xf[2:2 + n], 0.0, y)
    torch.cuda.synchronize()
    assert abs(y.cpu().numpy()[r] - (m32 @ xh)[r]) > 1.0            # (the old value would have passed nowhere near)
    check_y(new[0], xh, f64_product(shared, A, n, n).cpu().numpy(), 0.5)
    A.destroy()


def test_product_update_product_in_one_captured_graph(shared):
    torch = shared.torch
    csr, m, m32, csr32 = _cant_small(shared)
    n = csr[3]
    A = vc.tune(csr, dict(UPDATE_RUNS["plain"], **ON))
    A.values_plan(csr[0], csr[1])
    v = {seed: vc.new_values(csr, False, seed) for seed in (1, 2)}
    r32 = {seed: vc.with_values(csr, rounded(v[seed])) for seed in v}
    xh, xf = shared.x(n)
    x = xf[2:2 + n]
    src = torch.from_numpy(v[1].copy()).cuda()
    y1 = torch.zeros(n, dtype=torch.float64, device="cuda")
    y2 = torch.zeros(n, dtype=torch.float64, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    A.hip_matvec_kernel_f32(0.5, x.data_ptr(), 0.0, y1.data_ptr(), s)      # warm-up outside the capture
    A.hip_set_values(src.data_ptr(), s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = torch.cuda.current_stream().cuda_stream               # one stream, one chain
        A.hip_matvec_kernel_f32(0.5, x.data_ptr(), 0.0, y1.data_ptr(), cap)
        A.hip_set_values(src.data_ptr(), cap)
        A.hip_matvec_kernel_f32(0.5, x.data_ptr(), 0.0, y2.data_ptr(), cap)
    g.replay()
    torch.cuda.synchronize()
    check_y(r32[1], xh, y1.cpu().numpy(), 0.5)
    check_y(r32[1], xh, y2.cpu().numpy(), 0.5)
    src.copy_(torch.from_numpy(v[2].copy()).cuda())                 # a second value array where the graph reads it
    g.replay()
    torch.cuda.synchronize()
    check_y(r32[1], xh, y1.cpu().numpy(), 0.5)                      # (the first product still saw the first array)
    check_y(r32[2], xh, y2.cpu().numpy(), 0.5)
    assert np.abs(y2.cpu().numpy() - y1.cpu().numpy()).max() > 1e-3
    A.destroy()


# ---- 6. where there is no copy -------------------------------------------------------------------------------------------

def test_option_off_no_copy(shared):
    gen, opts, _ = CASES["cant"]
    mat = shared.matrix("cant", gen)
    for value in (None, "false"):
        key = ("cant", "off", value)
        A = shared.load(key, mat[0], mat[1], dict(opts, **({} if value is None else {OPT: value})))
        assert_no_copy(shared, A)
        shared.drop(key)


@pytest.mark.parametrize("name", ["tiles", "segments", "no-once"])
def test_symmetric_tunes_ignore_the_option(shared, name):
    gen, opts = tt.SYM_CASES[name]
    mat = shared.matrix("sym-" + name, lambda: (gen(), None))
    csr, m = mat[0], mat[1]
    key = ("sym", name)
    A = shared.load(key, csr, m, dict(opts, **ON), sym=True)
    assert A.info().symmetric
    assert_no_copy(shared, A)
    n = csr[3]
    check_y(csr, shared.x(n)[0], f64_product(shared, A, n, n).cpu().numpy(), 0.5)
    shared.drop(key)


def test_restore_reads_the_option_at_restore_time(shared, tmp_path):
    gen, opts, _ = CASES["cant"]
    mat = shared.matrix("cant", gen)
    files = {}
    for value in ("true", "false"):
        A = tune(mat[0], dict(opts, **{OPT: value}))
        files[value] = str(tmp_path / (value + ".spx"))
        A.save(files[value])
        A.destroy()
    assert open(files["true"], "rb").read() == open(files["false"], "rb").read()
    for saved in ("true", "false"):
        sx.options_reset()
        sx.option_set(OPT, "true")
        B = sx.mat_restore(files[saved])
        assert B.values_f32_bytes() == 4 * stream_values(B) > 0
        f32_runs(shared, B, mat, pairs=mc.ALPHA_BETA[:2], what="cant restored with the option on")
        n = mat[0][3]
        check_y(mat[0], shared.x(n)[0], f64_product(shared, B, n, n).cpu().numpy(), 0.5)
        B.destroy()
        sx.options_reset()
        B = sx.mat_restore(files[saved])
        assert_no_copy(shared, B)
        B.destroy()
    sx.options_reset()


def test_argument_failures(shared):
    torch = shared.torch
    A, (csr, m, m32, csr32) = shared.case("band-wide")
    nr, nc = m.shape
    L = sx.lib()
    st = torch.cuda.current_stream().cuda_stream
    buf = torch.zeros(nr + nc, dtype=torch.float64, device="cuda")
    x, y = buf[:nc], buf[nc:]
    assert L.spx_hip_matvec_kernel_f32(1.0, A.handle, x.data_ptr(), 0.0, y.data_ptr(), st) == sx.SPX_SUCCESS
    assert L.spx_hip_matvec_kernel_f32(1.0, None, x.data_ptr(), 0.0, y.data_ptr(), st) == sx.SPX_FAILURE
    assert L.spx_hip_matvec_kernel_f32(1.0, A.handle, None, 0.0, y.data_ptr(), st) == sx.SPX_FAILURE
    assert L.spx_hip_matvec_kernel_f32(1.0, A.handle, x.data_ptr(), 0.0, None, st) == sx.SPX_FAILURE
    assert L.spx_hip_matvec_mult_f32(1.0, A.handle, x.data_ptr(), None, st) == sx.SPX_FAILURE
    torch.cuda.synchronize()
    buf.fill_(1.0)
    for xp, yp in ((buf[:nc].data_ptr(), buf[nc - 1:].data_ptr()), (buf[nr - 1:].data_ptr(), buf[:nr].data_ptr()),
                   (buf.data_ptr(), buf.data_ptr())):
        assert L.spx_hip_matvec_kernel_f32(1.0, A.handle, xp, 0.0, yp, st) == sx.SPX_FAILURE
        with pytest.raises(sx.SpxError):
            A.hip_matvec_kernel_f32(1.0, xp, 0.0, yp, st)
    torch.cuda.synchronize()
    assert bool((buf == 1.0).all()), "a refused call wrote"
    good_x, good_y = sx.DeviceVector(nc), sx.DeviceVector(nr)
    sx.matvec_kernel_f32_vec(A, 1.0, good_x, 0.0, good_y)
    for bx, by in ((sx.DeviceVector(nr), sx.DeviceVector(nc)), (sx.DeviceVector(nc + 1), good_y),
                   (good_x, sx.DeviceVector(nr - 1))):
        with pytest.raises(sx.SpxError):
            sx.matvec_kernel_f32_vec(A, 1.0, bx, 0.0, by)
    torch.cuda.synchronize()


# ---- 7. a general row slice ------------------------------------------------------------------------------------------------

def test_row_slices_write_their_own_rows(shared):
    """Ranks 0 and 1 of 2 in one process: each writes only its rows, right against fl32(A)."""
    torch = shared.torch
    csr, m, m32, csr32 = shared.matrix("dist-nlpkkt", lambda: (dc.MATRICES["nlpkkt"](), None))
    n = csr[3]
    xh, xf = shared.x(n)
    y0h = shared.x(n, seed=9)[0]
    opts = dict(dc.NOSAMPLE, **dict({"spx.gpu.waves": dc.WAVES, "spx.gpu.wave_tiles": "false"}, **ON))
    covered = 0
    for rank in range(2):
        A = dc.tune_rank(csr, rank, 2, opts)
        inf = A.info()
        lo, hi = inf.row_lo, inf.row_hi
        assert not inf.symmetric and 0 <= lo < hi <= n and hi - lo < n
        assert A.values_f32_bytes() == 4 * stream_values(A) > 0
        part = dc.general_part(m, lo, hi)
        part32 = dc.general_part(m32, lo, hi)
        for alpha, beta in mc.ALPHA_BETA:
            y = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
            if beta != 0.0:
                y[lo:hi] = torch.from_numpy(y0h[lo:hi].copy())
            A.matvec_f32(alpha, xf[2:2 + n], beta, y)
            torch.cuda.synchronize()
            yh = y.cpu().numpy()
            assert np.isnan(yh[:lo]).all() and np.isnan(yh[hi:]).all(), "a slice wrote rows of another rank"
            own = np.zeros(n)
            own[lo:hi] = yh[lo:hi]
            y0 = np.zeros(n)
            y0[lo:hi] = y0h[lo:hi]
            check_y((part32.indptr, part32.indices, part32.data, n), xh, own, alpha, beta, y0 if beta != 0.0 else None)
            if alpha != 0.0:
                assert_reads_floats((None, sp.csr_matrix(part), sp.csr_matrix(part32), None), xh, own, alpha, beta, y0,
                                    "rank %d alpha %g" % (rank, alpha))
        covered += hi - lo
        A.destroy()
    assert covered == n


# ---- 8. iterative refinement ---------------------------------------------------------------------------------------------------

REFINE_OUTER, REFINE_SWEEPS = 12, 3
# The computed residual of the converged iterate lies within one fp64 bound of the true one, and the last update
# of x (one rounding per element, |dx| <= 2^-53 |x|) moves A x by less than another: twice the bound of A x.
REFINE_FACTOR = 2.0


def test_refinement_reaches_fp64_with_fp64_residuals_only(shared):
    """band-400 plus a diagonal that makes it strictly diagonally dominant.  Iterative refinement whose correction
    is REFINE_SWEEPS Jacobi sweeps with the float product: with the residual b - A x from the fp64 product of the
    SAME handle it reaches the fp64 level; with the float product for the residual as well it stalls far above."""
    torch = shared.torch
    (rp, ci, va, n), band = mc.band(**mc.BANDS["band-400"][0])
    rng = np.random.RandomState(41)
    off = band - sp.diags(band.diagonal())
    d = 1.5 * np.asarray(abs(off).sum(axis=1)).ravel() + rng.uniform(1.0, 2.0, n)
    m = sp.csr_matrix(off + sp.diags(d))
    m.sort_indices()
    csr = (m.indptr.astype(np.int32), m.indices.astype(np.int32), m.data.copy(), n)
    A = tune(csr, dict(mc.band_options("pinned"), **ON))
    assert A.values_f32_bytes() == 4 * stream_values(A)
    bh = synth.random_x(n, seed=43)
    b = torch.from_numpy(bh.copy()).cuda()
    dinv = torch.from_numpy(1.0 / m.diagonal()).cuda()
    st = torch.cuda.current_stream().cuda_stream

    def refine(residual_f32):
        x = torch.zeros(n, dtype=torch.float64, device="cuda")
        for _ in range(REFINE_OUTER):
            r = b.clone()
            if residual_f32:
                A.matvec_f32(-1.0, x, 1.0, r)
            else:
                A.hip_matvec_kernel(-1.0, x.data_ptr(), 1.0, r.data_ptr(), st)
            dx = dinv * r
            for _ in range(REFINE_SWEEPS):
                t = r.clone()
                A.matvec_f32(-1.0, dx, 1.0, t)
                dx = dx + dinv * t
            x = x + dx
        torch.cuda.synchronize()
        xh = x.cpu().numpy()
        ld = np.longdouble
        # the true residual, in extended precision, over the fp64 bound of A x
        ax = np.zeros(n, dtype=ld)
        rows = np.repeat(np.arange(n), np.diff(m.indptr))
        np.add.at(ax, rows, m.data.astype(ld) * xh[m.indices].astype(ld))
        res = np.abs(bh.astype(ld) - ax).astype(np.float64)
        bound = FP64_BOUND_FACTOR * U * (abs(m) @ np.abs(xh))
        return res / bound

    good = refine(False)
    stalled = refine(True)
    print("refinement: residual over the fp64 bound of A x, max %.3g with fp64 residuals, median %.3g / max %.3g with float ones" % (
        good.max(), np.median(stalled), stalled.max()))
    assert good.max() <= REFINE_FACTOR
    assert np.median(stalled) > 100.0 * REFINE_FACTOR
    A.destroy()
