"""The float product on symmetric handles: spx_hip_matvec_kernel_f32 / Matrix.matvec_f32 on matrices tuned as
symmetric ones with spx.gpu.values_f32=all -- the float instances of csx_spmv_symtile_kernel (+ csx_symfix_kernel),
csx_spmv_symtile_atomic_kernel, csx_spmv_symseg_kernel, csx_spmv_symseg_notile_kernel, csx_spmv_symtile_det_kernel
and csx_spmv_sx_kernel, and the general float kernels on a stream that stores the mirror image, with the float forms
of csx_sym_init_kernel, csx_sym_mirror_rows_kernel and csx_fixup_kernel around them.

The reference is the one of test_gpu_values_f32.py: helpers.check_y -- the project's fp64 bound and its relative
1e-6 criterion -- on the CSR arrays with values.astype(float32).astype(float64), DIAGONAL INCLUDED: the product is
the fp64 product of the matrix whose every stored entry is rounded to float.  On the matrices used here
(syn_nlpkkt, syn_nd24k, syn_cant, syn_kkt2f with synth.random_x) that rounded product lies beyond A's own fp64 bound
on every row, so assert_reads_floats' "at least half the non-empty rows" holds for the reference alone; and a product
that rounds everything but the diagonal lies beyond the bound of the rounded product on every row, so a diagonal
left unrounded anywhere cannot pass check_y.  Handles, matrices and vectors are shared per module."""
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
import test_gpu_sym_pipeline as tsp
import test_gpu_transpose as tt
import test_gpu_values_f32 as tf
from test_gpu_values_f32 import Shared, assert_reads_floats, f32_runs, rounded

pytestmark = pytest.mark.gpu

OPT = tf.OPT
ALL = {OPT: "all"}
NOSAMPLE = mc.NOSAMPLE
U = 2.0 ** -53

# name -> (matrix name, generator, options of the tune without the float option)
SYM = {
    # csx_spmv_sx_kernel: runs of 42 segments fill passes of their own
    "sx": ("kkt44", lambda: synth.syn_nlpkkt(44), dict(tsp.ON)),
    # csx_spmv_symseg_notile_kernel: runs too short for a pass of their own ...
    "notile-30": ("kkt30", lambda: synth.syn_nlpkkt(30), dict(tsp.ON)),
    # ... or the pipeline switched off
    "notile-44": ("kkt44", lambda: synth.syn_nlpkkt(44), dict(tsp.ON, **{"spx.gpu.sym_pipeline": "false"})),
    "atomic": ("nd24k", lambda: synth.syn_nd24k(0.05), dict(NOSAMPLE, **{"spx.gpu.sym_spill": "atomic"})),
    "lists": ("nd24k", lambda: synth.syn_nd24k(0.05), dict(NOSAMPLE, **{"spx.gpu.sym_spill": "lists"})),
    # csx_spmv_symseg_kernel: dense tiles and read-once segments in one stream
    "tiles+segments": ("nd24k", lambda: synth.syn_nd24k(0.05), dict(NOSAMPLE, **{"spx.gpu.sym_segments": "true"})),
    "det-nd24k": ("nd24k", lambda: synth.syn_nd24k(0.05), dict(NOSAMPLE, **{"spx.gpu.deterministic": "true"})),
    "det-kkt20": ("kkt20", lambda: synth.syn_nlpkkt(20), dict(NOSAMPLE, **{"spx.gpu.deterministic": "true"})),
    "no-once": ("kkt20", lambda: synth.syn_nlpkkt(20), dict(tt.SYM_CASES["no-once"][1])),
}


def landed(name, inf, sx_passes):
    """the kernel family the handle runs, through info()"""
    assert inf.symmetric and inf.on_device
    if name == "sx":
        return inf.sym_pipeline == 1 and inf.sym_segments == 2
    if name in ("notile-30", "notile-44"):
        return inf.sym_segments == 2 and (inf.sym_pipeline == 0 or sx_passes == 0)
    if name == "atomic":
        return inf.sym_tiles == 2 and inf.sym_segments == 0 and inf.wave_tiles == 0
    if name == "lists":
        return inf.sym_tiles == 1 and inf.sym_segments == 0 and inf.wave_tiles == 0
    if name == "tiles+segments":
        return inf.sym_segments == 1 and inf.sym_tiles == 2
    if name == "det-nd24k":
        return inf.wave_tiles == 1 and inf.sym_tiles == 1
    if name == "det-kkt20":
        return inf.wave_tiles == 1
    if name == "no-once":
        return inf.sym_tiles == 0 and inf.sym_segments == 0 and inf.wave_tiles == 0
    raise KeyError(name)


def sym_case(shared, name, more=None, option=ALL):
    mname, gen, opts = SYM[name]
    mat = shared.matrix("sym-" + mname, lambda: (gen(), None))
    o = dict(dict(opts, **option), **(more or {}))
    key = ("sym", name, tuple(sorted((more or {}).items())), tuple(sorted(option.items())))
    return shared.load(key, mat[0], mat[1], o, sym=True), mat, key


def has_copy(A):
    return A.values_f32_bytes() == 4 * (A.info().value_bytes // 8) > 0


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


# ---- 1. one case per kernel family -------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(SYM))
def test_every_family_against_the_rounded_csr_product(shared, name):
    A, mat, _ = sym_case(shared, name)
    inf = A.info()
    _, _, cnt = A.sym_pipeline()
    print("%s: %d row-blocks, waves %d, sym_tiles %d, sym_segments %d, sym_pipeline %d (%d SX passes), wave tiles %d" % (
        name, inf.n_rowblocks, inf.waves, inf.sym_tiles, inf.sym_segments, inf.sym_pipeline, cnt["sx_passes"], inf.wave_tiles))
    assert landed(name, inf, cnt["sx_passes"]), "the tune did not land on the family of this case"
    assert has_copy(A)
    f32_runs(shared, A, mat, what=name)


@pytest.mark.parametrize("name", ["det-nd24k", "det-kkt20"])
def test_deterministic_float_products_are_bit_identical(shared, name):
    torch = shared.torch
    A, mat, _ = sym_case(shared, name)
    n = mat[0][3]
    xh, xf = shared.x(n)
    ys = []
    for _ in range(2):
        y = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
        A.matvec_f32(0.5, xf[2:2 + n], 0.0, y)
        ys.append(y)
    torch.cuda.synchronize()
    assert torch.equal(ys[0], ys[1])
    check_y(mat[3], xh, ys[0].cpu().numpy(), 0.5)


# ---- 2. variations on the SX and the tile case -----------------------------------------------------------------------------

VARIATIONS = {
    "waves-2": {"spx.gpu.waves": "2"},
    "waves-4": {"spx.gpu.waves": "4"},
    "waves-8": {"spx.gpu.waves": "8"},
    "wide-2048": {"spx.gpu.sym_wide_rows": "2048"},
    "rows-200": {"spx.gpu.rowblock_rows": "200", "spx.gpu.sym_wide_rows": "512"},
    "threads-3": {"spx.rt.nr_threads": "3"},
    "segment-min-3": {"spx.gpu.sym_segment_min": "3", "spx.gpu.inline_desc": "false"},
}


@pytest.mark.parametrize("variation", list(VARIATIONS))
@pytest.mark.parametrize("name", ["sx", "atomic"])
def test_variations_of_the_stream(shared, name, variation):
    more = VARIATIONS[variation]
    A, mat, key = sym_case(shared, name, more)
    inf = A.info()
    print("%s %s: %d row-blocks, waves %d, sym_tiles %d, sym_segments %d, sym_pipeline %d" % (
        name, variation, inf.n_rowblocks, inf.waves, inf.sym_tiles, inf.sym_segments, inf.sym_pipeline))
    if variation.startswith("waves-"):
        assert inf.waves == int(more["spx.gpu.waves"])
    if name == "sx":
        assert inf.sym_segments >= 1 and (variation == "segment-min-3" or inf.sym_pipeline == 1)
    else:
        assert inf.sym_tiles == 2
    assert has_copy(A)
    f32_runs(shared, A, mat, pairs=mc.ALPHA_BETA[:2], what="%s %s" % (name, variation))
    shared.drop(key)


@pytest.mark.parametrize("name", ["sx", "atomic", "lists"])
def test_vectors_at_8_mod_16(shared, name):
    """x and y 8 but not 16 bytes aligned: the tile pass' other x path, the SX stage's unaligned pairs"""
    A, mat, _ = sym_case(shared, name)
    f32_runs(shared, A, mat, pairs=mc.ALPHA_BETA[:2], shift=1, what=name + " at 8 mod 16")


# ---- 3. values that change ---------------------------------------------------------------------------------------------------

def _small(name):
    return {"sx": lambda: synth.syn_nlpkkt(44), "atomic": lambda: synth.syn_nd24k(0.05),
            "no-once": lambda: synth.syn_nlpkkt(20)}[name]


@pytest.mark.parametrize("name", ["sx", "atomic", "no-once"])
def test_set_values_writes_both_arrays(shared, name):
    torch = shared.torch
    mname, gen, opts = SYM[name]
    csr = shared.matrix("sym-" + mname, lambda: (gen(), None))[0]
    n = csr[3]
    A = vc.tune(csr, dict(opts, **ALL), sym=True)
    assert has_copy(A)
    A.values_plan(csr[0], csr[1])
    xh, xf = shared.x(n)
    v = vc.new_values(csr, True, 1)
    A.set_values(torch.from_numpy(v.copy()).cuda())
    new = Shared(torch).matrix("new", lambda: (vc.with_values(csr, v), None))
    f32_runs(shared, A, new, pairs=mc.ALPHA_BETA[:2], what=name + " after set_values")
    # ... and the doubles hold the new values unrounded
    check_y(new[0], xh, tf.f64_product(shared, A, n, n).cpu().numpy(), 0.5)
    A.destroy()


def _entry_matrix(csr, r, c, value):
    rp, ci, va, n = csr
    va2 = np.array(va, dtype=np.float64).copy()
    for a, b in ((r, c), (c, r)):
        k = int(rp[a]) + int(np.searchsorted(ci[rp[a]:rp[a + 1]], b))
        assert ci[k] == b
        va2[k] = value
    return (rp, ci, va2, n)


@pytest.mark.parametrize("name", ["sx", "atomic", "no-once"])
def test_set_entry_patches_the_float(shared, name):
    """a strictly lower entry (on no-once its mirror copy is stored too): both uses change in both products; a
    diagonal entry that is no float: the float product sees it rounded, the fp64 product exact"""
    torch = shared.torch
    mname, gen, opts = SYM[name]
    mat = shared.matrix("sym-" + mname, lambda: (gen(), None))
    csr, m, m32 = mat[0], mat[1], mat[2]
    rp, ci, va, n = csr
    A = vc.tune(csr, dict(opts, **ALL), sym=True)
    assert has_copy(A)
    xh, xf = shared.x(n)
    y = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    A.matvec_f32(1.0, xf[2:2 + n], 0.0, y)                          # a product is in flight before the edit
    r = n - n // 5
    c = int(ci[rp[r]])
    assert c < r
    new_value = 1000.0 + 1.0 / 3.0                                  # (not a float)
    assert np.float64(np.float32(new_value)) != new_value
    A.set_entry(r, c, new_value)
    assert A.get_entry(r, c) == new_value and A.get_entry(c, r) == new_value
    csr2 = _entry_matrix(csr, r, c, new_value)
    new = Shared(torch).matrix("entry", lambda: (csr2, None))
    f32_runs(shared, A, new, pairs=mc.ALPHA_BETA[:2], what=name + " after set_entry")
    y.fill_(float("nan"))
    A.matvec_f32(1.0, xf[2:2 + n], 0.0, y)
    torch.cuda.synchronize()
    yh = y.cpu().numpy()
    old = m32 @ xh
    assert abs(yh[r] - old[r]) > 1.0 and abs(yh[c] - old[c]) > 1.0   # (both uses; the old value passes nowhere near)
    check_y(csr2, xh, tf.f64_product(shared, A, n, n).cpu().numpy(), 0.5)
    # the diagonal
    d = n // 3
    dval = 2000.0 + 1.0 / 7.0
    assert np.float64(np.float32(dval)) != dval
    A.set_entry(d, d, dval)
    assert A.get_entry(d, d) == dval
    csr3 = _entry_matrix(csr2, d, d, dval)
    new3 = Shared(torch).matrix("diag", lambda: (csr3, None))
    f32_runs(shared, A, new3, pairs=mc.ALPHA_BETA[:2], what=name + " after set_entry on the diagonal")
    y64 = tf.f64_product(shared, A, n, n, alpha=1.0).cpu().numpy()
    check_y(csr3, xh, y64, 1.0)
    y.fill_(float("nan"))
    A.matvec_f32(1.0, xf[2:2 + n], 0.0, y)
    torch.cuda.synchronize()
    # the two products differ on that row by the rounding of the diagonal entry (and of the row's other entries):
    # the float one holds float(dval) * x, the fp64 one dval * x
    lhs = (y.cpu().numpy()[d] - y64[d])
    rhs = ((new3[2] - new3[1])[d] @ xh)[0]
    assert abs((np.float64(np.float32(dval)) - dval) * xh[d]) > 100 * FP64_BOUND_FACTOR * U * (abs(new3[1])[d] @ np.abs(xh))[0]
    assert abs(lhs - rhs) <= 2 * FP64_BOUND_FACTOR * U * (abs(new3[1])[d] @ np.abs(xh))[0]
    A.destroy()


# ---- 4. two symmetric row slices --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("family", ["lists", "segments"])
def test_two_symmetric_slices_sum_to_the_rounded_product(shared, family):
    """Ranks 0 and 1 of 2 (spx.rt.gpu_world=2) in one process: each partial vector against the rounded part it
    multiplies by -- lower triangle, diagonal and mirror image, the thin mirror list of rank 1 among it -- and their
    sum against the rounded CSR product."""
    torch = shared.torch
    from stream_decode import Stream
    import tempfile, os
    csr, m, m32, csr32 = shared.matrix("thin-mirror", lambda: (dc.MATRICES["thin-mirror"](), None))
    n = csr[3]
    xh, xf = shared.x(n)
    opts = lc.sym_options(family, dict({"spx.gpu.waves": dc.WAVES}, **ALL))
    total = {ab: np.zeros(n) for ab in mc.ALPHA_BETA[:2]}
    ref_total = {ab: np.zeros(n) for ab in mc.ALPHA_BETA[:2]}
    bound_total = {ab: np.zeros(n) for ab in mc.ALPHA_BETA[:2]}
    mirror_rows = []
    for rank in range(2):
        A = dc.tune_rank(csr, rank, 2, opts, symmetric=True)
        inf = A.info()
        lo, hi = inf.row_lo, inf.row_hi
        assert inf.symmetric and 0 <= lo < hi <= n and hi - lo < n
        assert has_copy(A)
        with tempfile.TemporaryDirectory() as d:
            f = os.path.join(d, "slice.spx")
            A.save(f)
            mirror_rows.append(int(Stream(f).mirror_rows.size))
        part = dc.symmetric_part(m, lo, hi)
        part32 = dc.symmetric_part(m32, lo, hi)
        y0 = dc.nan_outside(n, lo, hi, seed=100)
        for alpha, beta in mc.ALPHA_BETA[:2]:
            y = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
            if beta != 0.0:
                y.copy_(torch.from_numpy(y0))
            A.matvec_f32(alpha, xf[2:2 + n], beta, y)
            torch.cuda.synchronize()
            yh = y.cpu().numpy()
            ref, bound = dc.reference(part32, lo, hi, xh, alpha, beta, y0)
            ratio = dc.max_ratio(yh, ref, bound, slice(0, hi))
            print("%s rank %d rows [%d, %d) alpha %g beta %g: max error / bound %.3g, %d rows in the thin mirror list" % (
                family, rank, lo, hi, alpha, beta, ratio, mirror_rows[-1]))
            assert ratio <= 1.0
            assert np.array_equal(yh[hi:], np.zeros(n - hi))
            y0z = np.where(np.isnan(y0), 0.0, y0)
            assert_reads_floats((None, sp.csr_matrix(part), sp.csr_matrix(part32), None), xh, yh, alpha, beta, y0z,
                                "%s rank %d alpha %g" % (family, rank, alpha))
            total[(alpha, beta)] += yh
            ref_total[(alpha, beta)] += ref
            bound_total[(alpha, beta)] += bound
        A.destroy()
    assert mirror_rows[0] == 0 and mirror_rows[1] > 0, mirror_rows
    for alpha, beta in mc.ALPHA_BETA[:2]:
        if beta == 0.0:
            full = alpha * (m32 @ xh)
            r = dc.max_ratio(total[(alpha, beta)], full, bound_total[(alpha, beta)] + 4 * U * np.abs(full))
            assert r <= 1.0, "sum over the ranks: max error / bound %g" % r


# ---- 5. lifecycle and the other option values ---------------------------------------------------------------------------------------

def test_restore_reads_the_option_at_restore_time(shared, tmp_path):
    mname, gen, opts = SYM["sx"]
    mat = shared.matrix("sym-" + mname, lambda: (gen(), None))
    n = mat[0][3]
    A, _, _ = sym_case(shared, "sx")
    f = str(tmp_path / "sx.spx")
    A.save(f)
    for value, copy in (("all", True), ("true", False), ("false", False)):
        sx.options_reset()
        sx.option_set(OPT, value)
        B = sx.mat_restore(f)
        assert B.info().symmetric and B.info().sym_pipeline == 1
        if copy:
            assert has_copy(B)
            f32_runs(shared, B, mat, pairs=mc.ALPHA_BETA[:2], what="restored with all")
        else:
            tf.assert_no_copy(shared, B)
        check_y(mat[0], shared.x(n)[0], tf.f64_product(shared, B, n, n).cpu().numpy(), 0.5)
        B.destroy()
    sx.options_reset()


@pytest.mark.parametrize("name", ["sx", "atomic", "no-once"])
def test_true_keeps_no_copy_on_a_symmetric_tune(shared, name):
    A, mat, key = sym_case(shared, name, option={OPT: "true"})
    tf.assert_no_copy(shared, A)
    shared.drop(key)


@pytest.mark.parametrize("name", ["det-nd24k", "det-kkt20"])
def test_fp64_product_does_not_see_the_copy(shared, name):
    """spx.gpu.deterministic: the fp64 product of a handle with the copy is that of a handle tuned with false, bit
    for bit (before and after float products ran on it)"""
    torch = shared.torch
    A0, mat, key0 = sym_case(shared, name, option={OPT: "false"})
    n = mat[0][3]
    y0 = tf.f64_product(shared, A0, n, n)
    tf.assert_no_copy(shared, A0)
    shared.drop(key0)
    A1, _, _ = sym_case(shared, name)
    assert has_copy(A1)
    y1 = tf.f64_product(shared, A1, n, n)
    y = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    A1.matvec_f32(0.5, shared.x(n)[1][2:2 + n], 0.0, y)
    y2 = tf.f64_product(shared, A1, n, n)
    torch.cuda.synchronize()
    assert torch.equal(y0, y1) and torch.equal(y1, y2), "the fp64 product changed with the copy"
    check_y(mat[0], shared.x(n)[0], y1.cpu().numpy(), 0.5)


@pytest.mark.parametrize("name", ["sx", "notile-30", "atomic", "lists", "tiles+segments", "no-once"])
def test_other_products_still_read_the_doubles(shared, name):
    """the fp64, the multi-vector and the transposed product of a handle with the copy, against unrounded A"""
    torch = shared.torch
    A, mat, _ = sym_case(shared, name)
    csr, m = mat[0], mat[1]
    n = csr[3]
    assert has_copy(A)
    xh, xf = shared.x(n)
    check_y(csr, xh, tf.f64_product(shared, A, n, n).cpu().numpy(), 0.5)
    mc.run(torch, A, m, 3, 2.0, -0.5, padx=tf.PAD, pady=tf.PAD)
    zh, zf = shared.x(n, seed=7)
    y = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    A.matvec_trans(0.5, zf[2:2 + n], 0.0, y)
    torch.cuda.synchronize()
    check_y(csr, zh, y.cpu().numpy(), 0.5)


# ---- 6. stream capture -----------------------------------------------------------------------------------------------------------------

def test_float_product_in_a_captured_graph(shared):
    """the float product of the SX case captured on one stream (one chain: no parallel branches) and replayed twice
    with x changed in between: it only enqueues and allocates nothing"""
    torch = shared.torch
    A, mat, _ = sym_case(shared, "sx")
    assert A.info().sym_pipeline == 1
    n = mat[0][3]
    xh, _ = shared.x(n)
    x2h = shared.x(n, seed=7)[0]
    x = torch.from_numpy(xh.copy()).cuda()
    y = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    A.hip_matvec_kernel_f32(0.5, x.data_ptr(), 0.0, y.data_ptr(), torch.cuda.current_stream().cuda_stream)   # warm-up
    torch.cuda.synchronize()
    y.fill_(float("nan"))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = torch.cuda.current_stream().cuda_stream
        A.hip_matvec_kernel_f32(0.5, x.data_ptr(), 0.0, y.data_ptr(), cap)
    g.replay()
    torch.cuda.synchronize()
    check_y(mat[3], xh, y.cpu().numpy(), 0.5)
    x.copy_(torch.from_numpy(x2h.copy()))
    g.replay()
    torch.cuda.synchronize()
    check_y(mat[3], x2h, y.cpu().numpy(), 0.5)


# ---- 7. iterative refinement with an inner CG -------------------------------------------------------------------------------------------

REFINE_GRID = 27                     # 27^3 = 19683 rows
REFINE_OUTER, REFINE_INNER = 8, 25


def refinement_matrix(g=REFINE_GRID, seed=47):
    """A 7-point Laplacian on a g^3 grid plus a random symmetric perturbation that is strictly diagonally dominant
    with a positive diagonal: SPD, about eight entries per row, no value a float."""
    n = g ** 3
    one = sp.diags([-np.ones(g - 1), 2.0 * np.ones(g), -np.ones(g - 1)], [-1, 0, 1])
    eye = sp.identity(g)
    lap = sp.kron(sp.kron(one, eye), eye) + sp.kron(sp.kron(eye, one), eye) + sp.kron(sp.kron(eye, eye), one)
    rng = np.random.RandomState(seed)
    k = n
    r, c = rng.randint(0, n, k), rng.randint(0, n, k)
    keep = r != c
    off = sp.coo_matrix((rng.uniform(-1.0, 1.0, keep.sum()) / 3.0, (r[keep], c[keep])), shape=(n, n)).tocsr()
    off = off + off.T
    d = np.asarray(abs(off).sum(axis=1)).ravel() + rng.uniform(0.5, 1.0, n)
    scale = 1.0 + rng.uniform(0.0, 1e-3)          # (the Laplacian's integers become non-floats)
    m = sp.csr_matrix(scale * (lap + off + sp.diags(d)) / 3.0)
    m.sum_duplicates()
    m.sort_indices()
    assert (abs(m - m.T)).max() == 0.0
    return (m.indptr.astype(np.int32), m.indices.astype(np.int32), m.data.copy(), n), m


def test_refinement_with_an_inner_cg_on_the_float_product(shared):
    """Iterative refinement on an SPD matrix tuned symmetric with the copy: the residual b - A x from the fp64
    product, the correction from REFINE_INNER steps of CG that use the float product only (device vectors, the
    BLAS-1 helpers, scalars in HBM).  It reaches the fp64 level; with the float product in the residual as well
    it stalls far above.  Thresholds: test_gpu_values_f32.test_refinement_reaches_fp64_with_fp64_residuals_only."""
    csr, m = refinement_matrix()
    n = csr[3]
    assert np.mean(rounded(csr[2]) != csr[2]) > 0.99
    A = tune(csr, dict(NOSAMPLE, **ALL), sym=True)
    assert A.info().symmetric and has_copy(A)
    bh = synth.random_x(n, seed=43)
    b = sx.DeviceVector(host=bh)
    x, r, p, ap, dx = (sx.DeviceVector(n) for _ in range(5))
    S = sx.DeviceVector(3)

    def refine(residual_f32):
        x.init(0.0)
        for _ in range(REFINE_OUTER):
            b.copy_into(r)
            if residual_f32:
                sx.matvec_kernel_f32_vec(A, -1.0, x, 1.0, r)
            else:
                sx.matvec_kernel_vec(A, -1.0, x, 1.0, r)
            # dx: REFINE_INNER steps of CG on fl32(A) dx = r, from dx = 0
            dx.init(0.0)
            r.copy_into(p)
            S.init(0.0)
            r.dot_into(r, S, 0)
            for _ in range(REFINE_INNER):
                sx.matvec_kernel_f32_vec(A, 1.0, p, 0.0, ap)
                p.dot_into(ap, S, 1)
                sx.cg_update(dx, p, r, ap, S)
                r.scale_add_ratio_into(p, p, 1.0, (S, 2))
            x.scale_add_into(dx, x, 1.0)
        xh = x.download()
        ld = np.longdouble
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
    assert good.max() <= tf.REFINE_FACTOR
    assert np.median(stalled) > 100.0 * tf.REFINE_FACTOR
    A.destroy()
