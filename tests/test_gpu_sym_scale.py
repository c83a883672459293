"""Norms and the scaling D * A * D of a matrix tuned as a symmetric one, in HBM (spx_hip_mat_sym_norms,
spx_hip_mat_sym_scale: csx_sym_norms_kernel and csx_sym_scale_kernel of sym_scale_kernels.hip): one case per kernel
family of the symmetric product, the norms against numpy over the full symmetric CSR arrays (the max kind bit for
bit, the sums within count * 2^-52), the scaled values bit for bit in every stored copy of the stream, the products,
the diagonal and the float copy after a scaling, the walker at the limits of the stream's fields, row slices, a
Jacobi scaling, a captured graph, and the calls that must fail.  Matrices are shared per module; a handle that a test
scales is that test's own."""
import numpy as np
import pytest

import sparsex_amd as sx
from sparsex_amd import synth
from sparsex_amd.api import SpxError

import dist_cases as dc
import limit_cases as lc
import matmat_cases as mc
import scale_cases as sc
import sym_scale_cases as ssc
import values_cases as vc
import test_gpu_values_f32 as tf
import test_gpu_values_f32_sym as tfs
from diag_cases import bits, matrix
from helpers import check_y
from test_gpu_values_f32 import Shared, f32_runs

pytestmark = pytest.mark.gpu

ALL = tfs.ALL
FAMILIES = ("sx", "notile-30", "atomic", "lists", "tiles+segments", "det-kkt20", "no-once")
PERIOD = 65537
_lds_seen = {"doubles": 0, "case": None}


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.float64)).cuda()


def sentinels(n):
    return sx.DeviceVector(host=np.full(n, ssc.SENTINEL))


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
    print("largest dynamic LDS of a norms launch: %d bytes (%s)" % (8 * _lds_seen["doubles"], _lds_seen["case"]))


def note_lds(stream, what):
    d = ssc.lds_doubles(stream)
    if d > _lds_seen["doubles"]:
        _lds_seen.update(doubles=d, case=what)
    print("%s: dynamic LDS of a norms launch %d bytes (largest so far %d, %s)" % (
        what, 8 * d, 8 * _lds_seen["doubles"], _lds_seen["case"]))
    return d


def device_norms(A, n, how="vector"):
    """kind -> the n norms on the host, read into sentinels: a DeviceVector, or the raw pointer 8 bytes into a longer
    vector whose neighbours survive"""
    def norms_of(kind):
        if how == "vector":
            out = sentinels(n)
            assert A.sym_norms(kind, out) is out
            return out.download()
        long = sentinels(n + 3)
        A.hip_mat_sym_norms(kind, long.data_ptr() + 8)
        g = long.download()
        assert g[0] == ssc.SENTINEL and g[n + 1] == ssc.SENTINEL and g[n + 2] == ssc.SENTINEL
        return g[1:n + 1]
    return norms_of


def products_and_diagonal(shared, A, csr, m, lo=0, hi=None):
    """forward, transposed and column-major multi-vector product and the diagonal against the CSR product of `csr`"""
    torch = shared.torch
    n = csr[3]
    hi = n if hi is None else hi
    xh, xf = shared.x(n)
    check_y(csr, xh, tf.f64_product(shared, A, n, n).cpu().numpy(), 0.5)
    zh, zf = shared.x(n, seed=7)
    y = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    A.matvec_trans(0.5, zf[2:2 + n], 0.0, y)
    torch.cuda.synchronize()
    check_y(csr, zh, y.cpu().numpy(), 0.5)
    mc.run(torch, A, m, 3, 2.0, -0.5, padx=tf.PAD, pady=tf.PAD)
    d = A.get_diag(sentinels(n)).download()
    assert np.array_equal(bits(d[lo:hi]), bits(m.diagonal()[lo:hi]))


def scale_and_check(shared, A, csr, tmp_path, what, products=True, period=None):
    """norms, sym_scale with a vector of mixed signs, every stored copy; returns (scaled values, scipy matrix,
    decoded stream)"""
    n = csr[3]
    ssc.check_all_norms(device_norms(A, n), csr)
    d = ssc.vector(n, 1, period)
    A.sym_scale(sx.DeviceVector(host=d))
    v1, m1 = ssc.scaled_matrix(csr, d)
    after = vc.check_stream(A, m1, tmp_path, sym=True)
    note_lds(after, what)
    ssc.check_all_norms(device_norms(A, n, "offset"), vc.with_values(csr, v1))
    if products:
        products_and_diagonal(shared, A, vc.with_values(csr, v1), m1)
    return v1, m1, after


# ---- 1. one case per kernel family of the symmetric product ---------------------------------------------------------

@pytest.mark.parametrize("name", FAMILIES)
def test_every_family(shared, name, tmp_path):
    mname, gen, opts = tfs.SYM[name]
    csr = shared.matrix("sym-" + mname, lambda: (gen(), None))[0]
    n = csr[3]
    A = vc.tune(csr, opts, sym=True)
    inf = A.info()
    _, _, cnt = A.sym_pipeline()
    print("%s: %d row-blocks, waves %d, sym_tiles %d, sym_segments %d, sym_pipeline %d (%d SX passes), wave tiles %d" % (
        name, inf.n_rowblocks, inf.waves, inf.sym_tiles, inf.sym_segments, inf.sym_pipeline, cnt["sx_passes"], inf.wave_tiles))
    assert tfs.landed(name, inf, cnt["sx_passes"]), "the tune did not land on the family of this case"
    A.values_plan(csr[0], csr[1])
    plan = A.values_plan_info()["src_values"]
    before = vc.decoded(A, tmp_path, "before.spx")
    v1, m1, after = scale_and_check(shared, A, csr, tmp_path, name)
    sc.untouched_positions(before, after, plan)
    with pytest.raises(SpxError):
        A.export_csx(inf.first_partition)                      # stale, as after set_values
    # powers of two through the host form of a matrix in HBM, undone by their reciprocals in a torch tensor on the
    # current stream
    torch = shared.torch
    p = ssc.pow2_vector(n, 3)
    A.sym_scale(p)
    mid = vc.decoded(A, tmp_path, "mid.spx")
    assert not np.array_equal(bits(mid.values), bits(after.values))
    A.sym_scale(dev(1.0 / p))
    torch.cuda.synchronize()
    again = vc.decoded(A, tmp_path, "again.spx")
    assert np.array_equal(bits(again.values), bits(after.values)) and np.array_equal(bits(again.dvalues), bits(after.dvalues))
    assert np.array_equal(bits(again.mirror_val), bits(after.mirror_val))
    # the host form of the norms, a vector made on request
    out = np.full(n, ssc.SENTINEL)
    A.sym_norms_host(sx.NORM_MAX_ABS, out)
    assert np.array_equal(bits(out), bits(ssc.expected_norms(vc.with_values(csr, v1), sx.NORM_MAX_ABS)[0]))
    made = A.sym_norms(sx.NORM_MAX_ABS)
    assert isinstance(made, sx.DeviceVector) and np.array_equal(bits(made.download()), bits(out))
    # a refresh overwrites with what the caller hands over
    A.set_values(dev(csr[2]))
    torch.cuda.synchronize()
    back = vc.decoded(A, tmp_path, "back.spx")
    assert np.array_equal(bits(back.values), bits(before.values)) and np.array_equal(bits(back.dvalues), bits(before.dvalues))
    A.destroy()


# ---- 2. wavefronts per workgroup ------------------------------------------------------------------------------------

@pytest.mark.parametrize("waves", (2, 4, 8))
@pytest.mark.parametrize("name", ("notile-30", "atomic"))
def test_waves(shared, name, waves, tmp_path):
    mname, gen, opts = tfs.SYM[name]
    csr = shared.matrix("sym-" + mname, lambda: (gen(), None))[0]
    A = vc.tune(csr, dict(opts, **{"spx.gpu.waves": str(waves)}), sym=True)
    assert A.info().waves == waves
    scale_and_check(shared, A, csr, tmp_path, "%s waves %d" % (name, waves), products=False)
    A.destroy()


# ---- 3. the limits of the stream's fields (limit_cases.py) ----------------------------------------------------------

# The families whose streams differ for this walker: "atomic" (tiles next to lower copies and mirror images; "lists" and
# "det" hand the same passes over in another way), "segments" (read-once segments, wide row-blocks) and "pipeline"
# (the same with the headers of the pipelined kernel next to the plain ones).
LIMIT_FAMILIES = ("atomic", "segments", "pipeline")


def limit_case(shared, csr, opts, family, waves, what, tmp_path, period=None):
    A = vc.tune(csr, dict(lc.sym_options(family, opts), **{"spx.gpu.waves": str(waves)}), sym=True)
    inf = A.info()
    assert inf.symmetric and inf.waves == waves
    print("%s %s: sym_tiles %d, sym_segments %d, sym_pipeline %d" % (what, family, inf.sym_tiles, inf.sym_segments, inf.sym_pipeline))
    scale_and_check(shared, A, csr, tmp_path, "%s %s waves %d" % (what, family, waves), products=False, period=period)
    A.destroy()
    return inf


@pytest.mark.parametrize("waves", lc.PASS_WAVES)
@pytest.mark.parametrize("family", ("atomic", "segments"))
def test_pass_counts_at_the_edges_of_the_wavefronts_turns(shared, family, waves, tmp_path):
    """row-blocks of 1, W, W + 1, 2 W, 2 W + 1 and 3 W + 1 passes; with segments, wide row-blocks whose passes add
    elem0 to the rows of their descriptors"""
    csr = shared.matrix("passes-edge-sym", lc.pass_edges_sym)[0]
    limit_case(shared, csr, lc.PASS_SYM_OPTS, family, waves, "passes-edge-sym", tmp_path)


@pytest.mark.parametrize("family", LIMIT_FAMILIES)
def test_column_offsets_of_24_bits(shared, family, tmp_path):
    csr = shared.matrix("off-sym-3", lc.SYM_OFFSETS["off-sym-3"][0])[0]
    limit_case(shared, csr, {}, family, 4, "off-sym-3", tmp_path, period=PERIOD)


@pytest.mark.parametrize("family", LIMIT_FAMILIES)
@pytest.mark.parametrize("case", ["step-127-sym", "slots-3072", "slots-wide-cap", "noslot"])
def test_symmetric_limit_cases(shared, case, family, tmp_path):
    """a chain of read-once segments with row and column step 127, 3072 and 8192 slots (the latter with 2048 rows:
    80 KB of LDS in a norms launch), lanes without a slot.  (limit_cases.STEPS holds no symmetric entry.)"""
    assert not [k for k, v in lc.STEPS.items() if v[2]]
    gen, opts, _ = lc.SYM_CASES[case]
    csr = shared.matrix(case, gen)[0]
    inf = limit_case(shared, csr, opts, family, 4, case, tmp_path)
    if family != "atomic":
        assert inf.sym_segments > 0


# ---- 4. row slices --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case,how", [("thin-mirror-w3-balanced", "row-offset"), ("nd24k-w3-shifted", "rank")])
def test_three_slices(shared, case, how, tmp_path):
    """d and out inside NaN-padded tensors: a write outside out shows; the partial results join to the whole
    matrix' norms"""
    torch = shared.torch
    mname, world, kind, extra, _, _ = dc.CASES[case]
    csr = dc.matrix(case)
    n = csr[3]
    cuts = dc.cut(csr, world, kind)
    opts = dict(dc.NOSAMPLE, **dict(extra, **{"spx.gpu.waves": dc.WAVES}))
    d = ssc.vector(n, 1)
    dpad = torch.full((n + 6,), float("nan"), dtype=torch.float64, device="cuda")
    dpad[2:2 + n] = torch.from_numpy(d.copy())
    v1, m1 = ssc.scaled_matrix(csr, d)
    parts = {k: [] for k in ssc.KINDS}
    counts = {k: [] for k in ssc.KINDS}
    mirror = []
    for rank in range(world):
        if how == "rank":
            A = dc.tune_rank(csr, rank, world, opts, symmetric=True)
        else:
            A = dc.tune_rows(csr, cuts[rank], cuts[rank + 1], opts, symmetric=True)
        inf = A.info()
        lo, hi = inf.row_lo, inf.row_hi
        assert inf.symmetric and inf.on_device and 0 <= lo < hi <= n and hi - lo < n

        def norms_of(k):
            pad = torch.full((n + 6,), float("nan"), dtype=torch.float64, device="cuda")
            A.sym_norms(k, pad[2:2 + n])
            torch.cuda.synchronize()
            h = pad.cpu().numpy()
            assert np.isnan(h[:2]).all() and np.isnan(h[2 + n:]).all(), "a write outside out"
            return h[2:2 + n].copy()

        ssc.check_all_norms(norms_of, csr, lo, hi)
        for k in ssc.KINDS:
            parts[k].append(norms_of(k))
            counts[k].append(ssc.expected_norms(csr, k, lo, hi)[1])
        A.sym_scale(dpad[2:2 + n])
        torch.cuda.synchronize()
        after = vc.check_stream(A, m1, tmp_path, sym=True)
        note_lds(after, "%s rank %d" % (case, rank))
        mirror.append(int(after.mirror_rows.size))
        ssc.check_all_norms(norms_of, vc.with_values(csr, v1), lo, hi)
        got_d = A.get_diag(sentinels(n)).download()
        assert np.array_equal(bits(got_d[lo:hi]), bits(m1.diagonal()[lo:hi]))
        # the product of the slice: the part of the scaled matrix it multiplies by
        part = dc.symmetric_part(m1, lo, hi)
        xh, xf = shared.x(n)
        y = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
        A.hip_matvec_kernel(0.5, xf[2:2 + n].data_ptr(), 0.0, y.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        ref, bound = dc.reference(part, lo, hi, xh, 0.5)
        assert dc.max_ratio(y.cpu().numpy(), ref, bound, slice(0, hi)) <= 1.0
        A.destroy()
    print("%s (%s): rows in the thin mirror lists %r" % (case, how, mirror))
    if case == dc.THIN_MIRROR:
        assert mirror[-1] > 0, "the last slice has no thin mirror list"
    for k in ssc.KINDS:
        ssc.check_joined(k, parts[k], counts[k], csr)
    sx.options_reset()


# ---- 5. the float copy ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ("sx", "atomic", "no-once"))
def test_float_copy_follows_the_scaling(shared, name, tmp_path):
    """matvec_f32 after the scaling against the CSR whose scaled values are rounded to float, diagonal included"""
    torch = shared.torch
    mname, gen, opts = tfs.SYM[name]
    csr = shared.matrix("sym-" + mname, lambda: (gen(), None))[0]
    n = csr[3]
    A = vc.tune(csr, dict(opts, **ALL), sym=True)
    assert tfs.has_copy(A)
    d = ssc.vector(n, 1)
    A.sym_scale(sx.DeviceVector(host=d))
    v1, m1 = ssc.scaled_matrix(csr, d)
    assert np.mean(tf.rounded(v1) != v1) > 0.9
    new = Shared(torch).matrix("scaled", lambda: (vc.with_values(csr, v1), None))
    f32_runs(shared, A, new, pairs=mc.ALPHA_BETA[:2], what=name + " after sym_scale")
    # ... and the doubles hold the scaled values unrounded
    vc.check_stream(A, m1, tmp_path, sym=True)
    check_y(new[0], shared.x(n)[0], tf.f64_product(shared, A, n, n).cpu().numpy(), 0.5)
    A.destroy()


# ---- 6. Jacobi scaling, eager and in a captured graph ---------------------------------------------------------------

def test_jacobi_scaling_gives_a_unit_diagonal(shared, tmp_path):
    """get_diag, rsqrt, sym_scale on an SPD matrix: the new diagonal is within 4 * 2^-52 of 1 -- six roundings of at
    most 2^-53 each (square root, division, two products with the factor squared in effect) plus second order"""
    csr, m = tfs.refinement_matrix()
    n = csr[3]
    A = vc.tune(csr, {"spx.gpu.waves": "4"}, sym=True)
    d = sx.DeviceVector(n)
    A.get_diag(d)
    d.rsqrt(d, if_zero=1.0)
    A.sym_scale(d)
    got = A.get_diag(sentinels(n)).download()
    err = np.abs(got - 1.0).max()
    print("Jacobi: max |a(i,i) - 1| = %.3g * 2^-52" % (err / 2.0 ** -52))
    assert err <= 4 * 2.0 ** -52
    dh = d.download()
    assert np.array_equal(bits(dh), bits(1.0 / np.sqrt(m.diagonal())))
    vc.check_stream(A, ssc.scaled_matrix(csr, dh)[1], tmp_path, sym=True)
    A.destroy()


def test_jacobi_and_norms_in_a_captured_graph(shared, tmp_path):
    """get_diag -> rsqrt -> sym_scale -> sym_norms(MAX_ABS) as one chain on one stream (no parallel branches),
    replayed once: the stream, the factors and the norms equal, bit for bit, the eager sequence on a second,
    identically tuned handle.  Every call ran once before the capture; that first chain scaled both handles alike."""
    import torch
    csr, _ = tfs.refinement_matrix()
    n = csr[3]
    opts = {"spx.gpu.waves": "4"}

    class T:
        pass
    ts = []
    for _ in range(2):
        t = T()
        t.A = vc.tune(csr, opts, sym=True)
        t.d, t.out = sentinels(n), sentinels(n)
        ts.append(t)
    ta, tb = ts

    def chain(t, s):
        t.A.get_diag(t.d, stream=s)
        t.d.rsqrt(t.d, if_zero=1.0, stream=s)
        t.A.sym_scale(t.d, stream=s)
        t.A.sym_norms(sx.NORM_MAX_ABS, t.out, stream=s)

    s = torch.cuda.current_stream().cuda_stream
    chain(ta, s)                                          # warm-up outside the capture
    chain(tb, s)
    torch.cuda.synchronize()
    first = vc.decoded(ta.A, tmp_path, "first.spx")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        chain(ta, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(bits(vc.decoded(ta.A, tmp_path, "cap.spx").values), bits(first.values))   # (the capture ran nothing)
    g.replay()
    chain(tb, s)
    torch.cuda.synchronize()
    sa, sb = vc.decoded(ta.A, tmp_path, "a.spx"), vc.decoded(tb.A, tmp_path, "b.spx")
    assert np.array_equal(bits(sa.values), bits(sb.values)) and np.array_equal(bits(sa.dvalues), bits(sb.dvalues))
    assert np.array_equal(bits(ta.d.download()), bits(tb.d.download()))
    assert np.array_equal(bits(ta.out.download()), bits(tb.out.download()))
    # ... and it is the chain: two of them by numpy
    v = csr[2]
    for _ in range(2):
        diag = vc.to_scipy(vc.with_values(csr, v)).diagonal()
        assert (diag > 0).all()
        v = ssc.scaled_values(vc.with_values(csr, v), 1.0 / np.sqrt(diag))
    vc.check_stream(ta.A, vc.to_scipy(vc.with_values(csr, v)), tmp_path, sym=True)
    assert np.array_equal(bits(ta.out.download()), bits(ssc.expected_norms(vc.with_values(csr, v), sx.NORM_MAX_ABS)[0]))
    for t in ts:
        t.A.destroy()
    sx.options_reset()


# ---- 7. calls that must fail ----------------------------------------------------------------------------------------

def test_calls_that_must_fail(tmp_path, capfd):
    import torch
    csr = matrix("nlpkkt")
    n = csr[3]
    W4 = {"spx.gpu.waves": "4"}
    out, d = sentinels(n), sx.DeviceVector(host=sc.vector(n, 1))

    def refused(A, what):
        capfd.readouterr()
        before = vc.decoded(A, tmp_path, "r0.spx")
        for call in (lambda: A.sym_norms(sx.NORM_MAX_ABS, out), lambda: A.hip_mat_sym_norms(sx.NORM_SUM_SQ, out.data_ptr()),
                     lambda: A.sym_scale(d), lambda: A.hip_mat_sym_scale(d.data_ptr())):
            with pytest.raises(SpxError):
                call()
        assert what in capfd.readouterr().err
        torch.cuda.synchronize()
        assert (out.download() == ssc.SENTINEL).all()
        after = vc.decoded(A, tmp_path, "r1.spx")
        assert np.array_equal(bits(after.values), bits(before.values)) and np.array_equal(bits(after.dvalues), bits(before.dvalues))

    # a general tune (the host forms too)
    G = vc.tune(csr, W4)
    refused(G, "tuned as a general one")
    with pytest.raises(SpxError):
        G.sym_norms_host(sx.NORM_MAX_ABS)
    with pytest.raises(SpxError):
        G.sym_scale(np.ones(n))
    G.export_csx(G.info().first_partition)                 # nothing went stale
    G.destroy()
    # a symmetric matrix with an exchange plan attached (a communicator of one rank)
    tr = sx.RcclTransport(sx.rccl_unique_id(), 0, 1)
    D = vc.tune(csr, W4, sym=True)
    D.dist_attach(tr)
    refused(D, "exchange plan")
    D.destroy()
    tr.destroy()
    # the device forms on a host-only matrix; the arguments of a good handle
    H = vc.tune(csr, W4, sym=True, host_only=True)
    refused(H, "host_only")
    H.destroy()
    A = vc.tune(csr, W4, sym=True)
    L = sx.lib()
    assert L.spx_hip_mat_sym_norms(A.handle, 3, out.data_ptr(), None) == sx.SPX_FAILURE
    assert L.spx_hip_mat_sym_norms(A.handle, 0, None, None) == sx.SPX_FAILURE
    assert L.spx_hip_mat_sym_scale(A.handle, None, None) == sx.SPX_FAILURE
    assert L.spx_hip_mat_sym_norms(None, 0, out.data_ptr(), None) == sx.SPX_FAILURE
    assert L.spx_hip_mat_sym_scale(None, d.data_ptr(), None) == sx.SPX_FAILURE
    torch.cuda.synchronize()
    assert (out.download() == ssc.SENTINEL).all()
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
    A = vc.tune(csr, {"spx.gpu.waves": "4"}, sym=True)
    out, d = sentinels(n), sx.DeviceVector(host=sc.vector(n, 1))
    try:
        torch.cuda.set_device(1)
        with pytest.raises(SpxError):
            A.hip_mat_sym_norms(sx.NORM_MAX_ABS, out.data_ptr())
        with pytest.raises(SpxError):
            A.hip_mat_sym_scale(d.data_ptr())
        with pytest.raises(SpxError):
            A.sym_norms_host(sx.NORM_MAX_ABS)
    finally:
        torch.cuda.set_device(0)
    assert (out.download() == ssc.SENTINEL).all()
    A.destroy()
    sx.options_reset()
