"""The transposed product spx_hip_matvec_trans_kernel / Matrix.matvec_trans on the GPU, y <- alpha*A^T*x + beta*y
over the stream A was tuned into (csx_spmv_t_kernel): against the CSR product of the transposed matrix
(helpers.check_y / matmat_cases.check_y_rect on a.T.tocsr()), with per-nonzero adds (spx.gpu.trans_windows=false)
and with the unit windows accumulating in LDS (true), on every kind of general stream -- unit passes of widths 1
to 8, gather passes of 16, 24 and 32 bits, window passes, over-long rows, column phases, rectangular matrices,
the limits of limit_cases.py -- and on symmetric tunes, where the forward product runs.  Then what
spx_hip_matvec_trans_mode reports, the adjoint identity, row slices, argument failures, a captured graph,
set_entry and the forward product's state.  Tuned matrices are shared per module."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import scipy.sparse as sp

import sparsex_amd as sx
from sparsex_amd import synth
from helpers import GOLDEN, FP64_BOUND_FACTOR, check_y, tune
import dist_cases as dc
import limit_cases as lc
import matmat_cases as mc

pytestmark = pytest.mark.gpu

PAD = 3          # NaN behind (and two doubles in front of) every vector on the device
NOSAMPLE = mc.NOSAMPLE
TW = "spx.gpu.trans_windows"


def _golden(name):
    with open(os.path.join(GOLDEN, "reference_matrices.json")) as f:
        m = json.load(f)[name]
    csr = (np.array(m["rowptr"], dtype=np.int32), np.array(m["colind"], dtype=np.int32), np.array(m["values"]), m["n"])
    return csr, None


def _square(gen):
    return lambda: (gen(), None)


def _band(name):
    return lambda: mc.band(**mc.BANDS[name][0])


# name -> (generator of (csr tuple, scipy matrix or None), options, whether a window plan can exist)
CASES = {
    "demopatt": (lambda: _golden("demopatt"), dict(NOSAMPLE, **{"spx.preproc.xform": "all"}), True),
    "cant": (_square(lambda: synth.syn_cant(0.05)), NOSAMPLE, True),
    "nlpkkt": (_square(lambda: synth.syn_nlpkkt(20)), NOSAMPLE, True),
    "webbase": (_square(lambda: synth.syn_webbase(0.02)), NOSAMPLE, True),
    "long-rows": (_square(mc.long_rows), NOSAMPLE, True),
    "band-400": (_band("band-400"), mc.band_options("pinned"), True),
    "band-wide": (_band("band-wide"), mc.band_options("pinned"), True),
    "band-tall": (_band("band-tall"), mc.band_options("pinned"), True),
    "phases-c2": (_square(lambda: synth.syn_nlpkkt(20)), dict(NOSAMPLE, **{"spx.gpu.col_phases": "c2"}), False),
    "phases-2": (_square(lambda: synth.syn_nlpkkt(20)), dict(NOSAMPLE, **{"spx.gpu.col_phases": "2"}), False),
    "phases-c4": (_square(lambda: synth.syn_webbase(0.02)), dict(NOSAMPLE, **{"spx.gpu.col_phases": "c4"}), False),
}
# the matrix a case generates, by a name of its own where several cases share it
MATRIX_OF = {"phases-c2": "nlpkkt", "phases-2": "nlpkkt", "phases-c4": "webbase"}
RUNS = [(name, tw) for name, c in CASES.items() for tw in (("false", "true") if c[2] else ("auto",))]
WAVE_RUNS = [(name, waves, tw) for name in ("cant", "nlpkkt") for waves in (2, 4, 8) for tw in ("false", "true")]


class Shared:
    """Matrices (with their transposes in CSR form), tuned handles and vectors, made once and shared."""

    def __init__(self, torch):
        self.torch = torch
        self.mats, self.tuned, self.xs = {}, {}, {}

    def matrix(self, name, gen):
        """(csr tuple, scipy matrix, its transpose in CSR form, the transpose's csr tuple)"""
        if name not in self.mats:
            csr, m = gen()
            if m is None:
                m = mc.to_scipy(csr)
            mt = m.T.tocsr()
            mt.sort_indices()
            self.mats[name] = (csr, m, mt, (mt.indptr, mt.indices, mt.data, mt.shape[0]))
        return self.mats[name]

    def load(self, key, csr, m, opts, sym=False):
        if key not in self.tuned:
            if m.shape[0] != m.shape[1]:
                self.tuned[key] = mc.load_rect(sx, csr, m.shape[1], opts)
            else:
                self.tuned[key] = tune(csr, opts, sym=sym)
        return self.tuned[key]

    def case(self, name, tw, waves=None):
        gen, opts, _ = CASES[name]
        mat = self.matrix(MATRIX_OF.get(name, name), gen)
        o = dict(opts, **{TW: tw})
        if waves is not None:
            o["spx.gpu.waves"] = str(waves)
        return self.load((name, tw, waves), mat[0], mat[1], o), mat

    def x(self, n, seed=5):
        """random vector of n elements (host, read-only) and a device tensor [NaN, NaN, x, NaN * PAD]"""
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


def expected_mode(A, tw):
    """What spx.gpu.trans_windows and the plan the device copy holds imply (the `auto` rule: windows where the
    plan stages fewer doubles than it serves nonzeros)."""
    inf = A.info()
    if inf.symmetric:
        return 0
    if inf.unit_window_lds == 0 or tw == "false":          # (no plan: nothing to accumulate in)
        return 1
    if tw == "true":
        return 2
    return 2 if inf.unit_window_staged < inf.unit_window_elems else 1


def trans_runs(shared, A, mat, pairs=mc.ALPHA_BETA, shift=2, what=""):
    """A.matvec_trans for every (alpha, beta) on vectors inside NaN-padded tensors (`shift`: where they start, in
    doubles: 2 = 16-byte aligned, 1 = not), beta == 0 over a y of NaN; each result against the CSR product of the
    transposed matrix."""
    torch = shared.torch
    csr, m, mt, csr_t = mat
    nr, nc = m.shape
    xh, xf = shared.x(nr)
    if shift != 2:
        xf = torch.full((nr + PAD + 2,), float("nan"), dtype=torch.float64, device="cuda")
        xf[shift:shift + nr] = torch.from_numpy(xh.copy())
    xv = xf[shift:shift + nr]
    assert xv.data_ptr() % 16 == (0 if shift == 2 else 8)
    y0h = shared.x(nc, seed=9)[0]
    for alpha, beta in pairs:
        yf = torch.full((nc + PAD + 2,), float("nan"), dtype=torch.float64, device="cuda")
        yv = yf[shift:shift + nc]
        if beta != 0.0:
            yv.copy_(torch.from_numpy(y0h.copy()))
        out = A.matvec_trans(alpha, xv, beta, yv)
        torch.cuda.synchronize()
        assert out is yv
        yh = yv.cpu().numpy()
        assert torch.isnan(yf[:shift]).all() and torch.isnan(yf[shift + nc:]).all(), "the padding of y was written"
        assert torch.isnan(xf[:shift]).all() and torch.isnan(xf[shift + nr:]).all()
        assert torch.equal(xv.cpu(), torch.from_numpy(xh.copy())), "x was written"
        mc.check_y_rect(mt, csr_t, xh, yh, alpha, beta, y0h if beta != 0.0 else None)


# ---- 1. the result against the CSR product of the transposed matrix ---------------------------------------------

@pytest.mark.parametrize("name,tw", RUNS)
def test_result_matches_csr_of_the_transpose(shared, name, tw):
    A, mat = shared.case(name, tw)
    mode = A.trans_mode()
    inf = A.info()
    print("%s trans_windows=%s: mode %d, %d row-blocks, staged %d, window nonzeros %d" % (
        name, tw, mode, inf.n_rowblocks, inf.unit_window_staged, inf.unit_window_elems))
    assert mode == expected_mode(A, tw)
    if not CASES[name][2]:
        assert mode == 1               # (column phases: several launches or XCD groups, no plan)
    trans_runs(shared, A, mat)


@pytest.mark.parametrize("name,waves,tw", WAVE_RUNS)
def test_wavefront_counts(shared, name, waves, tw):
    """csx_spmv_t_kernel<2 | 4 | 8, windows or not>: the six instances."""
    A, mat = shared.case(name, tw, waves)
    assert A.info().waves == waves
    assert A.trans_mode() == (2 if tw == "true" else 1)
    trans_runs(shared, A, mat)


@pytest.mark.parametrize("tw", ["false", "true"])
def test_misaligned_pointers(shared, tw):
    """x and y at addresses that are 8 but not 16 bytes aligned"""
    A, mat = shared.case("cant", tw)
    trans_runs(shared, A, mat, pairs=mc.ALPHA_BETA[:2], shift=1)


# ---- the limits of the stream's fields (limit_cases.py) -----------------------------------------------------------

OFF_RUNS = [("off-65536", "plain"), ("off-2p24", "plain"), ("off-65536", "unit-windows"), ("off-2p24", "unit-windows"),
            ("off-2x-65536", "slices-c2"), ("off-2x-2p24", "slices-c2")]


@pytest.mark.parametrize("case,family", OFF_RUNS)
def test_offsets_of_24_and_32_bits(shared, case, family):
    """SPX_LOAD_INDEX in the scatter direction: u16 + u8 and u32 column offsets, plain, with a window plan and in
    two column slices in one launch."""
    assert case in lc.OFFSETS and (case, family) in lc.OFF_WIDTHS and min(lc.OFF_WIDTHS[(case, family)]) >= 3
    mat = shared.matrix(case, lambda: lc.wide_offsets(lc.OFFSETS[case][0]))
    for tw in (("false", "true") if family == "unit-windows" else ("auto",)):
        A = shared.load((case, family, tw), mat[0], mat[1], dict(lc.off_options(family), **{TW: tw}))
        assert A.trans_mode() == expected_mode(A, tw)
        assert family == "unit-windows" or A.trans_mode() == 1
        trans_runs(shared, A, mat)
        shared.tuned.pop((case, family, tw)).destroy()


LINEAR_TRANS_MODES = ("waves-2", "waves-4", "waves-8", "unit-windows")


@pytest.mark.parametrize("mode", LINEAR_TRANS_MODES)
@pytest.mark.parametrize("case", list(lc.LINEAR))
def test_steps_segments_and_pass_counts(shared, case, mode):
    """unit_origin in the scatter direction: steps of 127 and 128, 8188 segments in front, joined row-blocks
    (SpxPass::elem0), the pass counts at the edges of the wavefronts' turns."""
    gen, _ = lc.LINEAR[case]
    mat = shared.matrix("diagonals" if case.startswith("segs") else case, gen)
    for tw in (("false", "true") if mode == "unit-windows" else ("auto",)):
        A = shared.load((case, mode, tw), mat[0], mat[1], dict(lc.linear_options(case, mode), **{TW: tw}))
        assert A.trans_mode() == expected_mode(A, tw)
        assert mode == "unit-windows" or A.trans_mode() == 1
        trans_runs(shared, A, mat)
        shared.tuned.pop((case, mode, tw)).destroy()


# ---- 2. the mode -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c[2]])
def test_mode_follows_option_and_plan(shared, name):
    for tw in ("false", "true", "auto"):
        A, _ = shared.case(name, tw)
        inf = A.info()
        print("%s %s: plan %s, staged %d, window nonzeros %d -> mode %d" % (
            name, tw, "yes" if inf.unit_window_lds else "no", inf.unit_window_staged, inf.unit_window_elems, A.trans_mode()))
        assert A.trans_mode() == expected_mode(A, tw)


def test_auto_counts_atomic_bytes(shared):
    """cant stages fewer doubles than its windows serve nonzeros: auto takes the windows; webbase stages more:
    auto adds per nonzero, and `true` still forces the windows."""
    A, _ = shared.case("cant", "auto")
    inf = A.info()
    assert 0 < inf.unit_window_staged < inf.unit_window_elems and A.trans_mode() == 2
    A, _ = shared.case("webbase", "auto")
    inf = A.info()
    assert inf.unit_window_staged > inf.unit_window_elems > 0 and A.trans_mode() == 1
    assert shared.case("webbase", "true")[0].trans_mode() == 2


def test_mode_2_with_unwindowed_row_blocks(shared):
    """at least one case runs windowed and unwindowed row-blocks in one launch"""
    mixed = []
    for name in ("webbase", "nlpkkt"):
        A, _ = shared.case(name, "true")
        plan = A.unit_windows(3072, 16)
        print("%s: %d of %d row-blocks with unit passes have windows" % (
            name, plan["rowblocks_with_windows"], plan["rowblocks_with_units"]))
        assert plan["staged_doubles"] == A.info().unit_window_staged       # (the plan the device copy holds)
        if A.trans_mode() == 2 and 0 < plan["rowblocks_with_windows"] < plan["rowblocks_with_units"]:
            mixed.append(name)
    assert mixed


@pytest.mark.parametrize("opts", [{"spx.gpu.unit_windows": "false"}, {"spx.gpu.deterministic": "true"}],
                         ids=["unit_windows=false", "deterministic"])
def test_no_plan_no_windows(shared, opts):
    mat = shared.matrix("cant", CASES["cant"][0])
    A = shared.load(("cant", "true", tuple(opts)), mat[0], mat[1], dict(NOSAMPLE, **dict(opts, **{TW: "true"})))
    assert A.info().unit_window_lds == 0 and A.trans_mode() == 1
    trans_runs(shared, A, mat, pairs=mc.ALPHA_BETA[:1])


@pytest.fixture(scope="module")
def saved_cant(shared, tmp_path_factory):
    """cant tuned with the module's options, with the unit windows forced on and without a window plan, each saved.
    All three tunes see the default spx.gpu.trans_windows (auto): the option is not part of the file."""
    mat = shared.matrix("cant", CASES["cant"][0])
    d = tmp_path_factory.mktemp("trans")
    files, windows = {}, {}
    for key, more in (("measured", {}), ("plan", {"spx.gpu.unit_windows": "true"}),
                      ("no-plan", {"spx.gpu.unit_windows": "false"})):
        A = tune(mat[0], dict(NOSAMPLE, **more))
        files[key] = str(d / (key + ".spx"))
        A.save(files[key])
        windows[key] = A.info().unit_windows        # (what the launch tuner settled on goes into the file)
        A.destroy()
    sx.options_reset()
    assert windows["plan"] == 1 and windows["no-plan"] == 0
    return mat, files, windows


@pytest.mark.parametrize("tw", ["false", "true", "auto"])
def test_restored_matrix_reads_the_option_at_restore_time(shared, saved_cant, tw):
    """spx.gpu.trans_windows is read where the device copy is built: a file restored under each value adds the way
    THAT value says, and multiplies right.  A restored matrix plans the unit windows only where its forward product
    was saved with them on (a tuned one always plans them unless told not to): the file of the default tune holds
    them or not by what the launch tuner measured, so the file with spx.gpu.unit_windows=true is the one that shows
    modes 1, 2 and 2; a file without a plan adds per nonzero whatever the option."""
    mat, files, windows = saved_cant
    for key in ("measured", "plan"):
        sx.options_reset()
        sx.option_set(TW, tw)
        B = sx.mat_restore(files[key])
        inf = B.info()
        print("%s restored, trans_windows=%s: mode %d, plan %s, staged %d, window nonzeros %d" % (
            key, tw, B.trans_mode(), "yes" if inf.unit_window_lds else "no", inf.unit_window_staged, inf.unit_window_elems))
        assert (inf.unit_window_lds > 0) == (windows[key] == 1)
        assert B.trans_mode() == expected_mode(B, tw)
        if key == "plan":
            # (cant stages fewer doubles than its windows serve nonzeros: test_auto_counts_atomic_bytes)
            assert B.trans_mode() == (1 if tw == "false" else 2)
        trans_runs(shared, B, mat)
        B.destroy()
    if tw == "true":
        sx.options_reset()
        sx.option_set(TW, tw)
        B = sx.mat_restore(files["no-plan"])
        assert B.info().unit_window_lds == 0 and B.trans_mode() == 1
        trans_runs(shared, B, mat, pairs=mc.ALPHA_BETA[:2])
        B.destroy()
    sx.options_reset()


# ---- 3. symmetric tunes ----------------------------------------------------------------------------------------

SYM_CASES = {
    "tiles": (lambda: synth.syn_nd24k(0.05), NOSAMPLE),
    "segments": (lambda: synth.syn_nlpkkt(20), dict(NOSAMPLE, **{"spx.gpu.sym_segments": "true"})),
    "no-once": (lambda: synth.syn_nlpkkt(20), dict(NOSAMPLE, **{"spx.gpu.sym_once": "false",
                                                                 "spx.gpu.sym_segments": "false"})),
}


@pytest.mark.parametrize("name", list(SYM_CASES))
def test_symmetric_tunes_run_the_forward_product(shared, name):
    torch = shared.torch
    gen, opts = SYM_CASES[name]
    mat = shared.matrix("sym-" + name, _square(gen))
    csr, m = mat[0], mat[1]
    A = shared.load(("sym", name), csr, m, dict(opts, **{TW: "true"}), sym=True)
    assert A.info().symmetric and A.trans_mode() == 0
    n = csr[3]
    xh, xf = shared.x(n)
    y0h = shared.x(n, seed=9)[0]
    for alpha, beta in mc.ALPHA_BETA:
        yf = torch.full((n + PAD,), float("nan"), dtype=torch.float64, device="cuda")
        if beta != 0.0:
            yf[:n] = torch.from_numpy(y0h.copy())
        A.matvec_trans(alpha, xf[2:2 + n], beta, yf[:n])
        torch.cuda.synchronize()
        assert torch.isnan(yf[n:]).all()
        # the forward product's criterion, against the CSR form of A itself
        check_y(csr, xh, yf[:n].cpu().numpy(), alpha, beta, y0h if beta != 0.0 else None)


# ---- 4. the adjoint identity -------------------------------------------------------------------------------------

@pytest.mark.parametrize("tw", ["false", "true"])
def test_adjoint_identity(shared, tw):
    """|<A x, z> - <x, A^T z>| <= sum_i bound(A x)_i |z_i| + sum_j bound(A^T z)_j |x_j|, the fp64 bounds of the two
    products (64 * 2^-53 * |A||x| and 64 * 2^-53 * |A^T||z|); the inner products in extended precision."""
    torch = shared.torch
    A, (csr, m, mt, csr_t) = shared.case("band-wide", tw)
    nr, nc = m.shape
    xh, xf = shared.x(nc)
    zh, zf = shared.x(nr, seed=7)
    ax = torch.full((nr,), float("nan"), dtype=torch.float64, device="cuda")
    atz = torch.full((nc,), float("nan"), dtype=torch.float64, device="cuda")
    A.hip_matvec_mult(1.0, xf[2:2 + nc].data_ptr(), ax.data_ptr(), torch.cuda.current_stream().cuda_stream)
    A.matvec_trans(1.0, zf[2:2 + nr], 0.0, atz)
    torch.cuda.synchronize()
    ld = np.longdouble
    lhs = np.dot(ax.cpu().numpy().astype(ld), zh.astype(ld))
    rhs = np.dot(xh.astype(ld), atz.cpu().numpy().astype(ld))
    eps = FP64_BOUND_FACTOR * 2.0 ** -53
    bound = eps * float(np.abs(zh) @ (abs(m) @ np.abs(xh))) + eps * float(np.abs(xh) @ (abs(mt) @ np.abs(zh)))
    print("adjoint identity: |lhs - rhs| = %.3e, bound %.3e" % (float(abs(lhs - rhs)), bound))
    assert float(abs(lhs - rhs)) <= bound


# ---- 5. row slices ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tw", ["false", "true"])
def test_row_slices_sum_to_the_whole(shared, tw):
    """Two general halves of one matrix, tuned in one process: each reads its own rows of the full-length x and
    leaves a partial vector over all columns; their sum is the transposed product of the whole matrix."""
    torch = shared.torch
    mat = shared.matrix("nlpkkt", CASES["nlpkkt"][0])
    csr, m, mt, csr_t = mat
    n = csr[3]
    opts = dict(NOSAMPLE, **{"spx.gpu.waves": "4", "spx.gpu.wave_tiles": "false", TW: tw})
    halves = []
    for rank in range(2):
        key = ("slice", rank, tw)
        if key not in shared.tuned:
            shared.tuned[key] = dc.tune_rank(csr, rank, 2, opts)
        halves.append(shared.tuned[key])
    infs = [h.info() for h in halves]
    assert infs[0].row_lo == 0 and infs[0].row_hi == infs[1].row_lo and infs[1].row_hi == n
    assert 0 < infs[0].row_hi < n
    assert all(h.trans_mode() == expected_mode(h, tw) for h in halves)
    xh, xf = shared.x(n)
    y0h = shared.x(n, seed=9)[0]
    for alpha, beta in mc.ALPHA_BETA:
        parts = []
        for rank, h in enumerate(halves):
            yf = torch.full((n + PAD,), float("nan"), dtype=torch.float64, device="cuda")
            b = beta if rank == 0 else 0.0             # (beta * y enters the sum once)
            if b != 0.0:
                yf[:n] = torch.from_numpy(y0h.copy())
            h.matvec_trans(alpha, xf[2:2 + n], b, yf[:n])
            torch.cuda.synchronize()
            assert torch.isnan(yf[n:]).all()
            parts.append(yf[:n].cpu().numpy())
        mc.check_y_rect(mt, csr_t, xh, parts[0] + parts[1], alpha, beta, y0h if beta != 0.0 else None)
    # a slice reads nothing of x outside its own rows
    lo, hi = infs[1].row_lo, infs[1].row_hi
    xn = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    xn[lo:hi] = xf[2 + lo:2 + hi]
    y = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    halves[1].matvec_trans(1.0, xn, 0.0, y)
    torch.cuda.synchronize()
    assert not torch.isnan(y).any()


# ---- 6. argument failures ----------------------------------------------------------------------------------------

def test_argument_failures(shared):
    torch = shared.torch
    A, (csr, m, mt, csr_t) = shared.case("band-wide", "true")
    nr, nc = m.shape
    L = sx.lib()
    st = torch.cuda.current_stream().cuda_stream
    buf = torch.zeros(nr + nc, dtype=torch.float64, device="cuda")
    x, y = buf[:nr], buf[nr:]
    assert L.spx_hip_matvec_trans_kernel(1.0, A.handle, x.data_ptr(), 0.0, y.data_ptr(), st) == sx.SPX_SUCCESS
    assert L.spx_hip_matvec_trans_kernel(1.0, None, x.data_ptr(), 0.0, y.data_ptr(), st) == sx.SPX_FAILURE
    assert L.spx_hip_matvec_trans_kernel(1.0, A.handle, None, 0.0, y.data_ptr(), st) == sx.SPX_FAILURE
    assert L.spx_hip_matvec_trans_kernel(1.0, A.handle, x.data_ptr(), 0.0, None, st) == sx.SPX_FAILURE
    assert L.spx_hip_matvec_trans_mult(1.0, A.handle, x.data_ptr(), None, st) == sx.SPX_FAILURE
    # overlap: y starts on the last element of x / x starts on the last element of y / the same vector
    torch.cuda.synchronize()
    buf.fill_(1.0)
    for xp, yp in ((buf[:nr].data_ptr(), buf[nr - 1:].data_ptr()), (buf[nc - 1:].data_ptr(), buf[:nc].data_ptr()),
                   (buf.data_ptr(), buf.data_ptr())):
        assert L.spx_hip_matvec_trans_kernel(1.0, A.handle, xp, 0.0, yp, st) == sx.SPX_FAILURE
        with pytest.raises(sx.SpxError):
            A.hip_matvec_trans_kernel(1.0, xp, 0.0, yp, st)
    torch.cuda.synchronize()
    assert bool((buf == 1.0).all()), "a refused call wrote"
    # device vectors of the wrong length: the forward product's lengths, and one element off
    good_x, good_y = sx.DeviceVector(nr), sx.DeviceVector(nc)
    sx.matvec_trans_kernel_vec(A, 1.0, good_x, 0.0, good_y)
    for bx, by in ((sx.DeviceVector(nc), sx.DeviceVector(nr)), (sx.DeviceVector(nr + 1), good_y),
                   (good_x, sx.DeviceVector(nc - 1))):
        with pytest.raises(sx.SpxError):
            sx.matvec_trans_kernel_vec(A, 1.0, bx, 0.0, by)
    torch.cuda.synchronize()


# ---- 7. graph capture ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tw", ["false", "true"])
def test_captured_product_follows_x(shared, tw):
    torch = shared.torch
    A, (csr, m, mt, csr_t) = shared.case("cant", tw)
    n = csr[3]
    x = torch.from_numpy(synth.random_x(n, seed=21)).cuda()
    y = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    A.matvec_trans(0.5, x, 0.0, y)                                    # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        A.hip_matvec_trans_kernel(0.5, x.data_ptr(), 0.0, y.data_ptr(), torch.cuda.current_stream().cuda_stream)
    for seed in (22, 23):
        xh = synth.random_x(n, seed=seed)
        x.copy_(torch.from_numpy(xh))
        y.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        check_y(csr_t, xh, y.cpu().numpy(), 0.5)


# ---- 8. set_entry --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tw", ["false", "true"])
def test_set_entry_is_seen(shared, tw):
    torch = shared.torch
    csr, m, _, _ = shared.matrix("cant", CASES["cant"][0])
    n = csr[3]
    A = tune(csr, dict(NOSAMPLE, **{TW: tw}))
    xh, xf = shared.x(n)
    y = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    A.matvec_trans(1.0, xf[2:2 + n], 0.0, y)                          # a product is in flight before the edit
    r = n // 2
    c = int(m.indices[m.indptr[r]])                                   # the first nonzero of a middle row
    assert A.get_entry(r, c) == m[r, c]
    A.set_entry(r, c, 1000.0)
    m2 = m.copy()
    m2[r, c] = 1000.0
    m2t = sp.csr_matrix(m2).T.tocsr()
    m2t.sort_indices()
    y.fill_(float("nan"))
    A.matvec_trans(1.0, xf[2:2 + n], 0.0, y)
    torch.cuda.synchronize()
    yh = y.cpu().numpy()
    check_y((m2t.indptr, m2t.indices, m2t.data, n), xh, yh, 1.0)
    assert abs(yh[c] - (m.T.tocsr() @ xh)[c]) > 1.0                    # (the old value would have passed nowhere near)
    A.destroy()


# ---- 9. the forward product's state ----------------------------------------------------------------------------------

def test_forward_product_unchanged_by_a_transposed_one(shared):
    """spx.gpu.deterministic: the forward product is bit-identical before and after a transposed one (which is
    not covered by the option, and touches nothing the forward product keeps)."""
    torch = shared.torch
    mat = shared.matrix("long-rows", CASES["long-rows"][0])
    csr, m, mt, csr_t = mat
    n = csr[3]
    A = shared.load(("long-rows", "det"), csr, m, dict(NOSAMPLE, **{"spx.gpu.deterministic": "true"}))
    assert A.trans_mode() == 1 and A.info().n_shared_rows > 0
    xh, xf = shared.x(n)
    st = torch.cuda.current_stream().cuda_stream
    y1 = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    y2 = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    A.hip_matvec_mult(0.5, xf[2:2 + n].data_ptr(), y1.data_ptr(), st)
    trans_runs(shared, A, mat, pairs=mc.ALPHA_BETA[:2])
    A.hip_matvec_mult(0.5, xf[2:2 + n].data_ptr(), y2.data_ptr(), st)
    torch.cuda.synchronize()
    assert torch.equal(y1, y2)
    check_y(csr, xh, y2.cpu().numpy(), 0.5)
