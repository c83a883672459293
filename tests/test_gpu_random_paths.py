"""The randomised streams of test_stream_random.py and the zoo of test_stream_layout.py (random_cases.py) through the
GPU entry points that came after the forward product: the transposed product (csx_spmv_t_kernel), the product with
the float copy of the values (csx_spmv_*_f32_kernel, csx_spmv_xw_f32_kernel), the bulk value refresh
(csx_refresh_values_kernel, fp64 and fp64 + f32) in front of every product, and the K-vector product on read-once
symmetric streams (csx_spmv_mvsym_kernel, spx.gpu.sym_matmat).  test_random_cases.py proves on the CPU that these
streams hold what this file counts on: every unit kind with small steps in the zoo sweep, window plans, read-once
passes that serve a group, segments without a slot.

One tune per case, every path on that handle (the handles are shared per module).  The vectors live in NaN-padded
tensors, y starts as NaN where beta == 0, padding and x are checked for writes: the helpers are those of
test_gpu_transpose.py (trans_runs), test_gpu_values_f32.py (f32_runs, assert_reads_floats) and matmat_cases.py
(run).  The references and tolerances are the project's own: helpers.check_y / matmat_cases.check_y_rect against the
CSR product (of the transposed matrix; of the values rounded to float), relative 1e-6 and 64 * 2^-53 * |A||x|."""
import numpy as np
import pytest
import scipy.sparse as sp

import sparsex_amd as sx
from helpers import check_y, tune
import matmat_cases as mc
import random_cases as rc
import values_cases as vc
import test_gpu_transpose as tt
import test_gpu_values_f32 as tf
from stream_decode import Stream

pytestmark = pytest.mark.gpu

PAD = tt.PAD
TW, UW = "spx.gpu.trans_windows", "spx.gpu.unit_windows"
# the zoo under (trans_windows, unit_windows, waves): per-nonzero adds and LDS windows over a plan, and -- without the
# plan, where the plain float kernels run -- the transposed product that asks for windows and finds none
ZOO_VARIANTS = (("false", "true", 4), ("true", "true", 2), ("true", "false", 8))
GENERAL_CASES = [("seed", s) for s in rc.GENERAL_SEEDS] + \
                [("zoo", x, v) for x in rc.ZOO_XFORMS for v in range(len(ZOO_VARIANTS))]


def case_id(case):
    if case[0] == "seed":
        return "seed-%d" % case[1]
    return "zoo-%s-tw_%s-uw_%s" % ((case[1],) + ZOO_VARIANTS[case[2]][:2])


class Case:
    """A tuned handle and its references: the matrix, its transpose, its float-rounded twin."""

    def __init__(self, name, csr, m, opts, sym=False):
        self.name, self.csr, self.opts, self.sym = name, csr, opts, sym
        self.m = sp.csr_matrix(m)
        self.m.sort_indices()
        self.A = mc.load_rect(sx, csr, self.m.shape[1], opts) if not sym else tune(csr, opts, sym=True)
        self.inf = self.A.info()
        self.group = self.A.matmat_group()
        self.mode = self.A.trans_mode()
        self.mat_t, self.mat_32 = self.references(csr[2])

    def references(self, values):
        """(what trans_runs takes, what f32_runs takes) for the pattern with `values`"""
        rp, ci, _, n = self.csr
        m = sp.csr_matrix((np.asarray(values), ci, rp), shape=self.m.shape)
        csr = (rp, ci, np.asarray(values), n)
        mt = m.T.tocsr()
        mt.sort_indices()
        m32 = sp.csr_matrix((tf.rounded(m.data), m.indices, m.indptr), shape=m.shape)
        return (csr, m, mt, (mt.indptr, mt.indices, mt.data, mt.shape[0])), \
               (csr, m, m32, (m32.indptr, m32.indices, m32.data, m32.shape[0]))

    def family(self):
        inf = self.inf
        if inf.symmetric:
            return "sym"
        return "accum" if inf.col_slices > 1 else "det" if inf.wave_tiles else "xw" if inf.unit_windows else "plain"

    def line(self):
        inf = self.inf
        return "%s: %s | %s, waves %d, %d row-blocks, window plan %s, trans_mode %d, group %d" % (
            self.name, " ".join("%s=%s" % (k.split(".", 1)[1], v) for k, v in sorted(self.opts.items())), self.family(),
            inf.waves, inf.n_rowblocks, "yes" if inf.unit_window_lds else "no", self.mode, self.group)


class Shared(tt.Shared):
    """test_gpu_transpose.Shared (the vectors trans_runs and f32_runs ask for) and the cases, tuned once each"""

    def __init__(self, torch):
        super().__init__(torch)
        self.cases = {}

    def case(self, case):
        if case not in self.cases:
            if case[0] == "seed":
                seed = case[1]
                csr, m = rc.general_matrix(seed)
                c = Case(case_id(case), csr, m, rc.general_options(seed))
                c.tw, c.seed = rc.TRANS_WINDOWS[seed % 3], seed
            elif case[0] == "zoo":
                tw, uw, waves = ZOO_VARIANTS[case[2]]
                csr, m = self.matrix("zoo", rc.zoo_matrix)[:2]
                c = Case(case_id(case), csr, m, rc.zoo_options(case[1], {TW: tw, UW: uw, "spx.gpu.waves": str(waves)}))
                c.tw, c.seed = tw, 100 + 3 * rc.ZOO_XFORMS.index(case[1]) + case[2]
            else:
                seed = case[1]
                csr, m = rc.random_matrix(seed, symmetric=True)
                c = Case("sym-seed-%d" % seed, csr, m, rc.sym_matmat_options(seed), sym=True)
                c.seed = seed
            print(c.line())
            self.cases[case] = c
        return self.cases[case]


@pytest.fixture(scope="module")
def shared():
    import torch
    s = Shared(torch)
    yield s
    for c in s.cases.values():
        c.A.destroy()
    s.cases.clear()
    s.mats.clear()
    s.xs.clear()
    sx.options_reset()
    torch.cuda.empty_cache()


def forward(shared, c, mat, alpha=0.5):
    """the fp64 product (beta == 0 over a y of NaN) against the CSR arrays of mat"""
    csr, m = mat[0], mat[1]
    nr, nc = m.shape
    y = tf.f64_product(shared, c.A, nc, nr, alpha)
    mc.check_y_rect(m, csr, shared.x(nc)[0], y.cpu().numpy(), alpha, 0.0, None)
    return y


# ---- general streams: seeds 0 .. 39 and the zoo sweep ------------------------------------------------------------------

@pytest.mark.parametrize("case", GENERAL_CASES, ids=case_id)
def test_transposed_product(shared, case):
    """a. against the CSR product of a.T, and the mode against what the option and the plan imply"""
    c = shared.case(case)
    assert not c.inf.symmetric
    assert c.mode == tt.expected_mode(c.A, c.tw)
    tt.trans_runs(shared, c.A, c.mat_t)


@pytest.mark.parametrize("case", GENERAL_CASES, ids=case_id)
def test_float_product(shared, case, tmp_path):
    """b. against the CSR product of fl32(A), beyond the fp64 bound of A's own product (the floats were read).
    spx.gpu.deterministic: two float products are bit-identical, and the fp64 product is that of the same stream
    without the copy -- restored from the saved file, and tuned again where the launch settings are pinned (a tune
    that leaves the wavefront count to the measurement may settle on another one, with another order of the sums)."""
    torch = shared.torch
    c = shared.case(case)
    A = c.A
    assert A.values_f32_bytes() == 4 * tf.stream_values(A) > 0
    tf.f32_runs(shared, A, c.mat_32, what=c.name)
    if c.opts.get("spx.gpu.deterministic") != "true":
        return
    nr, nc = c.m.shape
    xh, xf = shared.x(nc)
    ys = []
    for _ in range(2):
        y = torch.full((nr,), float("nan"), dtype=torch.float64, device="cuda")
        A.matvec_f32(0.5, xf[2:2 + nc], 0.0, y)
        ys.append(y)
    y1 = forward(shared, c, c.mat_t)
    torch.cuda.synchronize()
    assert torch.equal(ys[0], ys[1]), "two float products differ"
    f = str(tmp_path / "det.spx")
    A.save(f)
    sx.options_reset()
    B = sx.mat_restore(f)
    tf.assert_no_copy(shared, B)
    assert torch.equal(tf.f64_product(shared, B, nc, nr), y1), "the fp64 product changed with the copy (restored twin)"
    B.destroy()
    o = dict(c.opts)
    del o["spx.gpu.values_f32"]
    pinned = o["spx.gpu.waves"] != "0"
    T = mc.load_rect(sx, c.csr, nc, o)
    tf.assert_no_copy(shared, T)
    ti = T.info()
    same = (ti.waves, ti.n_rowblocks, ti.wave_tiles) == (c.inf.waves, c.inf.n_rowblocks, c.inf.wave_tiles)
    assert same or not pinned
    if same:
        assert torch.equal(tf.f64_product(shared, T, nc, nr), y1), "the fp64 product changed with the copy (tuned twin)"
    else:
        print("%s: the twin without the copy settled on waves %d, %d row-blocks (with: %d, %d)" % (
            c.name, ti.waves, ti.n_rowblocks, c.inf.waves, c.inf.n_rowblocks))
    T.destroy()


@pytest.mark.parametrize("case", GENERAL_CASES, ids=case_id)
def test_value_refresh(shared, case):
    """c. new values from a device array (values_cases.new_values: another value at every position), then every
    product against them; the tuned values again from a host array"""
    torch = shared.torch
    c = shared.case(case)
    A, csr = c.A, c.csr
    A.values_plan(csr[0], csr[1])
    v = vc.new_values(csr, False, c.seed)
    A.set_values(torch.from_numpy(v.copy()).cuda())
    new_t, new_32 = c.references(v)
    try:
        forward(shared, c, new_t)
        mc.run(torch, A, new_t[1], 3, 2.0, -0.5, padx=PAD, pady=PAD)
        tt.trans_runs(shared, A, new_t, pairs=mc.ALPHA_BETA[:2])
        tf.f32_runs(shared, A, new_32, pairs=mc.ALPHA_BETA[:2], what=c.name + " after set_values")
    finally:
        A.set_values(np.array(csr[2]))
    forward(shared, c, c.mat_t)
    tf.f32_runs(shared, A, c.mat_32, pairs=mc.ALPHA_BETA[:1], what=c.name + ", the tuned values again")
    A.values_plan_drop()


def test_general_cases_cover_the_paths(shared):
    """What the cases above ran, from what their handles report: both ways of adding of the transposed product on
    ten seeds each, the float kernels with and without unit windows and with a y tile per wavefront, 2, 4 and 8
    wavefronts, a rectangular matrix with a window plan.  (Where the tuner's choices leave one short, pin the
    option by seed in random_cases.general_options.)"""
    modes, uw, wt, waves, rect_plan, fam = {1: [], 2: []}, set(), set(), set(), [], {}
    for case in GENERAL_CASES:
        c = shared.case(case)
        fam.setdefault(c.family(), []).append(c.name)
        uw.add(int(c.inf.unit_windows))
        wt.add(int(c.inf.wave_tiles))
        waves.add(int(c.inf.waves))
        if case[0] == "seed":
            modes[c.mode].append(case[1])
            if rc.is_rect(case[1]) and c.inf.unit_window_lds > 0:
                rect_plan.append(case[1])
    print("trans_mode 1: %d seeds %s\ntrans_mode 2: %d seeds %s" % (len(modes[1]), modes[1], len(modes[2]), modes[2]))
    print("unit_windows %s, wave_tiles %s, waves %s, rectangular with a plan %s" % (
        sorted(uw), sorted(wt), sorted(waves), rect_plan))
    print("kernel families: %s" % {k: len(v) for k, v in sorted(fam.items())})
    assert len(modes[1]) >= 10 and len(modes[2]) >= 10
    assert uw == {0, 1}
    assert 1 in wt
    assert {2, 4, 8} <= waves
    assert rect_plan


# ---- symmetric streams under spx.gpu.sym_matmat: seeds 40 .. 89 ----------------------------------------------------------

SYM_CASES = [("sym", s) for s in rc.SYM_SEEDS]


def sym_id(case):
    return "seed-%d" % case[1]


def device_census(c, tmp_path):
    """the census of the stream the device copy holds (the launch tuner may have emitted it again), once per case"""
    if not hasattr(c, "census"):
        c.census = rc.census(c.A, str(tmp_path / "device.spx"), windows=False)
        c.census.pop("stream")
    return c.census


@pytest.mark.parametrize("case", SYM_CASES, ids=sym_id)
def test_symmetric_matmat(shared, case, tmp_path):
    """d. 13 = 8 + 4 + 1 vectors; the group the device serves against the independent restatement on the saved
    stream (random_cases.expected_group).  With read-once passes and a group >= 2, csx_spmv_mvsym_kernel ran."""
    torch = shared.torch
    c = shared.case(case)
    seed = case[1]
    cen = device_census(c, tmp_path)
    print("%s: read-once passes %s, group %d%s" % (c.name, "yes" if rc.has_read_once(cen) else "no", c.group,
                                                   " (csx_spmv_mvsym_kernel)" if rc.has_read_once(cen) and c.group >= 2 else ""))
    assert c.inf.symmetric
    assert c.group == rc.expected_group(cen, c.inf)
    alpha, beta = mc.ALPHA_BETA[seed % 3]
    mc.run(torch, c.A, c.m, rc.NVEC_SYM, alpha, beta, padx=1 + seed % 4, pady=2 + seed % 3)


@pytest.mark.parametrize("case", SYM_CASES, ids=sym_id)
def test_symmetric_handle_runs_the_forward_product_for_the_transposed(shared, case):
    """f. matvec_trans on a symmetric handle, against the CSR form of A itself"""
    torch = shared.torch
    c = shared.case(case)
    assert c.mode == 0
    n = c.csr[3]
    xh, xf = shared.x(n)
    y0h = shared.x(n, seed=9)[0]
    for alpha, beta in mc.ALPHA_BETA:
        yf = torch.full((n + PAD,), float("nan"), dtype=torch.float64, device="cuda")
        if beta != 0.0:
            yf[:n] = torch.from_numpy(y0h.copy())
        c.A.matvec_trans(alpha, xf[2:2 + n], beta, yf[:n])
        torch.cuda.synchronize()
        assert torch.isnan(yf[n:]).all()
        assert torch.isnan(xf[:2]).all() and torch.isnan(xf[2 + n:]).all()
        check_y(c.csr, xh, yf[:n].cpu().numpy(), alpha, beta, y0h if beta != 0.0 else None)


@pytest.mark.parametrize("case", SYM_CASES, ids=sym_id)
def test_symmetric_value_refresh(shared, case):
    """e. new symmetric values from a device array, then five vectors at once and the single-vector product
    against them; the tuned values again from a host array"""
    torch = shared.torch
    c = shared.case(case)
    A, csr, seed = c.A, c.csr, case[1]
    A.values_plan(csr[0], csr[1])
    v = vc.new_values(csr, True, seed)
    A.set_values(torch.from_numpy(v.copy()).cuda())
    new = c.references(v)[0]
    try:
        alpha, beta = mc.ALPHA_BETA[(seed + 1) % 3]
        mc.run(torch, A, new[1], 5, alpha, beta, padx=seed % 3, pady=1 + seed % 2)
        forward(shared, c, new)
    finally:
        A.set_values(np.array(csr[2]))
    forward(shared, c, c.mat_t)
    A.values_plan_drop()


def test_symmetric_cases_ran_the_k_vector_kernel(shared, tmp_path):
    """at least 15 seeds hold read-once passes and ran with a group >= 2: the count of test_random_cases.py, against
    what the device reported"""
    ran = []
    for case in SYM_CASES:
        c = shared.case(case)
        if rc.has_read_once(device_census(c, tmp_path)) and c.group >= 2:
            ran.append((case[1], c.group))
    print("read-once passes and a group >= 2: %d seeds, (seed, group) %s" % (len(ran), ran))
    assert len(ran) >= 15
