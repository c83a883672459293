"""Row slices on the GPU, in one process and without a transport: every case of dist_cases.py, rank by rank,
through every kernel family -- spx_hip_matvec_kernel, spx_hip_matmat_kernel and spx_hip_matvec_parts against the
float64 references of dist_cases.py (rows [lo, hi) of the product on the general path, the partial vector of an
unattached slice on the symmetric one), with (alpha, beta) = limit_cases.ALPHA_BETA and with beta = 0 over a y
of NaN.  y0 holds NaN outside the rank's own rows: a general slice must leave those bit patterns alone, a
symmetric one must not read them.  test_dist_cases.py proves on the CPU what each case holds."""
import numpy as np
import pytest

import sparsex_amd as sx
from sparsex_amd import synth
import dist_cases as dc
from stream_decode import Stream

pytestmark = pytest.mark.gpu

PADX, PADY, NVEC = 3, 5, 5
A_, B_ = dc.ALPHA_BETA
RUNS = ((A_, B_), (0.5, 0.0))


class Case:
    """What the tests of one case share: the matrix, its cut, x (NVEC vectors; on the device with NaN behind
    each), the part matrix of every rank and the references, computed once and never written again."""

    def __init__(self, torch, name):
        self.name = name
        self.csr = dc.matrix(name)
        self.n = self.csr[3]
        self.m = dc.to_scipy(self.csr)
        self.cuts = dc.bounds(name, self.csr)
        self.world = len(self.cuts) - 1
        self.xh = np.stack([synth.random_x(self.n, seed=5 + j) for j in range(NVEC)])
        self.xf = torch.full((NVEC, self.n + PADX), float("nan"), dtype=torch.float64, device="cuda")
        self.xf[:, :self.n] = torch.from_numpy(self.xh)
        self._parts, self._refs, self._y0 = {}, {}, {}

    def rows(self, rank):
        return self.cuts[rank], self.cuts[rank + 1]

    def part(self, sym, lo, hi):
        if (sym, lo, hi) not in self._parts:
            self._parts[(sym, lo, hi)] = (dc.symmetric_part if sym else dc.general_part)(self.m, lo, hi)
        return self._parts[(sym, lo, hi)]

    def y0(self, lo, hi, j):
        if (lo, hi, j) not in self._y0:
            self._y0[(lo, hi, j)] = dc.nan_outside(self.n, lo, hi, seed=100 + j)
        return self._y0[(lo, hi, j)]

    def ref(self, sym, lo, hi, j, alpha, beta):
        key = (sym, lo, hi, j, alpha, beta)
        if key not in self._refs:
            r = dc.reference(self.part(sym, lo, hi), lo, hi, self.xh[j], alpha, beta, self.y0(lo, hi, j))
            for a in r:
                a.setflags(write=False)
            self._refs[key] = r
        return self._refs[key]


@pytest.fixture(scope="module")
def cases():
    import torch
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Case(torch, name)
        return cache[name]
    yield get
    cache.clear()
    sx.options_reset()
    torch.cuda.empty_cache()


def check_family(A, family, sym):
    """The family named is the one that runs (as test_gpu_stream_limits does, through info())."""
    inf = A.info()
    assert inf.on_device and inf.waves == int(dc.WAVES)
    if not sym:
        assert not inf.symmetric
        assert bool(inf.wave_tiles) == (family == "det")
        # (a slice of one row may hold nothing for a second column slice: it then stays uncut)
        want = {"slices-c2": 2, "slices-2": -2}.get(family, 1)
        assert inf.col_slices == want or (inf.row_hi - inf.row_lo == 1 and inf.col_slices == 1)
        if family == "unit-windows":
            # (csx_spmv_xw_kernel runs where the plan stages a window for a row-block: not in a slice of one row)
            assert inf.unit_windows == (1 if A.unit_windows(3072, 16)["rowblocks_with_windows"] > 0 else 0)
        else:
            assert inf.unit_windows == 0
        return inf
    assert inf.symmetric
    _, _, cnt = A.sym_pipeline()
    print("rows [%d, %d): sym_tiles %d, sym_segments %d, sym_pipeline %d (%d SX passes), wave_tiles %d" % (
        inf.row_lo, inf.row_hi, inf.sym_tiles, inf.sym_segments, inf.sym_pipeline, cnt["sx_passes"], inf.wave_tiles))
    if family in ("lists", "atomic"):
        assert inf.sym_segments == 0 and inf.sym_tiles in (0, 1 if family == "lists" else 2)
    if family in ("segments", "pipeline"):
        assert inf.sym_tiles in (0, 2)               # (read-once segments imply the atomic hand-over)
        # (csx_spmv_sx_kernel: streams of read-once segments without dense tiles -- sym_segments == 2 -- whose plan
        # holds a pass for it)
        assert inf.sym_pipeline == (1 if family == "pipeline" and cnt["sx_passes"] > 0 and inf.sym_segments == 2 else 0)
    else:
        assert inf.sym_pipeline == 0
    assert bool(inf.wave_tiles) == (family == "det")
    return inf


def check(c, sym, lo, hi, j, alpha, beta, y, what):
    """One column against the reference; the rows a slice must not write."""
    ref, bound = c.ref(sym, lo, hi, j, alpha, beta)
    r = dc.max_ratio(y, ref, bound, slice(0, hi) if sym else slice(lo, hi))
    print("%s rows [%d, %d) column %d alpha %g beta %g: max error / bound %.3g" % (what, lo, hi, j, alpha, beta, r))
    assert r <= 1.0, "%s: max error / bound %g" % (what, r)
    if sym:
        assert np.array_equal(y[hi:], np.zeros(c.n - hi)), "%s: rows at or behind hi are not 0" % what
    return ref, bound


def start_y(torch, c, lo, hi, nvec, beta):
    """(nvec, n + PADY) of NaN; beta != 0: the ranks' own y0 on the rows [lo, hi)"""
    yf = torch.full((nvec, c.n + PADY), float("nan"), dtype=torch.float64, device="cuda")
    if beta != 0.0:
        for j in range(nvec):
            yf[j, :c.n] = torch.from_numpy(c.y0(lo, hi, j))
    return yf


def untouched(c, sym, lo, hi, before, after, what):
    """General slices: every row outside [lo, hi) keeps its bit pattern.  Both: so does the padding."""
    assert np.array_equal(dc.bits(before[:, c.n:]), dc.bits(after[:, c.n:])), "%s: the padding was written" % what
    if not sym:
        for s in (slice(0, lo), slice(hi, c.n)):
            assert np.array_equal(dc.bits(before[:, s]), dc.bits(after[:, s])), "%s: rows outside [lo, hi) were written" % what


def products(torch, c, A, sym, lo, hi):
    """spx_hip_matvec_kernel and spx_hip_matmat_kernel (NVEC vectors, padded, NaN in the padding) with both
    (alpha, beta); returns the single products on the host, {(alpha, beta): y}."""
    st = torch.cuda.current_stream().cuda_stream
    out = {}
    for alpha, beta in RUNS:
        yf = start_y(torch, c, lo, hi, 1, beta)
        before = yf.cpu().numpy()
        A.hip_matvec_kernel(alpha, c.xf[0].data_ptr(), beta, yf.data_ptr(), st)
        torch.cuda.synchronize()
        after = yf.cpu().numpy()
        check(c, sym, lo, hi, 0, alpha, beta, after[0, :c.n], "matvec")
        untouched(c, sym, lo, hi, before, after, "matvec")
        out[(alpha, beta)] = after[0, :c.n].copy()
        Yf = start_y(torch, c, lo, hi, NVEC, beta)
        before = Yf.cpu().numpy()
        A.hip_matmat_kernel(alpha, c.xf.data_ptr(), c.n + PADX, NVEC, beta, Yf.data_ptr(), c.n + PADY, st)
        torch.cuda.synchronize()
        after = Yf.cpu().numpy()
        for j in range(NVEC):
            check(c, sym, lo, hi, j, alpha, beta, after[j, :c.n], "matmat")
        untouched(c, sym, lo, hi, before, after, "matmat")
    assert torch.isnan(c.xf[:, c.n:]).all()
    return out


def check_sum(c, sym, ys):
    """The ranks' vectors summed on the host (general: the rows of each, the others counted as 0) against the
    full product, within the sum of the ranks' bounds."""
    for alpha, beta in RUNS:
        total, ref, bound = np.zeros(c.n), np.zeros(c.n), np.zeros(c.n)
        for r in range(c.world):
            lo, hi = c.rows(r)
            y = ys[r][(alpha, beta)]
            rr, bb = c.ref(sym, lo, hi, 0, alpha, beta)
            if sym:
                total += y
                ref += rr
                bound += bb
            else:
                total[lo:hi] += y[lo:hi]
                ref[lo:hi] += rr[lo:hi]
                bound[lo:hi] += bb[lo:hi]
        # (the references of the parts sum to the product of the whole: test_dist_cases.py)
        full = alpha * (c.m @ c.xh[0])
        if beta != 0.0:
            for r in range(c.world):
                lo, hi = c.rows(r)
                full[lo:hi] += beta * c.y0(lo, hi, 0)[lo:hi]
        ratio = dc.max_ratio(total, full, bound + 4 * 2.0 ** -53 * np.abs(full))
        assert ratio <= 1.0, "sum over the ranks: max error / bound %g" % ratio


@pytest.mark.parametrize("case,family", dc.pairs(False))
def test_general_slices(cases, case, family):
    """Rows [lo, hi) of alpha*A*x + beta*y0, everything else untouched; in three launches
    (spx_hip_matvec_parts) where the slice has the row-blocks for it."""
    import torch
    c = cases(case)
    st = torch.cuda.current_stream().cuda_stream
    ys = []
    for rank in range(c.world):
        lo, hi = c.rows(rank)
        A = dc.tune_rows(c.csr, lo, hi, dc.family_options(case, family, False))
        inf = check_family(A, family, False)
        assert (inf.row_lo, inf.row_hi) == (lo, hi) and A.nrows == c.n
        ys.append(products(torch, c, A, False, lo, hi))
        if case in dc.OVERLAP:
            assert inf.n_rowblocks >= 64
            for alpha, beta in RUNS:
                yf = start_y(torch, c, lo, hi, 1, beta)
                before = yf.cpu().numpy()
                launched = A.hip_matvec_parts(alpha, c.xf[0].data_ptr(), beta, yf.data_ptr(), 3, st)
                torch.cuda.synchronize()
                after = yf.cpu().numpy()
                assert launched >= 2, "the product ran in %d launch(es)" % launched
                check(c, False, lo, hi, 0, alpha, beta, after[0, :c.n], "parts")
                untouched(c, False, lo, hi, before, after, "parts")
        A.destroy()
    check_sum(c, False, ys)


@pytest.mark.parametrize("case,family", dc.pairs(True))
def test_symmetric_slices(cases, case, family):
    """The partial vector of an unattached slice: its lower triangle and diagonal on the owned rows (with the beta
    term, there only), the mirror image in front, exactly 0 at and behind hi; the ranks' vectors sum to the
    product."""
    import torch
    c = cases(case)
    ys = []
    seen = {"segments": 0, "pipeline": 0, "tiles": 0}
    for rank in range(c.world):
        lo, hi = c.rows(rank)
        A = dc.tune_rows(c.csr, lo, hi, dc.family_options(case, family, True), symmetric=True)
        inf = check_family(A, family, True)
        assert (inf.row_lo, inf.row_hi) == (lo, hi) and A.nrows == c.n
        seen["segments"] += inf.sym_segments > 0
        seen["pipeline"] += inf.sym_pipeline
        seen["tiles"] += inf.sym_tiles > 0
        ys.append(products(torch, c, A, True, lo, hi))
        A.destroy()
    if family in ("segments", "pipeline"):
        assert seen["segments"] > 0
    if family == "pipeline" and case in dc.PIPELINED:
        assert seen["pipeline"] > 0
    if family in ("lists", "atomic", "det"):
        assert (seen["tiles"] > 0) == (dc.CASES[case][0] == "nd24k")
    check_sum(c, True, ys)


@pytest.mark.parametrize("symmetric", [False, True], ids=["general", "symmetric"])
@pytest.mark.parametrize("name", ["nlpkkt", "nd24k"])
@pytest.mark.parametrize("world", [2, 3])
def test_both_ways_of_making_a_slice_agree(cases, world, name, symmetric):
    """The whole matrix with spx.rt.gpu_rank / gpu_world (one partition per rank), and the rows the library then
    owns handed over alone (spx.rt.row_offset / global_rows, one partition): the same owned rows, and with
    spx.gpu.deterministic bit-identical products."""
    import torch
    case = next(k for k, v in dc.CASES.items() if v[0] == name)
    c = cases(case)
    st = torch.cuda.current_stream().cuda_stream
    opts = dc.family_options(case, "det", symmetric)
    at = 0
    for rank in range(world):
        A = dc.tune_rank(c.csr, rank, world, opts, symmetric)
        inf = A.info()
        lo, hi = inf.row_lo, inf.row_hi
        assert lo == at and hi > lo and (inf.first_partition, inf.last_partition) == (rank, rank + 1)
        at = hi
        B = dc.tune_rows(c.csr, lo, hi, opts, symmetric, threads=1)
        assert (B.info().row_lo, B.info().row_hi) == (lo, hi)
        for alpha, beta in RUNS:
            got = []
            for M in (A, B):
                yf = start_y(torch, c, lo, hi, 1, beta)
                M.hip_matvec_kernel(alpha, c.xf[0].data_ptr(), beta, yf.data_ptr(), st)
                torch.cuda.synchronize()
                got.append(yf.cpu().numpy())
            ref, bound = dc.reference(c.part(symmetric, lo, hi), lo, hi, c.xh[0], alpha, beta, c.y0(lo, hi, 0))
            r = dc.max_ratio(got[0][0, :c.n], ref, bound, slice(0, hi) if symmetric else slice(lo, hi))
            assert r <= 1.0, "gpu_rank slice: max error / bound %g" % r
            assert np.array_equal(dc.bits(got[0]), dc.bits(got[1])), "the two slices' products differ"
        A.destroy()
        B.destroy()
    assert at == c.n


def test_set_entry_reaches_the_thin_mirror_list(cases, tmp_path):
    """spx_mat_set_entry on an entry whose mirror image lives in the thin mirror list of the last slice
    (device_poke_mirror): both triangles read the new value, and so does the product."""
    import torch
    case = "thin-mirror-w3-balanced"
    c = cases(case)
    st = torch.cuda.current_stream().cuda_stream
    lo, hi = c.rows(c.world - 1)
    rp, ci, va, n = c.csr
    A = dc.tune_rows(c.csr, lo, hi, dc.family_options(case, "lists", True), symmetric=True)
    f = str(tmp_path / "last.spx")
    A.save(f)
    r, col = dc.thin_mirror_entry(c.csr, lo, Stream(f).mirror_rows)
    k = int(rp[r]) + int(np.searchsorted(ci[rp[r]:rp[r + 1]], col))
    assert A.get_entry(r, col) == va[k] and A.get_entry(col, r) == va[k]
    y = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    A.hip_matvec_mult(1.0, c.xf[0].data_ptr(), y.data_ptr(), st)         # (an edit after a product: the batch path)
    torch.cuda.synchronize()
    A.set_entry(r, col, 4.5)
    assert A.get_entry(r, col) == 4.5 and A.get_entry(col, r) == 4.5
    va2 = va.copy()
    va2[k] = 4.5
    va2[rp[col] + int(np.searchsorted(ci[rp[col]:rp[col + 1]], r))] = 4.5
    m2 = dc.to_scipy((rp, ci, va2, n))
    part = dc.symmetric_part(m2, lo, hi)
    for alpha, beta in RUNS:
        yf = start_y(torch, c, lo, hi, 1, beta)
        A.hip_matvec_kernel(alpha, c.xf[0].data_ptr(), beta, yf.data_ptr(), st)
        torch.cuda.synchronize()
        got = yf.cpu().numpy()[0, :n]
        ref, bound = dc.reference(part, lo, hi, c.xh[0], alpha, beta, c.y0(lo, hi, 0))
        ratio = dc.max_ratio(got, ref, bound)
        assert ratio <= 1.0, "after set_entry: max error / bound %g" % ratio
        # the edit is visible at all: the old value misses the bound on the mirrored row
        old, _ = c.ref(True, lo, hi, 0, alpha, beta)
        assert abs(got[col] - old[col]) > bound[col]
    A.destroy()
