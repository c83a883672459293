"""The kernels at the limits of the row-block stream's fields (sparsex_amd/csrc/gpu_format.h): the cases of
limit_cases.py -- column offsets of 16, 24 and 32 bits, steps of 127, up to 8188 segments in front of a unit,
pass counts at the branch points of the pass loop, full sets of transposed-sum slots and lanes without one --
through every kernel family that decodes the field, the multi-vector kernel of the read-once symmetric passes
(spx.gpu.sym_matmat) among them: tuned with the option, and on default-tuned streams restored with it.
test_limit_cases.py proves on the CPU that each tune used here reaches its limit.  Every product is checked with helpers.check_y (matmat_cases.check_y_rect for the
rectangular ones): `mult` on a y of NaN, the alpha / beta kernel, NaN behind x and y on the device."""
import numpy as np
import pytest
import scipy.sparse as sp

import sparsex_amd as sx
from sparsex_amd import synth
from helpers import tune
import limit_cases as lc
import matmat_cases as mc
import matmat_sym_cases as msc
from stream_decode import Stream

pytestmark = pytest.mark.gpu

PADX, PADY = 3, 5


@pytest.fixture(scope="module")
def shared():
    """Matrices by name and x by length (host, and on the device with NaN behind it): generated once."""
    import torch
    mats, xs = {}, {}

    class Shared:
        def matrix(self, name, gen):
            if name not in mats:
                csr, m = gen()
                if m is None:
                    m = mc.to_scipy(csr)
                mats[name] = (csr, m)
            return mats[name]

        def x(self, nc):
            if nc not in xs:
                xh = synth.random_x(nc, seed=5)
                xf = torch.full((nc + PADX,), float("nan"), dtype=torch.float64, device="cuda")
                xf[:nc] = torch.from_numpy(xh)
                xs[nc] = (xh, xf)
            return xs[nc]
    yield Shared()
    mats.clear()
    xs.clear()
    sx.options_reset()
    torch.cuda.empty_cache()


def _load(csr, m, opts, sym=False):
    if m.shape[0] != m.shape[1]:
        return mc.load_rect(sx, csr, m.shape[1], opts)
    return tune(csr, opts, sym=sym)


def _check(m, x, y, alpha, beta=0.0, y0=None):
    mc.check_y_rect(m, (m.indptr, m.indices, m.data, m.shape[0]), x, y, alpha, beta, y0)


def products(torch, shared, A, m, host=True, beta=True, repeat=False):
    """The device entry points on padded vectors: mult into a y of NaN (returned, on the device), then the
    alpha / beta kernel; `host`: spx_matvec_mult on host vectors as well; `repeat`: the product again, bit for
    bit the same."""
    nr, nc = m.shape
    xh, xf = shared.x(nc)
    st = torch.cuda.current_stream().cuda_stream
    yf = torch.full((nr + PADY,), float("nan"), dtype=torch.float64, device="cuda")
    A.hip_matvec_mult(0.5, xf.data_ptr(), yf.data_ptr(), st)
    torch.cuda.synchronize()
    y = yf[:nr].clone()
    _check(m, xh, y.cpu().numpy(), 0.5)
    assert torch.isnan(yf[nr:]).all(), "the padding of y was written"
    if repeat:
        for _ in range(3):
            yf[:nr] = float("nan")
            A.hip_matvec_mult(0.5, xf.data_ptr(), yf.data_ptr(), st)
            torch.cuda.synchronize()
            assert torch.equal(yf[:nr], y), "repeated products differ"
    if beta:
        a_, b_ = lc.ALPHA_BETA
        y0 = synth.random_x(nr, seed=9)
        yf[:nr] = torch.from_numpy(y0)
        A.hip_matvec_kernel(a_, xf.data_ptr(), b_, yf.data_ptr(), st)
        torch.cuda.synchronize()
        _check(m, xh, yf[:nr].cpu().numpy(), a_, b_, y0)
        assert torch.isnan(yf[nr:]).all() and torch.isnan(xf[nc:]).all()
    if host:
        yh = np.full(nr, np.nan)
        A.matvec_mult(0.5, xh, yh)
        _check(m, xh, yh, 0.5)
    return y


# ---- 1. general path: offsets of 16, 24 and 32 bits ---------------------------------------------------------

def _is_big(case):
    return max(lc.OFFSETS[case][0]) > 2 ** 20


@pytest.mark.parametrize("case,family", sorted(lc.OFF_WIDTHS))
def test_general_offsets(shared, case, family):
    """csx_spmv_kernel at 2, 4 and 8 wavefronts ("plain"), csx_spmv_det_kernel, the column slices in one
    launch (csx_spmv_accum_kernel) and in sequence, csx_spmv_xw_kernel.  The vectors of the 2^24 cases are
    134 MB and more: there the alpha / beta kernel runs at 4 wavefronts only, and the host-vector product
    (which goes up in parts, by the columns stream_rowblock_xpieces decodes) once, for "plain"."""
    import torch
    csr, m = shared.matrix(case, lambda: lc.wide_offsets(lc.OFFSETS[case][0]))
    big = _is_big(case)
    for waves in ((2, 4, 8) if family == "plain" else (4,)):
        A = _load(csr, m, lc.off_options(family, waves))
        inf = A.info()
        assert inf.waves == waves
        assert bool(inf.wave_tiles) == (family == "det")
        assert inf.col_slices == {"slices-c2": 2, "slices-2": -2}.get(family, 1)    # (negative: one after the other)
        products(torch, shared, A, m, host=waves == 4 and (not big or family == "plain"),
                 beta=waves == 4 or not big, repeat=family == "det")
        A.destroy()


@pytest.mark.parametrize("case,family,nvecs", [
    ("off-65536", "plain", (2, 4, 8)), ("off-65536", "det", (2, 4, 8)), ("off-2x-65536", "slices-c2", (2, 4, 8)),
    ("off-2p24m1", "plain", (2,)), ("off-2p24", "plain", (2,)), ("off-2p24", "det", (2,)),
])
def test_matmat_offsets(shared, case, family, nvecs):
    """spx_hip_matmat_kernel expands the same SPX_LOAD_INDEX: K = 2, 4, 8 at 24 bits (and K = 2 where all eight
    bits of the high byte are in use), K = 2 at 32 (two columns of 2^24 doubles to generate and check);
    deterministic: every column bit for bit the single-vector product."""
    import torch
    csr, m = shared.matrix(case, lambda: lc.wide_offsets(lc.OFFSETS[case][0]))
    A = _load(csr, m, lc.off_options(family))
    assert A.matmat_group() >= max(nvecs)
    ref = mc.single_vector_columns(torch, A) if family == "det" else None
    for k, nvec in enumerate(nvecs):
        alpha, beta = mc.ALPHA_BETA[k % 2] if _is_big(case) else mc.ALPHA_BETA[k]
        mc.run(torch, A, m, nvec, alpha, beta, padx=1, pady=2, ref=ref)
    A.destroy()


# ---- 2. symmetric path -------------------------------------------------------------------------------------

def _sym_case(torch, shared, case, family, waves):
    gen, extra, pipelined = lc.SYM_CASES[case]
    csr, m = shared.matrix(case, gen)
    A = _load(csr, m, dict(lc.sym_options(family, extra), **{"spx.gpu.waves": str(waves)}), sym=True)
    inf = A.info()
    assert inf.symmetric and inf.waves == waves
    print("%s %s: sym_tiles %d, sym_segments %d, sym_pipeline %d, wave_tiles %d" % (
        case, family, inf.sym_tiles, inf.sym_segments, inf.sym_pipeline, inf.wave_tiles))
    if family in ("segments", "pipeline"):
        assert (inf.sym_segments > 0) == (case != "off-sym-3")
    assert inf.sym_pipeline == (1 if family == "pipeline" and pipelined else 0)
    products(torch, shared, A, m, repeat=family == "det")
    A.destroy()


@pytest.mark.parametrize("family", list(lc.SYM_FAMILIES))
@pytest.mark.parametrize("case", [c for c in lc.SYM_CASES if c != "passes-edge-sym"])
def test_symmetric_limits(shared, case, family):
    """Spilled sums (lists), the atomic hand-over, read-once segments with and without the pipelined kernel
    (csx_spmv_sx_kernel, where the case has passes for it), per-wavefront tiles: 24-bit offsets, a chain of
    read-once segments with row and column step 127, 3072 and 8192 slots, lanes without a slot."""
    import torch
    _sym_case(torch, shared, case, family, 4)


@pytest.mark.parametrize("waves", lc.PASS_WAVES)
@pytest.mark.parametrize("family", list(lc.SYM_FAMILIES))
def test_symmetric_pass_counts(shared, family, waves):
    import torch
    _sym_case(torch, shared, "passes-edge-sym", family, waves)


@pytest.mark.parametrize("family", ["lists", "segments"])
def test_symmetric_offsets_of_32_bits(shared, family):
    """2^24 + 4096 rows, the only symmetric case of that size: the device entry points only."""
    import torch
    csr, m = shared.matrix("off-sym-4", lc.SYM_OFFSETS["off-sym-4"][0])
    A = _load(csr, m, dict(lc.sym_options(family), **{"spx.gpu.waves": "4"}), sym=True)
    products(torch, shared, A, m, host=False, beta=family == "lists")
    A.destroy()


# ---- 2b. symmetric path, several vectors per pass -----------------------------------------------------------
# csx_spmv_mvsym_kernel (spx.gpu.sym_matmat): K = 2, 4 or 8 vectors per pass over a stream with read-once passes.
# Every column against the CSR product (matmat_cases.run: helpers.check_y, NaN behind every vector, a Y of NaN
# where beta = 0); the columns go through atomics, nothing is compared bit for bit.  The group is never
# hard-coded: it is what matmat_sym_cases.expected_mvsym_group makes of the saved stream.

def _stream_group(A, tmp_path):
    f = str(tmp_path / "group.spx")
    A.save(f)
    return msc.expected_mvsym_group(Stream(f))


def _matmat_runs(torch, A, m, nvecs=lc.NVECS_SYM):
    """The vector counts with the (alpha, beta) pairs in turn; ldx = columns + 1 or + 2: odd in every second run
    at least, where every second vector of X is 8-byte aligned only."""
    for k, nvec in enumerate(nvecs):
        alpha, beta = mc.ALPHA_BETA[k % 3]
        mc.run(torch, A, m, nvec, alpha, beta, padx=1 + k % 2, pady=5 if k % 2 else 2)


def _sym_matmat_case(torch, shared, tmp_path, case, waves):
    gen, _ = lc.SYM_MATMAT_CASES[case]
    csr, m = shared.matrix(case, gen)
    A = _load(csr, m, lc.sym_matmat_on(case, waves), sym=True)
    inf = A.info()
    assert inf.symmetric and inf.waves == waves and inf.sym_segments > 0 and not inf.wave_tiles
    g = A.matmat_group()
    print("%s tuned with spx.gpu.sym_matmat, %d wavefronts: group %d" % (case, waves, g))
    assert g == _stream_group(A, tmp_path)
    _matmat_runs(torch, A, m)
    A.destroy()


@pytest.mark.parametrize("case", list(lc.SYM_MATMAT_CASES))
def test_symmetric_matmat_limits(shared, tmp_path, case):
    """Tuned with the option, 4 wavefronts: read-once segments of every width 2 .. 8 with slots (seg-widths) and
    without, inline descriptors and listed ones (noslot) -- groups of eight, so that 15 vectors run K = 8, 4
    and 2 --, the chain with row and column step 127, 24-bit leftovers next to slots, full sets of slots."""
    import torch
    _sym_matmat_case(torch, shared, tmp_path, case, 4)


@pytest.mark.parametrize("waves", lc.PASS_WAVES)
def test_symmetric_matmat_pass_counts(shared, tmp_path, waves):
    """The pass loop of mvsym_body at its branch points.  (A launch of more than 40 KB of LDS runs eight
    wavefronts whatever the tune says: the groups of two run at the tune's count.)"""
    import torch
    _sym_matmat_case(torch, shared, tmp_path, "passes-edge-sym", waves)


@pytest.mark.parametrize("case", lc.SYM_MATMAT_RESTORED)
def test_symmetric_matmat_restored(shared, tmp_path, case):
    """A stream from a tune WITHOUT the option (row-blocks of up to 2048 rows), restored with it: the option is
    read at restore time and the group is what the stream's largest row-block leaves room for -- 1 for
    slots-wide-cap, whose product then runs column by column.  Restored without the option: group 1."""
    import torch
    gen, _ = lc.SYM_MATMAT_CASES[case]
    csr, m = shared.matrix(case, gen)
    H = tune(csr, lc.sym_matmat_default(case), sym=True, host_only=True)
    f = str(tmp_path / "default.spx")
    H.save(f)
    H.destroy()
    s = Stream(f)
    want = msc.expected_mvsym_group(s)
    assert int(s.rbs["n_rows"].max()) > 512
    assert (want == 1) == (case == "slots-wide-cap")
    sx.options_reset()
    sx.option_set("spx.gpu.sym_matmat", "true")
    B = sx.mat_restore(f)
    print("%s restored with spx.gpu.sym_matmat: group %d, largest row-block %d rows, largest core %d doubles" % (
        case, B.matmat_group(), int(s.rbs["n_rows"].max()),
        int((s.rbs["n_rows"].astype(np.int64) + s.rbs["n_slots"]).max())))
    assert B.info().symmetric and B.info().waves == 4
    assert B.matmat_group() == want
    _matmat_runs(torch, B, m)
    B.destroy()
    sx.options_reset()
    C = sx.mat_restore(f)
    assert C.matmat_group() == 1
    _matmat_runs(torch, C, m, nvecs=(3, 8))
    C.destroy()


# ---- 3. steps, segments in front, pass counts: general path -------------------------------------------------

LINEAR, LINEAR_MODES = lc.LINEAR, lc.LINEAR_MODES


@pytest.mark.parametrize("mode", list(LINEAR_MODES))
@pytest.mark.parametrize("case", list(LINEAR))
def test_steps_segments_and_pass_counts(shared, case, mode):
    """unit_origin of spmv_device.hpp and its copies (the window planner of xwindows.cpp, which turns columns
    into LDS offsets from the same bits): a disagreement is a wrong product."""
    import torch
    gen, opts = LINEAR[case]
    name = "diagonals" if case.startswith("segs") else case
    csr, m = shared.matrix(name, gen)
    A = _load(csr, m, lc.linear_options(case, mode))
    inf = A.info()
    assert bool(inf.wave_tiles) == mode.startswith("det")
    if mode == "unit-windows":
        assert inf.unit_windows == (0 if case == "step-128" else 1)       # (step-128 holds no unit pass)
    products(torch, shared, A, m, repeat=mode.startswith("det"))
    A.destroy()


@pytest.mark.parametrize("family", list(lc.LINEAR_MATMAT))
@pytest.mark.parametrize("case", list(LINEAR))
def test_steps_segments_and_pass_counts_matmat(shared, case, family):
    import torch
    gen, opts = LINEAR[case]
    name = "diagonals" if case.startswith("segs") else case
    csr, m = shared.matrix(name, gen)
    A = _load(csr, m, lc.linear_options(case, family))
    # device_mv_group: the widest K whose K * copies tiles (copies: a tile per wavefront for det, else 1) of
    # the largest row-block fit 10240 doubles -- 64 rows in passes-edge, 2048 in segs-joined, else 512
    # (segs-joined, det: 1, one product per column)
    g = A.matmat_group()
    rows = {"passes-edge": 64, "segs-joined": 2048}.get(case, 512)
    assert g == mc.expected_group(rows, 4 if family == "det" else 1)
    ref = mc.single_vector_columns(torch, A) if family == "det" else None
    mc.run(torch, A, m, 8, 0.5, 0.0, padx=1, pady=2, ref=ref)
    mc.run(torch, A, m, 11, 2.0, -0.5, padx=2, pady=1, ref=ref)
    A.destroy()


# ---- 4. edits: the host-side reader of the same fields (stream_index.cpp) -----------------------------------

def _far_end(m):
    """(row, column) of the first nonzero in the far end column of the (only) strip of an offsets case"""
    col = m.shape[1] - 38 + lc.OFF_LEFT
    for r in range(m.shape[0]):
        c = m.indices[m.indptr[r]:m.indptr[r + 1]]
        if c.size and c[-1] == col:
            return r, col
    raise AssertionError("no row holds the far end")


@pytest.mark.parametrize("case", ["off-65536", "off-2p24m1", "off-2p24", "segs-8188", "segs-joined"])
def test_set_entry_save_restore(shared, tmp_path, case):
    """set_entry on a nonzero whose offset has a non-zero high byte (the far end of a row-block's span, and a
    nonzero in the middle of it), respectively on segments far behind the first of their row-block; get_entry,
    the product, save, restore, the product; the restored off-2p24 still holds 32-bit offsets."""
    import torch
    if case.startswith("off"):
        csr, m = shared.matrix(case, lambda: lc.wide_offsets(lc.OFFSETS[case][0]))
        opts = lc.off_options("plain")
        span = lc.OFFSETS[case][0][0]
        r1, c1 = _far_end(m)
        assert c1 == lc.OFF_LEFT + span
        r2 = 333
        c2 = int(m.indices[m.indptr[r2 + 1] - 2])
        assert c2 - lc.OFF_LEFT >= 2 ** 23 or case == "off-65536"          # (bit 7 of the high byte of 24 bits)
        edits = [(r1, c1), (r2, c2)]
    else:
        csr, m = shared.matrix("diagonals", lc.diagonals)
        opts = lc.linear_options(case, "waves-4")
        # the last diagonals, in the last rows of the first row-block(s): segments 8000 and more behind the first
        edits = [(505, 505 + 15 * 211), (511, 511 + 15 * 211), (1500, 1500 + 12 * 211), (2040, 2040 + 9 * 211)]
    A = _load(csr, m, opts)
    m2 = m.copy()
    for k, (r, c) in enumerate(edits):
        assert A.get_entry(r, c) == m[r, c] != 0
        A.set_entry(r, c, 3.5 + k)
        assert A.get_entry(r, c) == 3.5 + k
        m2[r, c] = 3.5 + k
    m2 = sp.csr_matrix(m2)
    m2.sort_indices()
    assert m2.nnz == m.nnz
    products(torch, shared, A, m2, host=False)
    f = str(tmp_path / "m.spx")
    A.save(f)
    A.destroy()
    sx.options_reset()
    B = sx.mat_restore(f)
    for k, (r, c) in enumerate(edits):
        assert B.get_entry(r, c) == 3.5 + k
    products(torch, shared, B, m2, host=False, beta=False)
    if case == "off-2p24":
        g = str(tmp_path / "again.spx")
        B.save(g)
        assert lc.census(g)[0]["widths"] == {4}
    B.destroy()
