"""The preconditions of test_gpu_stream_limits.py, checked on the CPU: every case of limit_cases.py is tuned
host-only under the options its GPU test uses, saved and decoded (stream_decode.Stream).  The decoded stream
must be the input matrix exactly, and it must reach the limit the case exists for -- the width of the column
offsets, the largest step, the segments in front, the pass counts, the slots -- so that the GPU file cannot
pass because a case silently stopped reaching its limit.  (spx.gpu.waves changes the launch, not the stream:
the wavefront counts of the GPU file share the tune at 4 here, one case checks that.)"""
import numpy as np
import pytest
import scipy.sparse as sp

import sparsex_amd as sx
from helpers import tune
import limit_cases as lc
import matmat_cases as mc
import matmat_sym_cases as msc
from stream_decode import PASS, RB


def _tune(csr, m, opts, sym=False):
    if m is not None and m.shape[0] != m.shape[1]:
        return mc.load_rect(sx, csr, m.shape[1], opts, host_only=True)
    return tune(csr, opts, sym=sym, host_only=True)


def _decoded(tmp_path, csr, m, opts, sym=False, exact=True, rows_from=0):
    """census of the tuned stream; the stream holds the matrix exactly (symmetric: its strict triangles, and
    the diagonal apart)"""
    A = _tune(csr, m, opts, sym)
    f = str(tmp_path / "m.spx")
    A.save(f)
    c, s = lc.census(f, rows_from)
    if exact:
        rp, ci, va, n = csr
        ncols = s.ncols
        a = sp.csr_matrix((va, ci, rp), shape=(n, ncols))
        r, cc, v, b = s.triplets()
        got = sp.coo_matrix((v, (r, cc)), shape=(n, ncols)).tocsr()
        if sym:
            assert np.array_equal(s.dvalues, a.diagonal())
            a = (a - sp.diags(a.diagonal())).tocsr()
        else:
            assert r.size == rp[-1] == s.nnz_stored
            assert np.unique(r * ncols + cc).size == r.size
        assert got.nnz == 0 and a.nnz == 0 or abs(got - a).max() == 0
    return c, s, A


# ---- column-offset widths ---------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def off_matrices():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = lc.wide_offsets(lc.OFFSETS[name][0])
        return cache[name]
    yield get
    cache.clear()


def test_wide_offsets_generator():
    csr, m = lc.wide_offsets((1000, 300))
    rp, ci, va, n = csr
    assert m.shape == (700, 1000 + 38 + 300 + 38)
    again = lc.wide_offsets((1000, 300))[0]
    assert all(np.array_equal(a, b) for a, b in zip(csr[:3], again[:3]))
    rows = np.repeat(np.arange(n), np.diff(rp))
    for base, span in ((0, 1000), (1038, 300)):
        strip = (ci >= base) & (ci < base + span + 38)
        assert ci[strip].min() == base + 17 and ci[strip].max() == base + 17 + span
        for b in range(0, n, lc.OFF_RB):
            run = strip & (rows >= b) & (rows < b + lc.OFF_RB)
            lo = rows[run & (ci == base + 17)]
            hi = rows[run & (ci == base + 17 + span)]
            # both ends in every run of 50 rows, once, not in its first row, not in the same row; the far
            # end is the last of at least two nonzeros of its row's strip: not position 0 of its piece
            assert lo.size == 1 and hi.size == 1 and lo[0] != hi[0] and lo[0] > b and hi[0] > b
            assert int((run & (rows == hi[0])).sum()) >= 2
    # the ends' rows are not equally spaced (a vertical unit would take them out of the leftovers)
    first = rows[ci == 17]
    assert np.unique(np.diff(first)).size > 3


@pytest.mark.parametrize("case,family", sorted(lc.OFF_WIDTHS))
def test_offset_widths(tmp_path, off_matrices, case, family):
    csr, m = off_matrices(case)
    c, s, _ = _decoded(tmp_path, csr, m, lc.off_options(family))
    print("%s %s: widths %s, %d row-blocks" % (case, family, sorted(c["widths"]), len(s.rbs)))
    assert c["widths"] == lc.OFF_WIDTHS[(case, family)]
    assert lc.PASS_GATHER in c["kinds"]
    slices = {"slices-c2": 2, "slices-2": 2}.get(family, 1)
    assert int(((s.rbs["flags"] & 4) != 0).sum()) == slices - 1
    assert bool((s.rbs["flags"] & 8).all()) == (family == "slices-c2")
    # from the decoded stream: the largest offset of every row-block with leftovers of the full span sits
    # neither in lane 0 nor at position 0 of its piece
    spans = lc.OFFSETS[case][0]
    # (uncut: the strips side by side; two slices: a strip each, or -- one strip -- one end each, no full span)
    full = sum(spans) + 38 * (len(spans) - 1) if slices == 1 else spans[0] if len(spans) == 2 else None
    seen = owners = 0
    tops = set()
    for rb in s.rbs:
        if not (s.passes[int(rb["pass_off"]):int(rb["pass_off"]) + int(rb["n_pass"])]["kind"] == lc.PASS_GATHER).any():
            continue
        lane, pos, off = lc.gather_offsets(s, rb)
        tops |= set((off >> 24).tolist())
        owners += 1
        if int(off.max()) == full:
            k = int(np.argmax(off))
            assert lane[k] > 0 and pos[k] > 0
            seen += 1
    assert full is None or seen == owners >= 2
    assert slices == 2 or owners == lc.OFF_ROWS // lc.OFF_RB
    if family == "plain" and case == "off-2p24m1":
        # every byte varies at every position of a piece (bits 16-23: far more than the two values 0 and 1)
        lane, pos, off = lc.gather_offsets(s, s.rbs[0])
        for w in range(6):
            for byte in range(3):
                assert np.unique((off[pos == w] >> (8 * byte)) & 255).size > 8, (w, byte)
            assert (((off[pos == w] >> 16) & 255) >= 128).any()
    if family == "plain" and case == "off-2p24":
        assert tops == {0, 1}
    if family == "plain" and case == "off-2x-2p24":
        assert tops == {0, 1, 2}                           # (offsets up to 2^25 + 38: bits 24 and 25)


def test_the_borders_of_the_widths_sit_where_the_emitter_puts_them():
    """cidx_width of emit_gather_passes: 2 below a span of 65536, 3 below 2^24"""
    assert lc.OFF_WIDTHS[("off-65535", "plain")] == {2} and lc.OFF_WIDTHS[("off-65536", "plain")] == {3}
    assert lc.OFF_WIDTHS[("off-2p24m1", "plain")] == {3} and lc.OFF_WIDTHS[("off-2p24", "plain")] == {4}
    assert lc.OFFSETS["off-65535"][0] == (65535,) and lc.OFFSETS["off-2p24m1"][0] == (2 ** 24 - 1,)


def test_every_family_reaches_every_width():
    reached = {}
    for (case, family), widths in lc.OFF_WIDTHS.items():
        reached.setdefault(family, set()).update(widths)
    for family in lc.OFF_FAMILIES:
        missing = {2, 3, 4} - reached.get(family, set()) - {w for f, w in lc.OFF_UNREACHABLE if f == family}
        assert not missing, "%s: no case of width %s" % (family, sorted(missing))
    assert not any(w in reached.get(f, set()) for f, w in lc.OFF_UNREACHABLE)


def test_the_wavefront_count_does_not_change_the_stream(tmp_path, off_matrices):
    csr, m = off_matrices("off-65536")
    blobs = []
    for waves in (2, 4, 8):
        A = _tune(csr, m, lc.off_options("plain", waves))
        f = str(tmp_path / ("w%d.spx" % waves))
        A.save(f)
        s = lc.Stream(f)
        assert s.waves == waves
        blobs.append((s.rbs.tobytes(), s.passes.tobytes(), s.cidx.tobytes(), s.values.tobytes()))
    assert blobs[0] == blobs[1] == blobs[2]


@pytest.mark.parametrize("case", list(lc.SYM_OFFSETS))
def test_symmetric_offset_widths(tmp_path, case):
    """off-sym-4 holds 33 k row-blocks, all but a few of them a stretch of the diagonal with a handful of
    mirrored nonzeros: the lane-by-lane comparison is made for the row-blocks of the late rows, which hold
    the wide offsets, and for the two families its GPU test runs."""
    gen, width = lc.SYM_OFFSETS[case]
    csr, m = gen()
    rp, ci, va, n = csr
    big = case == "off-sym-4"
    for family in (("lists", "segments") if big else tuple(lc.SYM_FAMILIES)):
        c, s, _ = _decoded(tmp_path, csr, m, lc.sym_options(family), sym=True, exact=not big,
                           rows_from=n - 812 if big else 0)
        print("%s %s: widths %s" % (case, family, sorted(c["widths"])))
        assert max(c["widths"]) == width
        # ... in the row-blocks of the late rows: the lower triangle, not its mirror image
        late = s.rbs[s.rbs["cidx_width"] == width]
        assert len(late) and int(late["row0"].min()) >= n - 300 - 512
        if big:
            s.rbs = late
            r, cc, v, b = s.triplets()
            lo = int(late["row0"].min())
            assert int((late["row0"].astype(np.int64) + late["n_rows"]).max()) == n
            assert len(late) == 1 or (np.diff(late["row0"].astype(np.int64)) == late["n_rows"][:-1]).all()
            got = sp.coo_matrix((v, (r - lo, cc)), shape=(n - lo, n)).tocsr()
            want = m[lo:]
            want = (want - sp.diags(m.diagonal()[lo:], lo, shape=want.shape)).tocsr()
            assert abs(got - want).max() == 0


# ---- steps ------------------------------------------------------------------------------------------------

ALL_LINEAR_MODES = list(lc.LINEAR_MODES) + list(lc.LINEAR_MATMAT)


@pytest.mark.parametrize("case", list(lc.STEPS))
def test_steps(tmp_path, case):
    """every tune test_gpu_stream_limits.py makes of the case: limit_cases.linear_options"""
    gen, opts, sym, steps = lc.STEPS[case]
    csr, m = gen()
    for mode in ALL_LINEAR_MODES:
        c, s, A = _decoded(tmp_path, csr, m, lc.linear_options(case, mode))
        print("%s %s: steps by kind %s" % (case, mode, c["steps"]))
        assert c["steps"] == steps
        assert lc.PASS_GATHER in c["kinds"] or case != "step-128"
    if steps:
        # the unit-window planner re-derives the columns from the same bits; it stages the lines of all
        # row-blocks but the one of the horizontal line, whose 70 columns span more than a window holds
        plan = A.unit_windows()
        print("unit windows: %d of %d row-blocks" % (plan["rowblocks_with_windows"], plan["rowblocks_with_units"]))
        assert plan["rowblocks_with_windows"] >= plan["rowblocks_with_units"] - 1 > 0


def test_the_anti_diagonal_of_the_step_case_can_be_walked_the_wrong_way():
    """columns 9500 - 127 t: 9500 + 127 t stays inside x, so a kernel that took +step for -step would read a
    valid (and different) element"""
    csr, m = lc.step_lines(127)
    coo = m.tocoo()
    ad = (coo.row - 1100) % 127 == 0
    ad &= coo.col == 9500 - (coo.row - 1100)
    assert int(ad.sum()) == lc.STEP_LEN
    assert 9500 + 127 * lc.STEP_LEN < lc.STEP_N and 9500 - 127 * (lc.STEP_LEN - 1) >= 0


def test_symmetric_steps(tmp_path):
    csr, m = lc.step_lines_sym(127)
    for family in lc.SYM_FAMILIES:
        c, s, A = _decoded(tmp_path, csr, m, lc.sym_options(family, lc.STEP_SYM_OPTS), sym=True)
        print("step-127 symmetric, %s: steps %s, of read-once segments %s" % (family, c["steps"], c["symseg_steps"]))
        if family in ("segments", "pipeline"):
            assert c["symseg_steps"].get(3) == 127
            # the headers make_sx_header rewrites: row step 127, column step +127
            heads, n_sx, count = A.sym_pipeline()
            sx_heads = heads[((heads[:, 4] >> 24) & 4) != 0]
            geo = sx_heads[:, 1]
            drow, dcol = (geo >> 11) & 127, ((geo >> 18) & 255).astype(np.int64) - 128
            assert count["sx_passes"] == len(sx_heads) > 0
            assert ((drow == 127) & (dcol == 127)).any()
        else:
            assert c["steps"].get(3) == 127
    assert any("-127" in k for k in lc.UNREACHABLE)


# ---- segments in front, pass counts -----------------------------------------------------------------------

@pytest.mark.parametrize("case", list(lc.SEGS))
def test_segments_in_front(tmp_path, case):
    opts, front, seg0, n_pass, joined = lc.SEGS[case]
    assert lc.LINEAR[case][1] is opts
    csr, m = lc.diagonals()
    for mode in ALL_LINEAR_MODES:
        c, s, _ = _decoded(tmp_path, csr, m, lc.linear_options(case, mode))
        print("%s %s: segments in front %d (passes with elem0 > 0: %d), seg0 %d, n_pass %d, rows %d" % (
            case, mode, c["front"], c["elem0_front"], c["seg0"], c["n_pass"], c["rows"]))
        assert c["front"] >= front and c["front"] <= 8191 and c["seg0"] >= seg0 and c["n_pass"] >= n_pass
        assert c["rows"] == (2048 if joined else 512)       # (what the matmat groups of the GPU file assume)
        if joined:
            assert c["elem0_front"] >= front


def test_pass_counts_at_the_branch_points(tmp_path):
    assert lc.PASS_COUNTS == [1, 2, 3, 4, 5, 7, 8, 9, 13, 16, 17, 25]
    csr, m = lc.pass_edges()
    for mode in ALL_LINEAR_MODES:
        c, s, _ = _decoded(tmp_path, csr, m, lc.linear_options("passes-edge", mode))
        assert c["pass_counts"] - {0} == set(lc.PASS_COUNTS), sorted(c["pass_counts"])
        assert c["rows"] == 64
    csr, m = lc.pass_edges_sym()
    for family in lc.SYM_FAMILIES:
        c, s, _ = _decoded(tmp_path, csr, m, lc.sym_options(family, lc.PASS_SYM_OPTS), sym=True)
        print("passes-edge symmetric, %s: %s" % (family, sorted(c["pass_counts"])))
        assert c["pass_counts"] >= set(lc.PASS_COUNTS)
        assert (lc.PASS_SYMSEG in c["kinds"]) == (family in ("segments", "pipeline"))


# ---- slots ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", list(lc.SLOTS))
def test_slots(tmp_path, case):
    """The stream with read-once segments (family "segments"), decoded lane by lane against the matrix: the
    slots exist in it alone (limit_cases.SLOTS).  The pipeline is a plan on top of the same stream;
    slots-wide-cap, which is small, shows that byte for byte and is decoded under the other families too."""
    gen, extra, n_slots, noslot = lc.SLOTS[case]
    csr, m = gen()
    c, s, A = _decoded(tmp_path, csr, m, lc.sym_options("segments", extra), sym=True)
    print("%s: n_slots %d, lanes without a slot %d; wide row-blocks: n_slots %d, lanes without %d" % (
        case, c["n_slots"], c["noslot"], c["wide_slots"], c["wide_noslot"]))
    assert lc.PASS_SYMSEG in c["kinds"] and s.sym_atomic
    if n_slots is not None:
        assert c["n_slots"] == n_slots
    assert (A.sym_pipeline()[2]["rowblocks_with_sx"] > 0) == lc.SYM_CASES[case][2]
    assert c["noslot"] >= noslot and (noslot > 0 or c["noslot"] == 0)
    if case == "slots-wide-cap":
        # (limit_cases.UNREACHABLE: the slots of a wide row-block never run out)
        assert c["wide_slots"] == 8192 and c["wide_noslot"] == 0
        assert any("8192" in k for k in lc.UNREACHABLE)
        for family in lc.SYM_FAMILIES:
            if family == "segments":
                continue
            cf, p, _ = _decoded(tmp_path, csr, m, lc.sym_options(family, extra), sym=True)
            if family == "pipeline":
                assert p.rbs.tobytes() == s.rbs.tobytes() and p.passes.tobytes() == s.passes.tobytes()
                assert p.descs.tobytes() == s.descs.tobytes() and p.values.tobytes() == s.values.tobytes()
            else:
                assert cf["n_slots"] == 0 and lc.PASS_SYMSEG not in cf["kinds"]


@pytest.mark.parametrize("case", [c for c in lc.SYM_CASES if c not in lc.SLOTS])
def test_which_symmetric_cases_the_pipeline_takes(case):
    """plan_sym_pipeline on the host: the cases whose GPU test asserts info().sym_pipeline == 1 hold passes
    that make_sx_header rewrites, the others none (the slot cases: test_slots)."""
    gen, extra, pipelined = lc.SYM_CASES[case]
    csr, m = gen()
    A = tune(csr, lc.sym_options("pipeline", extra), sym=True, host_only=True)
    heads, n_sx, count = A.sym_pipeline()
    print("%s: %s" % (case, count))
    assert (count["rowblocks_with_sx"] > 0) == pipelined


# ---- symmetric path, several vectors per pass -----------------------------------------------------------------

def _sym_matmat_census(tmp_path, case, opts, gen=None):
    csr, m = (gen or lc.SYM_MATMAT_CASES[case][0])()
    c, s, A = _decoded(tmp_path, csr, m, opts, sym=True)
    A.destroy()
    c["group"] = msc.expected_mvsym_group(s)
    c["wide"] = [rb for rb in c["rowblocks"] if rb[0] > 512]
    return c, s


def _check_sym_matmat(case, mode, c):
    """What the stream of `case` under `mode` ("on": tuned with spx.gpu.sym_matmat, "default": without) must hold
    for its runs in test_gpu_stream_limits.py to reach the limit it is there for."""
    widths, steps = c["symseg_widths"], c["symseg_steps"]
    if mode == "on":
        assert c["rows"] <= 512                         # (the tune with the option emits no wide row-block)
    if case == "noslot" and mode == "on":
        assert widths >= lc.SEG_WIDTHS and c["symseg_inline"] > 0 and c["symseg_listed"] > 0
        assert c["noslot"] >= 100 and c["group"] == 8
    if case == "seg-widths" and mode == "on":
        assert widths >= lc.SEG_WIDTHS and c["symseg_inline"] == 0 and c["noslot"] == 0 and c["group"] == 8
    if case == "seg-widths" and mode == "default":
        # (not asked of a restored stream, but there: every width in row-blocks of more than 512 rows)
        assert widths >= lc.SEG_WIDTHS and c["wide"] and c["group"] >= 2
    if case == "step-127-sym":
        assert steps.get(3) == 127
        if mode == "default":
            assert c["wide"] and c["group"] >= 2
    if case == "passes-edge-sym" and mode == "on":
        assert c["pass_counts"] >= set(lc.PASS_COUNTS) and lc.PASS_SYMSEG in c["kinds"] and c["group"] >= 2
    if case == "off-sym-3-runs" and mode == "on":
        assert any(w == 3 and slots > 0 and {lc.PASS_GATHER, lc.PASS_SYMSEG} <= kinds
                   for rows, slots, w, kinds in c["rowblocks"])
    if case == "slots-3072" and mode == "default":
        assert any(slots == 3072 for rows, slots, w, kinds in c["wide"]) and c["n_slots"] == 3072
        assert lc.PASS_GATHER_LDS in c["kinds"] and c["group"] == 2
    if case == "slots-wide-cap" and mode == "default":
        assert any(rows == 2048 and slots == 8192 for rows, slots, w, kinds in c["wide"]) and c["group"] == 1
    if case == "noslot" and mode == "default":
        assert c["wide"] and c["group"] >= 2


@pytest.mark.parametrize("case", list(lc.SYM_MATMAT_CASES))
def test_symmetric_matmat_streams(tmp_path, case):
    """Tuned with the option and without it (the stream that test_gpu_stream_limits.py restores with it): the
    matrix exactly, and the limit the case is run for."""
    for mode, opts in (("on", lc.sym_matmat_on(case)), ("default", lc.sym_matmat_default(case))):
        c, s = _sym_matmat_census(tmp_path, case, opts)
        print("%s %s: group %d, rows %d, core %d, read-once widths %s (%d inline, %d not), %d lanes without a slot, "
              "steps %s, %d wide row-blocks" % (
                  case, mode, c["group"], c["rows"], max(rb[0] + rb[1] for rb in c["rowblocks"]),
                  sorted(c["symseg_widths"]), c["symseg_inline"], c["symseg_listed"], c["noslot"], c["symseg_steps"],
                  len(c["wide"])))
        assert s.symmetric and s.sym_atomic
        _check_sym_matmat(case, mode, c)
    assert set(lc.SYM_MATMAT_RESTORED) <= set(lc.SYM_MATMAT_CASES)
    assert not lc.SYM_MATMAT_UNREACHABLE


def test_symmetric_matmat_checks_bite(tmp_path):
    """seg-widths regenerated with runs of three columns only no longer passes its check; the expected group
    follows the core (a group of 8 needs 8 x core x 8 B + 4 B per slot group within 80 KB)."""
    c, s = _sym_matmat_census(tmp_path, "seg-widths", lc.sym_matmat_on("seg-widths"), gen=lambda: msc.seg_widths(3))
    assert c["symseg_widths"] == {3}
    with pytest.raises(AssertionError):
        _check_sym_matmat("seg-widths", "on", c)

    class Fake:
        symmetric, sym_atomic = 1, 1
        passes = np.zeros(1, dtype=PASS)

        def __init__(self, rows, slots):
            self.rbs = np.zeros(1, dtype=RB)
            self.rbs["n_rows"], self.rbs["n_slots"] = rows, slots
    Fake.passes["kind"] = lc.PASS_SYMSEG
    cores = ((512, 760), (512, 768), (1024, 8), (64, 1752), (930, 3072), (2048, 8192), (512, 3072))
    assert [msc.expected_mvsym_group(Fake(r, sl)) for r, sl in cores] == [8, 4, 8, 4, 2, 1, 2]
    Fake.passes["kind"] = lc.PASS_GATHER
    assert msc.expected_mvsym_group(Fake(64, 0)) == 1
