"""Cases that drive the fields of the row-block stream (sparsex_amd/csrc/gpu_format.h) to the upper end of
their ranges: column offsets of 16, 24 and 32 bits, the 7-bit step of a unit descriptor, its 13 bits of
"segments in front", the pass count of a row-block around the branch points of the kernels' pass loop, and
the transposed-sum slots of the symmetric path; and what the multi-vector kernel of the read-once symmetric
passes (spx.gpu.sym_matmat) adds to those: every width of a read-once segment, wide offsets in a row-block with
slots, streams of a default tune restored with the option.  test_limit_cases.py tunes every case host-only and asserts,
on the decoded stream, that it reaches the limit named here; test_gpu_stream_limits.py runs the same tunes
through every kernel family that decodes the field.  No pytest code in here.

Every generator is seeded and uses numpy / scipy only; it returns (csr tuple, scipy matrix) like
matmat_cases.band."""
import numpy as np
import scipy.sparse as sp

from sparsex_amd import synth
import matmat_sym_cases as msc
from stream_decode import Stream

NOSAMPLE = {"spx.preproc.sampling": "none"}
PASS_UNIT, PASS_GATHER, PASS_SYMTILE, PASS_GATHER_LDS, PASS_SYMSEG = 0, 2, 3, 4, 5
ALPHA_BETA = (2.0, -0.5)


def _csr(m):
    m = sp.csr_matrix(m)
    m.sum_duplicates()
    m.sort_indices()
    return (m.indptr.astype(np.int32), m.indices.astype(np.int32), m.data.copy(), m.shape[0]), m


def _symmetric(rows, cols, n, rng):
    """strict lower triangle (rows, cols) + its mirror image + a diagonal"""
    keep = cols < rows
    key = np.unique(rows[keep].astype(np.int64) * n + cols[keep])
    r, c = key // n, key % n
    v = rng.uniform(-1, 1, key.size)
    d = np.arange(n)
    m = sp.coo_matrix((np.concatenate([v, v, rng.uniform(1.0, 2.0, n)]),
                       (np.concatenate([r, c, d]), np.concatenate([c, r, d]))), shape=(n, n))
    return _csr(m)


# ---- column-offset widths ---------------------------------------------------------------------------------
# gpu_emit.cpp (emit_gather_passes): the width of a row-block's offsets is 2 where its leftovers span fewer than
# 65536 columns (cmax - cmin), 3 below 2^24, else 4.

OFF_ROWS, OFF_RB, OFF_LEFT = 700, 50, 17


def wide_offsets(spans, seed=7):
    """700 x sum(span + 38): one strip of columns per entry of `spans`, six nonzeros per row and strip.  In
    every run of 50 rows (a row-block under spx.gpu.rowblock_rows=50) one row holds the strip's column 17 and
    another one its column 17 + span -- never the first row of the run, and in a row of their own each; which
    rows, varies from run to run (at a constant distance the ends would be mined as a vertical unit and leave
    the leftovers).  The other columns are uniform over the span, so that every byte of an offset varies from
    lane to lane and along a piece.  A row's leftovers are sorted by column: the far end is the LAST nonzero
    of its piece (and never lane 0); the near end, offset 0, is by construction the first of its piece."""
    rng = np.random.RandomState(seed)
    n = OFF_ROWS
    rows, cols, base = [], [], 0
    for span in spans:
        for r in range(n):
            c = np.unique(rng.randint(OFF_LEFT + 1, OFF_LEFT + span, 6))
            rows.append(np.full(c.size, r)); cols.append(base + c)
        for b in range(0, n, OFF_RB):
            lo, hi = b + 1 + rng.choice(OFF_RB - 1, 2, replace=False)
            rows.append(np.array([lo, hi])); cols.append(base + np.array([OFF_LEFT, OFF_LEFT + span]))
        base += span + 38
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    m = sp.coo_matrix((rng.uniform(-1, 1, rows.size), (rows, cols)), shape=(n, base))
    return _csr(m)


OFF_OPTS = dict(NOSAMPLE, **{"spx.gpu.rowblock_rows": str(OFF_RB)})
# name -> (spans of the strips, the cidx_width every row-block with a kind-2 pass must have under "plain")
OFFSETS = {
    "off-65535": ((65535,), {2}),
    "off-65536": ((65536,), {3}),
    "off-2p24m1": ((2 ** 24 - 1,), {3}),
    "off-2p24": ((2 ** 24,), {4}),
    # twice as wide: a strip per half of the columns, for the streams that are cut into two column slices
    "off-2x-65536": ((65536, 65536), {3}),
    "off-2x-2p24": ((2 ** 24, 2 ** 24), {4}),
}
# The families of the general path.  All pin the wavefront count where the test does not: the launch tuner
# may emit the stream again with other row-blocks (autotune_launch of api.cpp).
OFF_FAMILIES = {
    "plain": {"spx.gpu.wave_tiles": "false", "spx.gpu.col_phases": "1", "spx.gpu.unit_windows": "false"},
    "no-window": {"spx.gpu.wave_tiles": "false", "spx.gpu.col_phases": "1", "spx.gpu.unit_windows": "false",
                  "spx.gpu.x_window": "false"},
    "det": {"spx.gpu.deterministic": "true", "spx.gpu.col_phases": "1", "spx.gpu.unit_windows": "false"},
    "slices-c2": {"spx.gpu.wave_tiles": "false", "spx.gpu.col_phases": "c2", "spx.gpu.unit_windows": "false"},
    "slices-2": {"spx.gpu.wave_tiles": "false", "spx.gpu.col_phases": "2", "spx.gpu.unit_windows": "false"},
    "unit-windows": {"spx.gpu.wave_tiles": "false", "spx.gpu.col_phases": "1", "spx.gpu.unit_windows": "true"},
}
# (case, family) -> the widths of the row-blocks that own a kind-2 pass.  A stream cut into two column slices
# holds each half of the columns in row-blocks of its own: a one-strip case loses its span there (each slice
# sees one end only), the two-strip cases keep one strip per slice.
OFF_WIDTHS = {}
for _c in ("off-65535", "off-65536", "off-2p24m1", "off-2p24"):
    for _f in ("plain", "no-window", "det", "unit-windows"):
        OFF_WIDTHS[(_c, _f)] = OFFSETS[_c][1]
for _f in ("slices-c2", "slices-2"):
    OFF_WIDTHS[("off-65535", _f)] = {2}
    OFF_WIDTHS[("off-2x-65536", _f)] = {3}
    OFF_WIDTHS[("off-2x-2p24", _f)] = {4}
# ... and uncut, the two strips side by side: offsets up to 2^25 + 38, bit 24 and bit 25 of the 32
OFF_WIDTHS[("off-2x-2p24", "plain")] = {4}
# (family, width) that no case reaches, each with the line that makes it so: none
OFF_UNREACHABLE = {}


def off_options(family, waves=4):
    return dict(OFF_OPTS, **dict(OFF_FAMILIES[family], **{"spx.gpu.waves": str(waves)}))


# symmetric: the leftovers of the lower triangle of ONE row-block span the width
def sym_wide(n, span, late=300, ends=24, seed=11, runs=False):
    """n x n symmetric: a diagonal, and `late` last rows with four nonzeros each, uniform over columns
    (3, 3 + span); `ends` of them, chosen at random, also hold column 3, as many others column 3 + span.  Few
    enough (fewer than the 64 leftovers an x window needs) and irregular enough (no vertical unit) to stay
    leftovers: the leftovers of the row-blocks of the late rows span `span` columns exactly.  `runs`: every late
    row r also holds the three columns from span + 40 + 8 * ((7 r) % 50) on, behind the span and in front of
    the late rows: read-once segments (with slots: 50 groups of eight columns) next to the wide leftovers."""
    rng = np.random.RandomState(seed)
    assert span + 16 < n - late
    r = np.repeat(np.arange(n - late, n), 4)
    c = rng.randint(4, 3 + span, late * 4)
    pick = rng.choice(late, 2 * ends, replace=False)
    r = np.concatenate([r, n - late + pick])
    c = np.concatenate([c, np.full(ends, 3), np.full(ends, 3 + span)])
    if runs:
        assert span + 40 + 8 * 49 + 3 <= n - late
        rr = np.arange(n - late, n)
        r = np.concatenate([r, np.repeat(rr, 3)])
        c = np.concatenate([c, (span + 40 + 8 * ((7 * rr) % 50)[:, None] + np.arange(3)[None, :]).ravel()])
    return _symmetric(r, c, n, rng)


SYM_OFFSETS = {
    "off-sym-3": (lambda: sym_wide(70000, 65536), 3),
    "off-sym-4": (lambda: sym_wide(2 ** 24 + 4096, 2 ** 24), 4),
}

# The families of the symmetric path.
SYM_FAMILIES = {
    "lists": {"spx.gpu.sym_spill": "lists", "spx.gpu.sym_segments": "false"},
    "atomic": {"spx.gpu.sym_spill": "atomic", "spx.gpu.sym_segments": "false"},
    "segments": {"spx.gpu.sym_segments": "true", "spx.gpu.sym_pipeline": "false"},
    "pipeline": {"spx.gpu.sym_segments": "true", "spx.gpu.sym_pipeline": "true"},
    "det": {"spx.gpu.deterministic": "true"},
}


def sym_options(family, extra=None):
    return dict(NOSAMPLE, **dict(SYM_FAMILIES[family], **(extra or {})))


# ---- steps ------------------------------------------------------------------------------------------------

STEP_N, STEP_LEN = 20000, 70


def step_lines(stride, seed=13):
    """20000 x 20000 with a vertical, a diagonal, an anti-diagonal and a horizontal line of 70 nonzeros each,
    `stride` apart.  The anti-diagonal starts at column 9500: stepping the wrong way from any of its nonzeros,
    by as many steps as the line is long, still lands inside x."""
    rng = np.random.RandomState(seed)
    t = np.arange(STEP_LEN) * stride
    rows = np.concatenate([300 + t, 700 + t, 1100 + t, np.full(STEP_LEN, 15000)])
    cols = np.concatenate([np.full(STEP_LEN, 12000), 10500 + t, 9500 - t, 400 + t])
    m = sp.coo_matrix((rng.uniform(0.5, 1.5, rows.size), (rows, cols)), shape=(STEP_N, STEP_N))
    return _csr(m)


def step_lines_sym(stride, seed=17):
    """The symmetric counterpart: the same four thin lines below the diagonal (in the symmetric tunes they
    are leftovers, but for the diagonal one: the general case is where the four kinds carry their step),
    and a chain of runs of three columns right in front of the diagonal, `stride` rows apart (rows r,
    columns r - 3 .. r - 1): what the read-once segments take, stacked along a diagonal with row and
    column step `stride`.  Plus a diagonal."""
    rng = np.random.RandomState(seed)
    t = np.arange(STEP_LEN) * stride
    rows = np.concatenate([10300 + t, 10700 + t, 10100 + t, np.full(STEP_LEN, 19500)])
    cols = np.concatenate([np.full(STEP_LEN, 6000), 700 + t, 9500 - t, 400 + t])
    chain = 40 + np.arange(150) * stride
    rows = np.concatenate([rows, np.repeat(chain, 3)])
    cols = np.concatenate([cols, (chain[:, None] - 3 + np.arange(3)[None, :]).ravel()])
    return _symmetric(rows, cols, STEP_N, rng)


def step_xform(stride):
    return "v{%d},d{%d},ad{%d},h{%d}" % ((stride,) * 4)


# (The symmetric step case, step_lines_sym(127) under STEP_SYM_OPTS, exercises ONE kind at step 127: the
# diagonal one, SPX_KIND_DIAG -- in the unit descriptors of the mirrored families and, with row and column step
# +127, in the read-once segments and the headers of their pipeline.  Its other three lines are leftovers
# there; the kinds 1, 2 and 4 carry step 127 in the general step-127 case only.  See UNREACHABLE.)
STEP_SYM_OPTS = {"spx.preproc.xform": step_xform(127)}
STEPS = {
    # name -> (generator, options, symmetric, {descriptor kind: largest step} the stream must hold)
    "step-127": (lambda: step_lines(127), dict(NOSAMPLE, **{"spx.preproc.xform": step_xform(127)}), False,
                 {1: 127, 2: 127, 3: 127, 4: 127}),
    # one past the field: no descriptor carries a step, the lines go to the gather passes
    "step-128": (lambda: step_lines(128), dict(NOSAMPLE, **{"spx.preproc.xform": step_xform(128)}), False, {}),
}


# ---- segments in front ------------------------------------------------------------------------------------

def diagonals(n=4096, ndiag=16, gap=211, seed=19):
    """n x n with `ndiag` diagonals `gap` columns apart, the first one the main diagonal: under
    spx.preproc.xform=d every nonzero is a one-wide segment of a diagonal unit."""
    rng = np.random.RandomState(seed)
    r = np.repeat(np.arange(n), ndiag)
    c = r + np.tile(np.arange(ndiag) * gap, n)
    keep = c < n
    m = sp.coo_matrix((rng.uniform(-1, 1, int(keep.sum())), (r[keep], c[keep])), shape=(n, n))
    return _csr(m)


SEG_OPTS = dict(NOSAMPLE, **{"spx.preproc.xform": "d", "spx.gpu.rowblock_rows": "512",
                             "spx.gpu.rowblock_elems": "8192"})
SEGS = {
    # name -> (options, least "segments in front", least seg0, least n_pass, elem0 > 0 required)
    # units of four nonzeros: the last descriptor of a row-block of 512 rows x 16 diagonals starts at segment 8188
    "segs-8188": (dict(SEG_OPTS, **{"spx.matrix.max_unit_size": "4"}), 8188, 8128, 128, False),
    # row-blocks joined from four planned ones: the passes of the later parts carry the first row of their part
    "segs-joined": (dict(SEG_OPTS, **{"spx.gpu.rowblock_rows": "2048", "spx.gpu.rowblock_elems": "24000"}),
                    8000, 8128, 129, True),
}

# ---- pass counts ------------------------------------------------------------------------------------------
# spmv_body of spmv_kernels.hip: wavefront w of W takes passes w, w + W, ... two at a time; `two` and the
# prefetch of the next round change at n_pass = W, W + 1, 2W, 2W + 1, 3W + 1.
PASS_WAVES = (2, 4, 8)
PASS_COUNTS = sorted({c for w in PASS_WAVES for c in (1, w, w + 1, 2 * w, 2 * w + 1, 3 * w + 1)})


def pass_edges(seed=23):
    """Diagonal blocks side by side, one per wanted pass count k: 64 rows with k diagonals 70 columns apart
    (shifted by the block's number: no diagonal goes on into the next block, every unit is 64 long), that is
    k passes of 64 one-wide segments in a row-block of 64 rows."""
    rng = np.random.RandomState(seed)
    nb = len(PASS_COUNTS)
    n = 64 * nb + 70 * max(PASS_COUNTS) + nb
    rows, cols = [], []
    for b, k in enumerate(PASS_COUNTS):
        r = np.repeat(64 * b + np.arange(64), k)
        rows.append(r); cols.append(r + b + np.tile(np.arange(k) * 70, 64))
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    m = sp.coo_matrix((rng.uniform(-1, 1, rows.size), (rows, cols)), shape=(n, n))
    return _csr(m)


PASS_OPTS = dict(NOSAMPLE, **{"spx.preproc.xform": "d", "spx.gpu.rowblock_rows": "64", "spx.gpu.rowblock_elems": "8192"})
PASS_SYM_OPTS = {"spx.gpu.rowblock_rows": "64", "spx.gpu.rowblock_elems": "8192", "spx.gpu.sym_wide_rows": "512"}


def pass_edges_sym(seed=29):
    """The same counts on the symmetric path: block b holds k runs of three columns per row, 70 apart, in
    front of the block and shifted by four columns from block to block (read-once segments where they are on,
    mirrored units elsewhere)."""
    rng = np.random.RandomState(seed)
    front = 2560                    # (a multiple of 64, and behind every column: the mirror image lands in front)
    assert 64 * len(PASS_COUNTS) + 70 * (max(PASS_COUNTS) - 1) + 4 * len(PASS_COUNTS) + 3 < front
    n = front + 64 * len(PASS_COUNTS)
    rows, cols = [], []
    for b, k in enumerate(PASS_COUNTS):
        r = front + 64 * b + np.arange(64)
        for d in range(k):
            for w in range(3):
                rows.append(r); cols.append(r - front + 70 * d + 4 * b + w)
    return _symmetric(np.concatenate(rows), np.concatenate(cols), n, rng)


# ---- the general-path tunes of the steps, the segments in front and the pass counts -------------------------
# name -> (generator, options); every tune of the GPU file is one of LINEAR x LINEAR_MODES or LINEAR x
# LINEAR_MATMAT, through linear_options.
LINEAR = {
    "step-127": (STEPS["step-127"][0], STEPS["step-127"][1]),
    "step-128": (STEPS["step-128"][0], STEPS["step-128"][1]),
    "segs-8188": (diagonals, SEGS["segs-8188"][0]),
    "segs-joined": (diagonals, SEGS["segs-joined"][0]),
    "passes-edge": (pass_edges, PASS_OPTS),
}
LINEAR_MODES = {
    "waves-2": {"spx.gpu.waves": "2", "spx.gpu.wave_tiles": "false", "spx.gpu.unit_windows": "false"},
    "waves-4": {"spx.gpu.waves": "4", "spx.gpu.wave_tiles": "false", "spx.gpu.unit_windows": "false"},
    "waves-8": {"spx.gpu.waves": "8", "spx.gpu.wave_tiles": "false", "spx.gpu.unit_windows": "false"},
    "det-2": {"spx.gpu.waves": "2", "spx.gpu.deterministic": "true"},
    "det-4": {"spx.gpu.waves": "4", "spx.gpu.deterministic": "true"},
    "det-8": {"spx.gpu.waves": "8", "spx.gpu.deterministic": "true"},
    "unit-windows": {"spx.gpu.waves": "4", "spx.gpu.wave_tiles": "false", "spx.gpu.unit_windows": "true"},
}
# the multi-vector product on the same cases
LINEAR_MATMAT = {
    "plain": {"spx.gpu.waves": "4", "spx.gpu.wave_tiles": "false"},
    "det": {"spx.gpu.waves": "4", "spx.gpu.deterministic": "true"},
}


def linear_options(case, mode):
    modes = LINEAR_MODES if mode in LINEAR_MODES else LINEAR_MATMAT
    return dict(dict(LINEAR[case][1], **{"spx.gpu.col_phases": "1"}), **modes[mode])


# ---- slots ------------------------------------------------------------------------------------------------

def wide_slots(seed=31):
    """Symmetric, 10752 rows; every row holds the run (row - 2, row - 1).  Rows 8192 .. 10239 (one row-block of
    2048 rows under spx.gpu.sym_wide_rows=2048) also hold a run of two columns each, two rows to an aligned
    group of eight early columns: 1023 groups, and one more for the run in front of the row-block's first
    row -- the 8192 slots of such a row-block (SPX_MAX_WIDE_SLOTS), exactly.  The 512 last rows (a row-block
    that has nothing to join) hold a run in a group of their own each: 512 groups where 384 fit
    (SPX_MAX_TILE_SLOTS = 3072 slots), the segments of the others get no slot."""
    rng = np.random.RandomState(seed)
    first, late, tail = 8192, 2048, 512
    n = first + late + tail
    i = np.arange(late)
    g = np.minimum(i // 2, 1022)
    far_r = np.repeat(first + i, 2)
    far_c = (8 * g + 4 * (i % 2))[:, None] + np.arange(2)[None, :]
    k = np.arange(tail)
    tail_r = np.repeat(first + late + k, 2)
    tail_c = (8 * k)[:, None] + 3 + np.arange(2)[None, :]
    r = np.arange(2, n)
    near_r = np.repeat(r, 2)
    near_c = (r[:, None] - 2 + np.arange(2)[None, :])
    return _symmetric(np.concatenate([far_r, tail_r, near_r]),
                      np.concatenate([far_c.ravel(), tail_c.ravel(), near_c.ravel()]), n, rng)


# name -> (generator, options on top of the family's, largest n_slots (exactly; None: not stated),
#          least number of lanes without a slot).  The slots exist in the streams with read-once segments only:
#          test_limit_cases.py decodes the "segments" tune of every case (the "pipeline" family runs the same
#          stream under a launch-side plan, shown byte for byte on slots-wide-cap); the "lists", "atomic" and
#          "det" tunes hold no such slots (n_slots 0 without tiles) and run the same matrices on the GPU as
#          further products, decoded on the CPU for slots-wide-cap only -- kkt44 takes 11 s per decode.
SLOTS = {
    "slots-3072": (lambda: (synth.syn_nlpkkt(44), None), {}, 3072, 0),
    "slots-wide-cap": (wide_slots, {"spx.gpu.sym_wide_rows": "2048", "spx.gpu.rowblock_rows": "512"}, 8192, 100),
    "noslot": (lambda: (synth.syn_cant(0.2), None), {}, None, 100),
}
# What no stream reaches, with the lines that make it so (sparsex_amd/csrc/gpu_emit.cpp).
UNREACHABLE = {
    "a row-block of more than 512 rows whose slots ran out (n_slots 8192 AND lanes without a slot in it)":
        "emit_gpu joins planned row-blocks only while the groups of eight columns their segments touch fit "
        "SPX_MAX_WIDE_SLOTS ('if (merged.size() * 8 > SPX_MAX_WIDE_SLOTS) break;'), and never one that holds "
        "tiles ('joinable': '!rb_tiles[i].empty()'), whose groups assign_slots would add on top: slots-wide-cap "
        "reaches 8192 slots in its wide row-block and runs out of slots in its last, narrow one (3072)",
    "read-once segments (SPX_PASS_SYMSEG) with a column step of -127, or a row step without a column step":
        "RbBuilder::stack_groups chains row segments along diagonals only (emit_chain(..., SPX_KIND_DIAG, step)), "
        "as blocks (step 0) or as chunks of one row (step 8): step-127 symmetric reaches drow = dcol = +127",
}


# The symmetric cases of the GPU file: name -> (generator, options on top of the family's, whether the
# read-once pipeline takes passes of it (csx_spmv_sx_kernel under the "pipeline" family)).
SYM_CASES = {
    "off-sym-3": (SYM_OFFSETS["off-sym-3"][0], {}, False),
    "step-127-sym": (lambda: step_lines_sym(127), STEP_SYM_OPTS, True),
    "slots-3072": (SLOTS["slots-3072"][0], SLOTS["slots-3072"][1], True),
    "slots-wide-cap": (SLOTS["slots-wide-cap"][0], SLOTS["slots-wide-cap"][1], True),
    "noslot": (SLOTS["noslot"][0], SLOTS["noslot"][1], False),
    "passes-edge-sym": (pass_edges_sym, PASS_SYM_OPTS, True),
}


# ---- symmetric path, several vectors per pass (spx.gpu.sym_matmat, csx_spmv_mvsym_kernel) --------------------
# The cases above that reach a limit in the read-once passes or next to them, and two of this kernel's own:
# read-once segments of every width (mvsym_seg_pass<W, K>, W = 2 .. 8), and 24-bit leftovers in a row-block
# with slots (the ordinary passes of this kernel see a header whose rows are the slots and the y tile together).
# name -> (generator, options on top of the family's)
SYM_MATMAT_CASES = {
    "step-127-sym": SYM_CASES["step-127-sym"][:2],
    "slots-3072": SYM_CASES["slots-3072"][:2],
    "slots-wide-cap": SYM_CASES["slots-wide-cap"][:2],
    "noslot": SYM_CASES["noslot"][:2],
    "passes-edge-sym": SYM_CASES["passes-edge-sym"][:2],
    "seg-widths": (msc.seg_widths, {}),
    "off-sym-3-runs": (lambda: sym_wide(70000, 65536, runs=True), {}),
}
SEG_WIDTHS = set(range(2, 9))
NVECS_SYM = (2, 3, 5, 8, 13, 15)            # (in one call 15 is 8 + 4 + 2 + 1 where the group is eight)
# the streams a default tune leaves, restored with the option: wide row-blocks, which the tune with it never emits
# (seg-widths on top of the four the limits call for: every width in row-blocks of up to 990 rows, group 4)
SYM_MATMAT_RESTORED = ("step-127-sym", "noslot", "slots-3072", "slots-wide-cap", "seg-widths")
# what test_limit_cases.py asks of these streams and the emitter's choices keep out of reach, with the line: nothing
SYM_MATMAT_UNREACHABLE = {}


def sym_matmat_on(case, waves=4):
    """SYM_MATMAT_ON: tuned with the option (no row-block of more than 512 rows, atomic hand-over)."""
    o = sym_options("segments", SYM_MATMAT_CASES[case][1])
    o.update({"spx.gpu.sym_matmat": "true", "spx.gpu.wave_tiles": "false", "spx.gpu.waves": str(waves)})
    return o


def sym_matmat_default(case, waves=4):
    """SYM_MATMAT_DEFAULT: what a tune without the option emits -- the hand-over pinned (spx.gpu.sym_spill=auto
    is a measurement at tune time), and the wavefront count."""
    o = sym_options("segments", SYM_MATMAT_CASES[case][1])
    o.update({"spx.gpu.sym_spill": "atomic", "spx.gpu.waves": str(waves)})
    return o


# ---- what a saved stream holds ----------------------------------------------------------------------------

def census(path, rows_from=0):
    """The figures of a saved stream that the limits are stated in (rows_from: of its row-blocks from that
    row on)."""
    s = Stream(path)
    out = {"widths": set(), "steps": {}, "front": 0, "seg0": 0, "n_pass": 0, "n_slots": 0, "noslot": 0,
           "elem0_front": 0, "pass_counts": set(), "kinds": set(), "symseg_steps": {}, "rows": 0,
           "wide_slots": 0, "wide_noslot": 0, "symseg_widths": set(), "symseg_inline": 0, "symseg_listed": 0,
           "rowblocks": []}
    for rb in s.rbs[s.rbs["row0"] >= rows_from]:
        ps = s.passes[int(rb["pass_off"]):int(rb["pass_off"]) + int(rb["n_pass"])]
        out["pass_counts"].add(int(rb["n_pass"]))
        out["n_pass"] = max(out["n_pass"], int(rb["n_pass"]))
        out["n_slots"] = max(out["n_slots"], int(rb["n_slots"]))
        out["rows"] = max(out["rows"], int(rb["n_rows"]))
        wide = int(rb["n_rows"]) > 512
        if wide:
            out["wide_slots"] = max(out["wide_slots"], int(rb["n_slots"]))
        out["kinds"] |= set(ps["kind"].tolist())
        # (rows, slots, width of the offsets, pass kinds) of every row-block
        out["rowblocks"].append((int(rb["n_rows"]), int(rb["n_slots"]), int(rb["cidx_width"]), set(ps["kind"].tolist())))
        if (ps["kind"] == PASS_GATHER).any():
            out["widths"].add(int(rb["cidx_width"]))
        for p in ps:
            if p["kind"] not in (PASS_UNIT, PASS_SYMSEG):
                continue
            sym = p["kind"] == PASS_SYMSEG
            nseg, mask = int(p["nseg"]), 0 if int(p["flags"]) & 1 else int(p["mask"])
            starts = np.array([(mask >> l) & 1 for l in range(nseg)])
            rank = int(rb["desc_off"]) + int(p["rank0"]) + (2 if sym else 1) * np.cumsum(starts)
            bits = s.descs["bits"][rank].astype(np.int64)
            front = (bits >> 9) & 8191
            out["front"] = max(out["front"], int(front.max()))
            out["seg0"] = max(out["seg0"], int(p["seg0"]))
            if int(p["elem0"]) > 0:
                out["elem0_front"] = max(out["elem0_front"], int(front.max()))
            for k, st in zip(((bits >> 22) & 7).tolist(), (bits >> 25).tolist()):
                tab = out["symseg_steps"] if sym else out["steps"]
                tab[k] = max(tab.get(k, 0), st)
            if sym:
                out["symseg_widths"].add(int(p["width"]))
                out["symseg_inline" if int(p["flags"]) & 1 else "symseg_listed"] += 1
                none = int((s.descs["col0"][rank + 1] == 0xFFFFFFFF).sum())       # (rank: per lane)
                out["noslot"] += none
                out["wide_noslot"] += none if wide else 0
    return out, s


def gather_offsets(s, rb):
    """(lane, position in the piece, offset) of every leftover of row-block `rb`'s kind-2 passes, as three
    arrays: the u16 / u16 + u8 / u32 offsets read the way SPX_LOAD_INDEX reads them."""
    L, P, O = [], [], []
    area = int(rb["cidx_off"]) * 16
    cw = int(rb["cidx_width"])
    for ps in s.passes[int(rb["pass_off"]):int(rb["pass_off"]) + int(rb["n_pass"])]:
        if ps["kind"] != PASS_GATHER:
            continue
        nseg, W, e0 = int(ps["nseg"]), int(ps["width"]), int(ps["elem0"])
        lanes = np.arange(nseg)
        sr = s.segrows[int(rb["seg_off"]) + int(ps["seg0"]) + lanes].astype(np.int64)
        plen = ((sr >> 11) & 7) + 1
        for w in range(W):
            e = e0 + w * nseg + lanes
            if cw == 3:
                off = s.cidx[area + 2 * e].astype(np.int64) | (s.cidx[area + 2 * e + 1].astype(np.int64) << 8)
                off |= s.cidx[area + int(rb["hi_off"]) * 16 + e].astype(np.int64) << 16
            else:
                off = sum(s.cidx[area + cw * e + b].astype(np.int64) << (8 * b) for b in range(cw))
            have = plen > w
            L.append(lanes[have]); P.append(np.full(int(have.sum()), w)); O.append(off[have])
    return np.concatenate(L), np.concatenate(P), np.concatenate(O)
