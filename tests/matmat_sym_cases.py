"""Cases and helpers shared by the tests of the multi-vector product on symmetric streams whose values are read
once (spx.gpu.sym_matmat; test_matmat_sym_host.py on the CPU, test_gpu_matmat_sym.py on the GPU): symmetric
matrices that make the emitter produce tiles, read-once segments, both, segments without a slot, rows shared
between row-blocks and a core small enough for a group of eight; and what a saved stream must look like.
seg_widths and expected_mvsym_group also serve the limit cases (limit_cases.py, test_gpu_stream_limits.py)."""
import numpy as np
import scipy.sparse as sp

from sparsex_amd import synth
from matmat_cases import NOSAMPLE
from stream_decode import Stream

NVECS = (1, 2, 3, 5, 8, 13)
PASS_SYMTILE, PASS_SYMSEG = 3, 5
NO_SLOT = 0xFFFFFFFF
MAX_RB_ROWS = 512                  # SPX_MAX_RB_ROWS of gpu_format.h
MAX_CORE = 512 + 3072              # ... + SPX_MAX_TILE_SLOTS: slots + y tile of a row-block, in doubles


def options(waves=4, more=None):
    """What every GPU case sets (the tune is symmetric: helpers.tune(..., sym=True)), and `more` on top."""
    o = dict(NOSAMPLE, **{"spx.gpu.sym_matmat": "true", "spx.gpu.wave_tiles": "false", "spx.gpu.waves": str(waves)})
    o.update(more or {})
    return o


def _symmetric(n, r, c, seed):
    """CSR tuple + scipy matrix of the symmetric n x n matrix with the pattern (r, c) mirrored and a full diagonal;
    values uniform in (-1, 1) on the stored triangle."""
    rng = np.random.RandomState(seed)
    r, c = np.asarray(r, dtype=np.int64), np.asarray(c, dtype=np.int64)
    lo = sp.coo_matrix((np.ones(r.size), (np.maximum(r, c), np.minimum(r, c))), shape=(n, n)).tocsr()
    lo.sum_duplicates()
    lo = sp.tril(lo, k=-1).tocsr()
    lo.data = rng.uniform(-1, 1, lo.nnz)
    m = (lo + lo.T + sp.diags(rng.uniform(1, 2, n))).tocsr()
    m.sort_indices()
    return (m.indptr.astype(np.int32), m.indices.astype(np.int32), m.data.copy(), n), m


def _blocks(bi, bj):
    """(rows, cols) of the dense 8x8 blocks (bi[k], bj[k])."""
    a, b = np.meshgrid(np.arange(8), np.arange(8), indexing="ij")
    r = (8 * np.asarray(bi)[:, None] + a.ravel()[None, :]).ravel()
    c = (8 * np.asarray(bj)[:, None] + b.ravel()[None, :]).ravel()
    return r, c


def _runs(rows, starts, width=3):
    r = np.repeat(np.asarray(rows), width)
    c = (np.asarray(starts)[:, None] + np.arange(width)[None, :]).ravel()
    return r, c


def tiles_and_segments():
    """n = 6144: dense 8x8 blocks on the two block diagonals under the main one, and in every row r >= 3072 a run
    of three columns far in front of the diagonal."""
    n = 6144
    nb = n // 8
    bi = np.concatenate([np.arange(1, nb), np.arange(2, nb)])
    bj = np.concatenate([np.arange(0, nb - 1), np.arange(0, nb - 2)])
    r1, c1 = _blocks(bi, bj)
    rows = np.arange(3072, n)
    r2, c2 = _runs(rows, (rows * 5) % 2000)
    return _symmetric(n, np.concatenate([r1, r2]), np.concatenate([c1, c2]), 5)


def segments_without_slot():
    """n = 20000: every row r >= 8000 carries a run of three columns whose start is spread over [0, 6000) -- eleven
    columns on from the row above -- so that the 512 rows of a row-block (spx.gpu.rowblock_elems lets them fill up)
    touch more column groups than the 384 its slots hold."""
    n = 20000
    rows = np.arange(8000, n)
    return _symmetric(n, *_runs(rows, (rows * 11) % 5997), seed=6)


def arrow():
    """n = 40000: the diagonal, runs of three columns in a few hundred rows and a last row with 30000 nonzeros
    (a row shared between row-blocks)."""
    n = 40000
    rng = np.random.RandomState(7)
    rows = np.arange(1000, n - 1, 97)
    r1, c1 = _runs(rows, rows - 600)
    c2 = np.sort(rng.choice(n - 1, 30000, replace=False))
    return _symmetric(n, np.concatenate([r1, np.full(c2.size, n - 1)]), np.concatenate([c1, c2]), 8)


def block_banded():
    """512 block rows of dense 8x8 blocks within +-8 block columns: few slots per row-block, a small core."""
    nb = 512
    bi, bj = [], []
    for d in range(0, 9):
        bi.append(np.arange(d, nb))
        bj.append(np.arange(0, nb - d))
    return _symmetric(8 * nb, *_blocks(np.concatenate(bi), np.concatenate(bj)), seed=9)


SEG_WIDTHS_N, SEG_WIDTHS_FIRST = 4096, 1024


def seg_widths(width=None):
    """n = 4096: every row r >= 1024 holds one run in front of the diagonal, 2 + (r // 128) % 11 columns wide (2 to
    12, the same for 128 rows in turn; the emitter cuts a run of more than eight columns into chunks), starting at
    column 8 * ((5 r) % 64) + r % 3: read-once segments of every width the kernels are instantiated for.  `width`:
    that width in every row instead (what test_limit_cases.py regenerates the case with, to see its check fail)."""
    n = SEG_WIDTHS_N
    rows = np.arange(SEG_WIDTHS_FIRST, n)
    wid = 2 + (rows // 128) % 11 if width is None else np.full(rows.size, width)
    start = 8 * ((5 * rows) % 64) + rows % 3
    r = np.repeat(rows, wid)
    c = np.repeat(start, wid) + (np.arange(r.size) - np.repeat(np.cumsum(wid) - wid, wid))
    return _symmetric(n, r, c, seed=10)


def _from_synth(csr):
    rp, ci, va, n = csr
    return csr, sp.csr_matrix((va, ci, rp), shape=(n, n))


# name -> (generator of (csr tuple, scipy matrix), options on top of options())
MATRICES = {
    "tiles": (lambda: _from_synth(synth.syn_nd24k(0.05)), {}),
    "segments": (lambda: _from_synth(synth.syn_nlpkkt(20)), {"spx.gpu.sym_segments": "true"}),
    "tiles-and-segments": (tiles_and_segments, {"spx.gpu.sym_segments": "true"}),
    "no-slot": (segments_without_slot, {"spx.gpu.sym_segments": "true", "spx.gpu.rowblock_elems": "4096"}),
    "arrow": (arrow, {"spx.gpu.sym_segments": "true"}),
    "block-banded": (block_banded, {}),
}


def case_options(name, waves=4):
    return options(waves, MATRICES[name][1])


def slotless_groups(s):
    """Number of read-once segment groups (descriptors of SPX_PASS_SYMSEG passes) of the stream `s` whose slot
    entry is SPX_NO_SLOT: their lanes add straight to y."""
    n = 0
    for rb in s.rbs:
        d0 = int(rb["desc_off"])
        for ps in s.passes[int(rb["pass_off"]):int(rb["pass_off"]) + int(rb["n_pass"])]:
            if ps["kind"] != PASS_SYMSEG:
                continue
            mask = 0 if int(ps["flags"]) & 1 else int(ps["mask"])
            starts = np.array([(mask >> l) & 1 for l in range(int(ps["nseg"]))])
            rank = np.unique(int(ps["rank0"]) + 2 * np.cumsum(starts))
            n += int((s.descs[d0 + rank + 1]["col0"] == NO_SLOT).sum())
    return n


MVSYM_LDS_BUDGET = 80 * 1024      # of device_runtime.cpp, in bytes


def expected_mvsym_group(s):
    """The group a device copy of the stream `s`, tuned or restored under spx.gpu.sym_matmat=true with one tile per
    workgroup, serves (sparsex_hip.h, device_mv_group of device_runtime.cpp): 1 unless the stream is symmetric, hands
    over with atomics and holds read-once passes; else the widest K of 8, 4, 2 of which that many copies of
    {slots, y tile} of the largest row-block, and the first columns of the slot groups of the one with the most
    slots, fit 80 KB of LDS; 1 where not even two do."""
    if not (s.symmetric and s.sym_atomic and len(s.rbs)):
        return 1
    if not np.isin(s.passes["kind"], (PASS_SYMTILE, PASS_SYMSEG)).any():
        return 1
    core = int((s.rbs["n_rows"].astype(np.int64) + s.rbs["n_slots"]).max())
    groups = (int(s.rbs["n_slots"].max()) + 7) // 8
    for K in (8, 4, 2):
        if K * core * 8 + groups * 4 <= MVSYM_LDS_BUDGET:
            return K
    return 1


def check_stream_fits(path, m):
    """A stream saved under spx.gpu.sym_matmat: atomic hand-over, no wide row-blocks, a core that K copies of fit
    the LDS, and -- decoded lane by lane -- the product of the matrix `m`.  Returns the Stream."""
    s = Stream(path)
    assert s.symmetric and s.sym_atomic == 1
    assert int(s.rbs["n_rows"].max()) <= MAX_RB_ROWS
    assert int((s.rbs["n_rows"].astype(np.int64) + s.rbs["n_slots"]).max()) <= MAX_CORE
    x = synth.random_x(m.shape[0])
    assert np.allclose(s.matvec(x), m @ x, rtol=1e-12, atol=1e-13)
    return s
