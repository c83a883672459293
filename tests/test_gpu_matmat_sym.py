"""The multi-vector product on symmetric streams whose values are read once (spx.gpu.sym_matmat,
csx_spmv_mvsym_kernel) on the GPU: every column against the CSR product (helpers.check_y -- the products go
through atomics, so nothing is compared bit for bit) on streams of tiles, of read-once segments, of both, with
segments that found no slot, with rows shared between row-blocks and with a group of eight; a row slice, a
captured graph, edits with save / restore, and the settings that fall back to one product per column.  Tuned
matrices are shared per module."""
import numpy as np
import pytest
import scipy.sparse as sp

import sparsex_amd as sx
from sparsex_amd import synth
from helpers import tune
from matmat_cases import ALPHA_BETA, NOSAMPLE, block as _block, run
from matmat_sym_cases import MATRICES, NVECS, case_options, options, slotless_groups
from stream_decode import Stream

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tuned():
    mats, cache = {}, {}

    def get(name, waves=4):
        key = (name, waves)
        if name not in mats:
            mats[name] = MATRICES[name][0]()
        if key not in cache:
            cache[key] = tune(mats[name][0], case_options(name, waves), sym=True)
        return mats[name][0], mats[name][1], cache[key]
    yield get
    cache.clear()
    sx.options_reset()


def _all_nvecs(torch, A, m, padx=None):
    """NVECS with the (alpha, beta) pairs in turn; NaN in Y for beta = 0, NaN padding behind every vector."""
    for k, nvec in enumerate(NVECS):
        alpha, beta = ALPHA_BETA[k % 3]
        run(torch, A, m, nvec, alpha, beta, padx=(3 if k % 2 else 1) if padx is None else padx, pady=5 if k % 2 else 2)


def test_tiles(tuned):
    import torch
    csr, m, A = tuned("tiles")
    assert A.info().sym_tiles == 2
    assert A.matmat_group() >= 2, "tiles under spx.gpu.sym_matmat serve a group (group %d)" % A.matmat_group()
    assert csr[3] % 2 == 0
    # ldx = n + 3 is odd: the vectors 1, 3, ... of X are 8-byte aligned only
    for k, nvec in enumerate(NVECS):
        alpha, beta = ALPHA_BETA[k % 3]
        run(torch, A, m, nvec, alpha, beta, padx=3, pady=5)
    for k, nvec in enumerate(NVECS):
        alpha, beta = ALPHA_BETA[(k + 1) % 3]
        run(torch, A, m, nvec, alpha, beta, padx=0, pady=0)


# (info().waves is what the single-vector product runs with.  csx_spmv_mvsym_kernel runs with it where a launch takes
# at most 40 KB of LDS and with eight wavefronts above that: on "segments" K = 2 and 4 run at waves 2, 4 and 8 and
# K = 8 at eight only; on "tiles-and-segments" and "tiles" K = 8 stays within 40 KB and runs at the pinned count.)
@pytest.mark.parametrize("waves", [2, 4, 8])
def test_segments_without_tiles(tuned, waves):
    import torch
    _, m, A = tuned("segments", waves)
    assert A.info().sym_segments == 2 and A.info().waves == waves
    assert A.matmat_group() >= 2
    _all_nvecs(torch, A, m)


@pytest.mark.parametrize("waves", [2, 4, 8])
def test_tiles_and_segments_in_one_stream(tuned, waves):
    import torch
    _, m, A = tuned("tiles-and-segments", waves)
    assert A.info().sym_segments == 1 and A.info().waves == waves
    assert A.matmat_group() >= 2
    _all_nvecs(torch, A, m)


def test_segments_without_a_slot(tuned, tmp_path):
    import torch
    csr, m, A = tuned("no-slot")
    # the host-only stream of the same tune holds segment groups that add straight to y
    H = tune(csr, case_options("no-slot"), sym=True, host_only=True)
    f = str(tmp_path / "m.spx")
    H.save(f)
    assert slotless_groups(Stream(f)) >= 1
    assert A.info().sym_segments == 2 and A.matmat_group() >= 2
    _all_nvecs(torch, A, m)


def test_rows_shared_between_row_blocks(tuned):
    """... and both routes of the window gathers: the last row's x window (4096 doubles) is staged in LDS for a group
    of two (nvec 2, 3) and gathered through L2 for groups of four and eight, whose windows do not fit 80 KB."""
    import torch
    _, m, A = tuned("arrow")
    assert A.info().n_shared_rows > 0
    assert A.matmat_group() == 8
    _all_nvecs(torch, A, m)


def test_group_of_eight(tuned):
    import torch
    _, m, A = tuned("block-banded")
    assert A.info().sym_tiles == 2
    assert A.matmat_group() == 8
    for k, nvec in enumerate((8, 13)):
        for alpha, beta in ALPHA_BETA:
            run(torch, A, m, nvec, alpha, beta, padx=3 * k, pady=k)


def test_row_slice_writes_the_rows_of_the_single_product():
    import torch
    N = 12
    n = synth.nlpkkt_nrows(N)
    lo, hi = n // 4, (3 * n) // 4
    rl, cl, vl, _ = synth.syn_nlpkkt_rows(N, lo, hi)
    sx.options_reset()
    # (spx.gpu.sym_segments=true: left to itself a stencil of this size is held with its mirror image and the
    # ordinary multi-vector kernels would run)
    opts = options(more={"spx.rt.row_offset": str(lo), "spx.rt.global_rows": str(n), "spx.matrix.symmetric": "true",
                         "spx.gpu.sym_segments": "true"})
    for k, v in opts.items():
        sx.option_set(k, v)
    inp = sx.input_load_csr(rl, cl, vl, hi - lo, n)
    A = sx.mat_tune(inp)
    assert A.nrows == n
    assert A.info().sym_segments == 2 and A.matmat_group() >= 2
    s = torch.cuda.current_stream().cuda_stream
    for nvec, beta in ((3, 0.0), (5, 0.5), (8, 0.5)):
        _, X = _block(torch, A.ncols, nvec, 0, 7)
        _, Y = _block(torch, A.nrows, nvec, 0, 0, 123.0)
        Y1 = Y.clone()
        A.matmat(0.5, X, beta, Y)
        for j in range(nvec):
            A.hip_matvec_kernel(0.5, X[j].data_ptr(), beta, Y1[j].data_ptr(), s)
        torch.cuda.synchronize()
        y, y1 = Y.cpu().numpy(), Y1.cpu().numpy()
        assert np.array_equal(y == 123.0, y1 == 123.0), "not the rows the single-vector product writes"
        assert np.allclose(y, y1, rtol=1e-13, atol=1e-13)
    del A
    inp.destroy()
    sx.options_reset()


def test_captured_matmat_replays(tuned):
    import torch
    _, a, A = tuned("segments")
    n = a.shape[0]
    assert A.matmat_group() >= 2
    nvec = 5
    _, X = _block(torch, n, nvec, 2, 51)
    Y = torch.zeros((nvec, n), dtype=torch.float64, device="cuda")
    A.matmat(0.5, X, 0.0, Y)                                        # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(4):                                          # Y <- 0.5 A X + 0.25 Y, four times
            A.matmat(0.5, X, 0.25, Y)
    for rep in range(3):                                            # new inputs, same graph
        for j in range(nvec):
            X[j] = torch.from_numpy(synth.random_x(n, seed=500 + 10 * rep + j))
        Y.fill_(float(rep))
        g.replay()
        torch.cuda.synchronize()
        Xh, Yh = X.cpu().numpy(), Y.cpu().numpy()
        for j in range(nvec):
            ref = np.full(n, float(rep))
            for _ in range(4):
                ref = 0.5 * (a @ Xh[j]) + 0.25 * ref
            assert np.allclose(Yh[j], ref, rtol=1e-12, atol=1e-13)


def test_edits_and_restore(tmp_path):
    import torch
    csr, m = MATRICES["tiles-and-segments"][0]()
    rp, ci, va, n = csr
    A = tune(csr, case_options("tiles-and-segments"), sym=True)
    g = A.matmat_group()
    assert g >= 2
    rng = np.random.RandomState(17)
    m2 = m.tolil(copy=True)
    for r in rng.choice(np.arange(100, n), 25, replace=False):
        below = ci[rp[r]:rp[r + 1]]
        below = below[below < r]
        c = int(below[rng.randint(below.size)])
        v = float(rng.uniform(-2, 2))
        A.set_entry(int(r), c, v)
        m2[int(r), c] = v
        m2[c, int(r)] = v
    m2 = m2.tocsr()
    m2.sort_indices()
    run(torch, A, m2, 13, 2.0, -0.5, padx=3, pady=1)
    f = str(tmp_path / "m.spx")
    A.save(f)
    sx.options_reset()
    sx.option_set("spx.gpu.sym_matmat", "true")
    B = sx.mat_restore(f)
    assert B.matmat_group() == g
    run(torch, B, m2, 13, 0.5, 0.0, padx=3, pady=1)
    sx.options_reset()
    C = sx.mat_restore(f)
    assert C.matmat_group() == 1
    run(torch, C, m2, 5, 2.0, -0.5, padx=3, pady=1)
    sx.options_reset()


@pytest.mark.parametrize("name,more", [("deterministic", {"spx.gpu.deterministic": "true"}),
                                       ("lists", {"spx.gpu.sym_spill": "lists"}),
                                       ("off", {"spx.gpu.sym_matmat": "false"})])
def test_fallbacks_run_one_product_per_column(name, more):
    import torch
    csr, m = MATRICES["tiles"][0]()
    A = tune(csr, dict(case_options("tiles"), **more), sym=True)
    assert A.matmat_group() == 1
    for k, nvec in enumerate((3, 8)):
        alpha, beta = ALPHA_BETA[k]
        run(torch, A, m, nvec, alpha, beta, padx=3, pady=1)
    sx.options_reset()


def test_a_general_tune_keeps_its_group():
    import torch
    csr = synth.syn_cant(0.05)
    off = tune(csr, dict(NOSAMPLE, **{"spx.gpu.waves": "4", "spx.gpu.wave_tiles": "false"}))
    g = off.matmat_group()
    del off
    A = tune(csr, options())
    assert g >= 2 and A.matmat_group() == g
    run(torch, A, sp.csr_matrix((csr[2], csr[1], csr[0]), shape=(csr[3], csr[3])), 5, 0.5, 0.0, padx=3, pady=1)
    sx.options_reset()
