"""The multi-vector product (Matrix.matmat, spmv_mv_kernels.hip, the K-vector unit_passes, device_product) on
the streams test_gpu_matmat.py does not reach: x windows staged in LDS and gathered through L2 (the band cases
of matmat_cases.py, whose preconditions test_matmat_cases.py checks on the CPU), the randomised matrices and
options of test_stream_random.py, the rectangular and empty matrices of test_edge_cases.py, a single non-zero
column (no leak between the tiles, windows or carry slots of a group), every one of the 27 instantiations, and
edited / restored matrices.  Every column is checked with helpers.check_y; under spx.gpu.deterministic it must
equal the single-vector product bit for bit."""
import numpy as np
import pytest
import scipy.sparse as sp

import sparsex_amd as sx
from sparsex_amd import synth
from helpers import check_y, tune
from test_stream_random import random_matrix, random_options, random_sym_options
from test_edge_cases import MATS, OPTS, _tune as tune_rect
from test_gpu_matmat import CASES as MATMAT_CASES
import matmat_cases as mc

pytestmark = pytest.mark.gpu

NO_ONCE = {"spx.gpu.sym_once": "false", "spx.gpu.sym_segments": "false"}


# ---- 2. window passes, staged and not ---------------------------------------------------------------------

@pytest.mark.parametrize("mode", list(mc.BAND_MODES))
@pytest.mark.parametrize("name", list(mc.BANDS))
def test_band_windows_staged_and_gathered(name, mode):
    """nvec 13 = 8 + 4 + 1 and 7 = 4 + 2 + 1: the windows of the "unstaged" cases go through L2 at K = 8 and
    through LDS at K = 4 within one call.  The wavefront count is pinned in both modes (matmat_cases.BAND_MODES),
    so that the stream is the one whose windows test_matmat_cases.py measured."""
    import torch
    kw, _ = mc.BANDS[name]
    csr, a = mc.band(**kw)
    det = mode == "deterministic"
    A = mc.load_rect(sx, csr, a.shape[1], mc.band_options(mode))
    assert A.matmat_group() == 8
    assert bool(A.info().wave_tiles) == det
    ref = mc.single_vector_columns(torch, A) if det else None
    k = 0
    for nvec in (13, 7):
        for alpha, beta in mc.ALPHA_BETA:
            mc.run(torch, A, a, nvec, alpha, beta, padx=3 + k % 2, pady=6 - k % 2, ref=ref)
            k += 1


# ---- 3. random streams ------------------------------------------------------------------------------------

def _random_case(torch, seed, symmetric, opts, native):
    csr, a = random_matrix(seed, symmetric=symmetric)
    o = dict(opts)
    o["spx.gpu.waves"] = str([0, 2, 4, 8][seed % 4])
    det = seed % 3 == 0
    if det:
        o["spx.gpu.deterministic"] = "true"
    A = tune(csr, o, sym=symmetric)
    g = A.matmat_group()
    if native:
        assert g >= 2, "the K-vector kernels should run (group %d)" % g
    else:
        print("seed %d: group %d%s" % (seed, g, " (one product per column)" if g == 1 else ""))
    alpha, beta = mc.ALPHA_BETA[seed % 3]
    mc.run(torch, A, a, 15, alpha, beta, padx=1 + seed % 4, pady=2 + seed % 3,
           ref=mc.single_vector_columns(torch, A) if det else None)


@pytest.mark.parametrize("seed", range(40))
def test_general_random_matmat(seed):
    import torch
    _random_case(torch, seed, False, random_options(seed), True)


@pytest.mark.parametrize("seed", range(40, 90))
def test_symmetric_random_matmat_mirrored(seed):
    import torch
    _random_case(torch, seed, True, dict(random_options(seed), **NO_ONCE), True)


@pytest.mark.parametrize("seed", range(40, 90))
def test_symmetric_random_matmat_any_path(seed):
    """random_sym_options: tiles and read-once segments run one product per column (group 1) unless the tune opts
    in with spx.gpu.sym_matmat=true: test_gpu_random_paths.py runs these seeds through that path
    (csx_spmv_mvsym_kernel)."""
    import torch
    _random_case(torch, seed, True, random_sym_options(seed, random_options(seed)), False)


# ---- 4. shapes --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(MATS))
@pytest.mark.parametrize("opts", OPTS)
def test_rectangular_and_empty_rows_matmat(name, opts):
    import torch
    a = MATS[name]
    a.eliminate_zeros()
    a = sp.csr_matrix(a)
    a.sort_indices()
    A = tune_rect(a, opts, host_only=False)
    assert A.matmat_group() >= 2
    for nvec, pad in ((5, (2, 3)), (8, (0, 0))):
        mc.run(torch, A, a, nvec, 0.5, 0.0, padx=pad[0], pady=pad[1])
        mc.run(torch, A, a, nvec, 2.0, -0.5, padx=pad[1], pady=pad[0])


def test_empty_matrix_matmat():
    import torch
    a = sp.csr_matrix((30, 20))
    A = tune_rect(a, {}, host_only=False)
    for nvec in (5, 8):
        _, X = mc.block(torch, 20, nvec, 3, 11)
        yf, Y = mc.block(torch, 30, nvec, 1, 0, float("nan"))
        A.matmat(1.0, X, 0.0, Y)
        torch.cuda.synchronize()
        assert (Y == 0).all() and torch.isnan(yf[:, 30:]).all()
        yf, Y = mc.block(torch, 30, nvec, 1, 101)
        y0 = Y.clone()
        A.matmat(1.0, X, 3.0, Y)
        torch.cuda.synchronize()
        assert torch.equal(Y, 3.0 * y0) and torch.isnan(yf[:, 30:]).all()


# ---- tunes shared by the tests below ----------------------------------------------------------------------

SHARED = {
    "long-rows": (mc.long_rows, mc.NOSAMPLE, False),           # carry slots and the fix-up kernel
    "sym-no-once": (MATMAT_CASES["sym-no-once"][0], dict(mc.NOSAMPLE, **NO_ONCE), True),
    "phases-c2": (MATMAT_CASES["phases-c2"][0], MATMAT_CASES["phases-c2"][1], False),   # the scale kernel, atomics
}
EDITED = {
    "cant": (lambda: synth.syn_cant(0.05), mc.NOSAMPLE, False),
    "sym-no-once": SHARED["sym-no-once"],
}


@pytest.fixture(scope="module")
def tuned():
    cache = {}

    def get(name):
        if name not in cache:
            gen, opts, sym = SHARED[name]
            csr = gen()
            cache[name] = (csr, tune(csr, opts, sym=sym))
        return cache[name]
    yield get
    cache.clear()
    sx.options_reset()


# ---- 5. column isolation ----------------------------------------------------------------------------------

@pytest.mark.parametrize("beta", [0.0, 0.25])
@pytest.mark.parametrize("name", ["long-rows", "sym-no-once", "phases-c2"])
def test_a_single_column_of_x_reaches_a_single_column_of_y(tuned, name, beta):
    """X is zero but for column j -- the first, a middle and the last vector of a group of 8, and the lone
    ninth: every other column of Y is beta * y0 exactly (numeric ==, so that -0.0 passes); a leak between the
    tiles, windows or carry slots of a group may be far too small for the fp64 bound."""
    import torch
    csr, A = tuned(name)
    n = csr[3]
    assert A.matmat_group() >= 2
    nvec = 9
    y0 = np.stack([synth.random_x(n, seed=700 + i) for i in range(nvec)])
    want = beta * y0
    for j in (0, 3, 7, 8):
        xj = synth.random_x(n, seed=40 + j)
        xf = torch.full((nvec, n + 2), float("nan"), dtype=torch.float64, device="cuda")
        X = xf[:, :n]
        X.zero_()
        X[j] = torch.from_numpy(xj)
        yf, Y = mc.block(torch, n, nvec, 5, 0, float("nan"))
        if beta != 0.0:
            Y.copy_(torch.from_numpy(y0))
        A.matmat(-1.5, X, beta, Y)
        torch.cuda.synchronize()
        Yh = Y.cpu().numpy()
        for i in range(nvec):
            if i != j:
                bad = np.flatnonzero(~(Yh[i] == want[i]))
                assert bad.size == 0, "column %d of X reached column %d of Y (%d rows, first %d: %r, not %r)" % (
                    j, i, bad.size, bad[0], Yh[i][bad[0]], want[i][bad[0]])
        check_y(csr, xj, Yh[j], -1.5, beta, y0[j] if beta != 0.0 else None)
        assert torch.isnan(yf[:, n:]).all()


# ---- 6. which instantiations ran --------------------------------------------------------------------------

ALL_KERNELS = {(f, K, w) for f in mc.FAMILIES for K in (2, 4, 8) for w in mc.KERNEL_WAVES}
# instantiations that no option reaches, each with the line that makes it so: none
UNREACHABLE = {}


@pytest.fixture(scope="module")
def kernel_runs():
    """(matrix, family, waves) -> the (family, K, waves) instantiations that ran, each run checked."""
    import torch
    done, mats = {}, {}

    def ensure(matrix, family, waves):
        key = (matrix, family, waves)
        if key in done:
            return done[key]
        if matrix not in mats:
            mats[matrix] = mc.KERNEL_MATRICES[matrix]()
        csr, a = mats[matrix]
        A = mc.load_rect(sx, csr, a.shape[1], mc.kernel_options(family, waves))
        inf, g = A.info(), A.matmat_group()
        assert g == mc.KERNEL_TUNES[(matrix, family)]
        # launch_rowblocks_mv: accum where the column slices run in one launch, else det where a tile per
        # wavefront is kept, else plain; launch_spmv_mv: the matrix' wavefront count
        ran_family = "accum" if inf.col_slices > 1 else "det" if inf.wave_tiles else "plain"
        ran = set()
        for k, nvec in enumerate((2, 4, 8)):
            alpha, beta = mc.ALPHA_BETA[k]
            mc.run(torch, A, a, nvec, alpha, beta, padx=1, pady=2,
                   ref=mc.single_vector_columns(torch, A) if ran_family == "det" else None)
            ran.add((ran_family, min(g, nvec), int(inf.waves)))
        done[key] = ran
        return ran
    yield ensure
    done.clear()
    mats.clear()
    sx.options_reset()


@pytest.mark.parametrize("waves", mc.KERNEL_WAVES)
@pytest.mark.parametrize("matrix,family", list(mc.KERNEL_TUNES))
def test_pinned_family_and_waves_run(kernel_runs, matrix, family, waves):
    g = mc.KERNEL_TUNES[(matrix, family)]
    assert kernel_runs(matrix, family, waves) == {(family, K, waves) for K in (2, 4, 8) if K <= g}


def test_all_27_instantiations_ran(kernel_runs):
    seen = set()
    for (matrix, family) in mc.KERNEL_TUNES:
        for waves in mc.KERNEL_WAVES:
            seen |= kernel_runs(matrix, family, waves)
    assert len(ALL_KERNELS) == 27
    missing = ALL_KERNELS - seen - set(UNREACHABLE)
    assert not missing, "instantiations that never ran: %s" % sorted(missing)
    assert not (set(UNREACHABLE) & seen), "listed as unreachable, but ran"


# ---- 7. edited and restored matrices ----------------------------------------------------------------------

@pytest.mark.parametrize("name", ["cant", "sym-no-once"])
def test_set_entry_save_restore_matmat(tmp_path, name):
    import torch
    gen, opts, sym = EDITED[name]
    csr = gen()
    rp, ci, va, n = csr
    A = tune(csr, opts, sym=sym)
    g = A.matmat_group()
    assert g >= 2
    mc.run(torch, A, mc.to_scipy(csr), 13, 0.5, 0.0, padx=3, pady=5)
    rows = np.repeat(np.arange(n), np.diff(rp))
    rng = np.random.RandomState(5)
    va2 = va.copy()
    for e in rng.choice(rp[-1], size=25, replace=False):
        r, c = int(rows[e]), int(ci[e])
        A.set_entry(r, c, 3.5)
        va2[e] = 3.5
        if sym:
            va2[rp[c] + int(np.searchsorted(ci[rp[c]:rp[c + 1]], r))] = 3.5
    a2 = sp.csr_matrix((va2, ci, rp), shape=(n, n))
    mc.run(torch, A, a2, 13, 2.0, -0.5, padx=3, pady=5)
    f = str(tmp_path / "m.spx")
    A.save(f)
    A.destroy()
    sx.options_reset()
    B = sx.mat_restore(f)
    assert B.matmat_group() == g
    mc.run(torch, B, a2, 13, 2.0, -0.5, padx=3, pady=5)
    mc.run(torch, B, a2, 8, 0.5, 0.0, padx=1, pady=0)
    B.destroy()
