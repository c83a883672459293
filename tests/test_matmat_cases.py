"""The preconditions of the multi-vector GPU tests (test_gpu_matmat_streams.py), checked on the CPU: every case
of matmat_cases.py is tuned host-only, saved and decoded (stream_decode.Stream), and must hold the passes,
windows and row-blocks its GPU test relies on -- so that a case cannot go vacuous when the emitter changes."""
import numpy as np
import pytest

import sparsex_amd as sx
from helpers import tune
from stream_decode import Stream
from test_stream_random import random_matrix, random_options
import matmat_cases as mc


def _saved(A, tmp_path):
    f = str(tmp_path / "m.spx")
    A.save(f)
    return f


def test_band_generator():
    csr, m = mc.band(500, 40, 0.2, ncols=800, seed=3)
    rp, ci, va, n = csr
    assert m.shape == (500, 800) and n == 500 and rp[-1] == m.nnz == ci.size == va.size
    assert 0 < m.nnz <= int(500 * 81 * 0.2)
    r = np.repeat(np.arange(500), np.diff(rp))
    assert (np.abs(ci - r * 800 // 500) <= 40).all() and ci.min() >= 0 and ci.max() < 800
    assert (np.abs(va) < 1).all() and m.has_sorted_indices
    assert np.unique(r.astype(np.int64) * 800 + ci).size == m.nnz
    again = mc.band(500, 40, 0.2, ncols=800, seed=3)[0]
    assert all(np.array_equal(a, b) for a, b in zip(csr[:3], again[:3]))
    assert mc.band(300, 10, 0.5)[1].shape == (300, 300)


@pytest.mark.parametrize("name", list(mc.BANDS))
def test_band_streams_hold_the_windows_their_gpu_tests_need(tmp_path, name):
    kw, what = mc.BANDS[name]
    csr, m = mc.band(**kw)
    assert m.nnz <= 1500000
    for mode in mc.BAND_MODES:
        A = mc.load_rect(sx, csr, m.shape[1], mc.band_options(mode), host_only=True)
        n4, xwin, rows = mc.census(_saved(A, tmp_path))
        print("%s %s: %d kind-4 passes, largest window %d doubles, largest row-block %d rows" % (name, mode, n4, xwin, rows))
        assert n4 > 0, "no SPX_PASS_GATHER_LDS passes: the window paths of mv_body would not run"
        if what == "unstaged":
            assert xwin > mc.NEVER_STAGED_AT_8, "eight windows fit the LDS budget: K = 8 would stage them"
            # ... and K = 4 stages them, even with eight copies of the tiles: both paths within one call
            assert 4 * (8 * rows + xwin) <= mc.MV_LDS_BUDGET_DOUBLES
        else:
            assert 8 * (8 * rows + xwin) <= mc.MV_LDS_BUDGET_DOUBLES, "K = 8 would not stage the windows"


@pytest.mark.parametrize("name", list(mc.GENERAL))
def test_census_of_the_general_cases(tmp_path, name):
    gen, opts = mc.GENERAL[name]
    A = tune(gen(), opts, host_only=True)
    print("%s: %d kind-4 passes, largest window %d doubles, largest row-block %d rows" % ((name,) + mc.census(_saved(A, tmp_path))))


def test_random_general_streams_hold_small_and_large_windows(tmp_path):
    """Seeds 0-39 of test_stream_random.random_matrix with random_options, as test_gpu_matmat_streams.py runs
    them: at least one stream whose windows are never staged at K = 8, at least one whose windows are."""
    large, small = [], []
    for seed in range(40):
        csr, _ = random_matrix(seed, symmetric=False)
        A = tune(csr, random_options(seed), host_only=True)
        n4, xwin, rows = mc.census(_saved(A, tmp_path))
        if n4 and xwin > mc.NEVER_STAGED_AT_8:
            large.append(seed)
        elif n4:
            small.append(seed)
    print("windows above %d doubles: seeds %s; below: seeds %s" % (mc.NEVER_STAGED_AT_8, large, small))
    assert large and small


@pytest.mark.parametrize("matrix,family", list(mc.KERNEL_TUNES))
def test_kernel_table_groups(tmp_path, matrix, family):
    """The group every tune of the instantiation table gets (device_mv_group: the widest K whose K * copies
    tiles fit the budget; copies is the wavefront count for the det family, at most 8, else 1): the K = 8
    instantiations run only where it is 8."""
    csr, m = mc.KERNEL_MATRICES[matrix]()
    A = mc.load_rect(sx, csr, m.shape[1], mc.kernel_options(family, 8), host_only=True)
    s = Stream(_saved(A, tmp_path))
    rows = int(s.rbs["n_rows"].max())
    kinds = set()
    for rb in s.rbs:
        kinds |= set(s.passes[int(rb["pass_off"]):int(rb["pass_off"]) + int(rb["n_pass"])]["kind"].tolist())
    print("%s %s: pass kinds %s, largest row-block %d rows" % (matrix, family, sorted(kinds), rows))
    assert mc.expected_group(rows, 8 if family == "det" else 1) == mc.KERNEL_TUNES[(matrix, family)]
    if matrix != "cant":
        assert mc.PASS_GATHER_LDS in kinds
