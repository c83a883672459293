"""dist_cases.py on the CPU: every case tuned host-only, slice by slice, and looked at through the decoded stream
(stream_decode.Stream), the plans of the pipelined read-once kernel and of the unit windows, and info() -- each
case reaches on some rank what it is named for, the cuts are what they are named for, and the references are
consistent with each other and with the decoder.  test_gpu_slices.py and test_gpu_dist_step.py rely on it."""
import socket

import numpy as np
import pytest

import sparsex_amd as sx
from sparsex_amd import synth
import dist_cases as dc
from stream_decode import Stream

PASS_UNIT, PASS_SYMTILE, PASS_SYMSEG = 0, 3, 5


@pytest.fixture(scope="module")
def loaded():
    cache = {}

    def get(case):
        if case not in cache:
            csr = dc.matrix(case)
            cache[case] = (csr, dc.to_scipy(csr), dc.bounds(case, csr))
        return cache[case]
    yield get
    cache.clear()


def _slice(tmp_path, case, family, sym, csr, lo, hi, decode=True):
    A = dc.tune_rows(csr, lo, hi, dc.family_options(case, family, sym), sym, host_only=True)
    inf = A.info()
    assert (inf.row_lo, inf.row_hi) == (lo, hi) and A.nrows == csr[3] and not inf.on_device
    s = None
    if decode:
        f = str(tmp_path / "slice.spx")
        A.save(f)
        s = Stream(f)
    return A, inf, s


@pytest.mark.parametrize("case", list(dc.CASES))
def test_cuts_are_what_they_are_named_for(loaded, case):
    csr, m, cuts = loaded(case)
    _, world, kind, _, _, _ = dc.CASES[case]
    n = csr[3]
    assert len(cuts) == world + 1 and cuts[0] == 0 and cuts[-1] == n and all(a < b for a, b in zip(cuts, cuts[1:]))
    balanced = dc.cut(csr, world, "balanced")
    if kind == "shifted":
        assert [c - 3 for c in cuts[1:-1]] == balanced[1:-1]
    if kind == "one-row":
        assert cuts[-2] == n - 1
    if case in dc.MISALIGNED:
        assert all(c % 8 for c in cuts[1:-1]), "a boundary is a multiple of 8: it cuts no block row"
    # symmetric and with a diagonal: what the symmetric tunes and symmetric_part assume
    assert abs(m - m.T).max() == 0 and (m.diagonal() > 0).all()


@pytest.mark.parametrize("case", dc.MISALIGNED)
def test_tiles_on_both_sides_of_a_misaligned_boundary(tmp_path, loaded, case):
    """Dense 8x8 tiles in the slice in front of every boundary and in the one behind it, and the block row the
    boundary runs through holds nonzeros on both sides."""
    csr, m, cuts = loaded(case)
    tiles = []
    for r in range(len(cuts) - 1):
        A, inf, s = _slice(tmp_path, case, "lists", True, csr, cuts[r], cuts[r + 1])
        tiles.append(int((s.passes["kind"] == PASS_SYMTILE).sum()))
        assert inf.sym_tiles == 1
        A.destroy()
    assert all(t > 0 for t in tiles), tiles
    low = dc.sp.tril(m, k=-1).tocsr()
    for c in cuts[1:-1]:
        b = c - c % 8
        assert low[b:c].nnz > 0 and low[c:b + 8].nnz > 0


def test_thin_mirror_case_has_a_list(tmp_path, loaded):
    case = dc.THIN_MIRROR
    csr, m, cuts = loaded(case)
    lo, hi = cuts[-2], cuts[-1]
    A, inf, s = _slice(tmp_path, case, "lists", True, csr, lo, hi)
    assert s.mirror_rows.size > 0 and s.mirror_rows.max() < lo
    r, c = dc.thin_mirror_entry(csr, lo, s.mirror_rows)
    assert c < lo <= r and c in set(s.mirror_rows.tolist())
    assert A.get_entry(r, c) == m[r, c] == A.get_entry(c, r)
    A.destroy()
    # (the smallest edge: one below, the last slice has no list)
    small = synth.syn_kkt2f_rows(dc.THIN_EDGE - 1)
    b = dc.cut(small, 3, "balanced")
    B, _, s2 = _slice(tmp_path, case, "lists", True, small, b[-2], b[-1])
    assert s2.mirror_rows.size == 0
    B.destroy()


@pytest.mark.parametrize("case", dc.PIPELINED)
def test_pipeline_case_has_passes_of_its_own(tmp_path, loaded, case):
    csr, m, cuts = loaded(case)
    sx_passes = []
    for r in range(len(cuts) - 1):
        A, inf, _ = _slice(tmp_path, case, "pipeline", True, csr, cuts[r], cuts[r + 1], decode=False)
        _, n_sx, cnt = A.sym_pipeline()
        sx_passes.append(cnt["sx_passes"])
        assert cnt["sx_passes"] <= cnt["sym_passes"] and (cnt["sym_passes"] > 0) == (inf.sym_segments > 0)
        A.destroy()
    assert max(sx_passes) > 0, sx_passes


def _overlap_worker(rank, world, port, case, ret):
    import os
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from sparsex_amd.dist_torch import torch_transport
        csr = dc.matrix(case)
        cuts = dc.bounds(case, csr)
        A = dc.tune_rows(csr, cuts[rank], cuts[rank + 1], dc.family_options(case, "plain", False), host_only=True)
        A.dist_attach(torch_transport(rank, world))
        halo = A.dist_halo()
        ret[rank] = (int(A.info().n_rowblocks), len(A.dist_rounds()), int(halo["recv_cols"].size))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("case", dc.OVERLAP)
def test_overlap_case_has_the_row_blocks_and_the_rounds(case):
    """device_plan_chunks refuses fewer than 64 row-blocks: every rank's slice has them (smaller row-blocks, not
    a larger matrix), the plan has rounds, and every rank has a halo to move in them."""
    import torch.multiprocessing as mp
    world = dc.CASES[case][1]
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    ret = mp.Manager().dict()
    mp.spawn(_overlap_worker, args=(world, port, case, ret), nprocs=world, join=True)
    for r in range(world):
        n_rb, rounds, halo = ret[r]
        assert n_rb >= 64 and rounds >= 2 and halo > 0, (r, ret[r])


@pytest.mark.parametrize("case", [c for c, v in dc.CASES.items() if "unit-windows" in v[4]])
def test_unit_windows_are_planned_on_a_slice(tmp_path, loaded, case):
    csr, m, cuts = loaded(case)
    planned = []
    for r in range(len(cuts) - 1):
        A, inf, s = _slice(tmp_path, case, "unit-windows", False, csr, cuts[r], cuts[r + 1])
        xw = A.unit_windows(3072, 16)
        planned.append(int(xw["rowblocks_with_windows"]))
        assert (xw["rowblocks_with_units"] > 0) == bool((s.passes["kind"] == PASS_UNIT).any())
        A.destroy()
    assert max(planned) > 0, planned


@pytest.mark.parametrize("case", list(dc.CASES))
def test_references_are_consistent(loaded, case):
    """General parts tile the matrix, symmetric parts sum to it, entry for entry; the ranks' references sum to the
    product of the untuned CSR within its bound; the beta term is on the owned rows only."""
    csr, m, cuts = loaded(case)
    n, world = csr[3], len(cuts) - 1
    x = synth.random_x(n, seed=5)
    alpha, beta = dc.ALPHA_BETA
    for sym in (False, True):
        total = None
        ref_sum, y0_all = np.zeros(n), np.zeros(n)
        for r in range(world):
            lo, hi = cuts[r], cuts[r + 1]
            part = (dc.symmetric_part if sym else dc.general_part)(m, lo, hi)
            rows = np.unique(part.tocoo().row)
            assert rows.size == 0 or rows.max() < hi
            assert sym or rows.size == 0 or rows.min() >= lo
            total = part if total is None else total + part
            y0 = dc.nan_outside(n, lo, hi, seed=100 + r)
            ref, bound = dc.reference(part, lo, hi, x, alpha, beta, y0)
            assert np.isfinite(ref).all() and (bound > 0).all()
            plain, _ = dc.reference(part, lo, hi, x, alpha)
            assert np.array_equal(ref[:lo], plain[:lo]) and np.array_equal(ref[hi:], plain[hi:])
            assert not ref[hi:].any()
            ref_sum += ref
            y0_all[lo:hi] = y0[lo:hi]
        assert abs(total - m).max() == 0
        full, full_bound = dc.reference(m, 0, n, x, alpha, beta, y0_all)
        assert dc.max_ratio(ref_sum, full, full_bound) <= 1.0


@pytest.mark.parametrize("case", [c for c in dc.CASES if c not in dc.PIPELINED and c != dc.THIN_MIRROR])
def test_decoded_slices_compute_the_references(tmp_path, loaded, case):
    """The independent numpy decoder of the saved stream against the references, for one family per path: the
    slice's stream holds the part matrix the reference multiplies by."""
    csr, m, cuts = loaded(case)
    n = csr[3]
    x = synth.random_x(n, seed=5)
    _, _, _, _, gf, sf = dc.CASES[case]
    for sym, fams in ((False, gf), (True, sf)):
        for r in range(len(cuts) - 1 if fams else 0):
            lo, hi = cuts[r], cuts[r + 1]
            A, inf, s = _slice(tmp_path, case, fams[0], sym, csr, lo, hi)
            part = (dc.symmetric_part if sym else dc.general_part)(m, lo, hi)
            ref, bound = dc.reference(part, lo, hi, x, 1.0)
            assert dc.max_ratio(s.matvec(x), ref, bound) <= 1.0
            A.destroy()
