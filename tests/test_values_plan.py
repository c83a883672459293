"""New values for a tuned pattern on host-only matrices: spx_hip_mat_values_plan, spx_hip_mat_set_values_host and
spx_hip_mat_values_plan_get against the two decoders that share no code with the plan builder's walk -- the numpy
decoder of a saved stream (every stored copy) and spx_mat_get_entry / spx_mat_set_entry (stream_locate)."""
import filecmp

import numpy as np
import pytest
import scipy.sparse as sp

import sparsex_amd as sx
from sparsex_amd import synth
from sparsex_amd.api import SPX_INDEX_ONE_BASED, SpxError

import dist_cases as dc
import limit_cases as lc
import matmat_sym_cases as ms
import values_cases as vc

NONE = vc.NONE

# name -> (generator of the CSR tuple, options, symmetric)
GENERAL = {
    "nlpkkt": (lambda: synth.syn_nlpkkt(6), {}),
    "cant": (lambda: synth.syn_cant(0.02), {}),
    "webbase": (lambda: synth.syn_webbase(0.003), {}),
    "wide-offsets": (lambda: lc.wide_offsets((65536,))[0], lc.off_options("plain")),
    "wide-offsets-c2": (lambda: lc.wide_offsets((65536, 65536))[0], lc.off_options("slices-c2")),
    "pass-edges": (lambda: lc.pass_edges()[0], lc.PASS_OPTS),
    "diagonals": (lambda: lc.diagonals()[0], lc.SEGS["segs-8188"][0]),
    "diagonals-joined": (lambda: lc.diagonals()[0], lc.SEGS["segs-joined"][0]),
    "step-lines": (lambda: lc.step_lines(127)[0], lc.STEPS["step-127"][1]),
}
SYMMETRIC = {
    "nlpkkt": (lambda: synth.syn_nlpkkt(6), {}),
    "cant": (lambda: synth.syn_cant(0.02), {}),
    "nd24k": (lambda: synth.syn_nd24k(0.02), {}),
    "tiles-and-segments": (lambda: ms.tiles_and_segments()[0], ms.case_options("tiles-and-segments")),
    "no-slot": (lambda: ms.segments_without_slot()[0], ms.case_options("no-slot")),
    "arrow": (lambda: ms.arrow()[0], ms.case_options("arrow")),
    "block-banded": (lambda: ms.block_banded()[0], ms.case_options("block-banded")),
    "sym-wide": (lambda: lc.sym_wide(70000, 65536, runs=True)[0], lc.sym_options("segments")),
    "pass-edges-sym": (lambda: lc.pass_edges_sym()[0], dict(lc.sym_options("segments"), **lc.PASS_SYM_OPTS)),
}
GENERAL_OPTIONS = {
    "defaults": {},
    "no-stacking": {"spx.gpu.stack_segments": "false"},
    "no-recut": {"spx.gpu.recut_linear": "false"},
    "slices-c2": {"spx.gpu.col_phases": "c2"},
    "slices-2": {"spx.gpu.col_phases": "2"},
    "rows-2048": {"spx.gpu.rowblock_rows": "2048"},
    "onedim": {"spx.matrix.onedim_blocks": "true"},
}
SYMMETRIC_OPTIONS = {
    "defaults": {},
    "mirrored": {"spx.gpu.sym_once": "false"},
    "segments": {"spx.gpu.sym_segments": "true"},
    "no-segments": {"spx.gpu.sym_segments": "false"},
    "matmat": {"spx.gpu.sym_matmat": "true"},
    "rows-2048": {"spx.gpu.rowblock_rows": "2048"},
    "onedim": {"spx.matrix.onedim_blocks": "true"},
}
_cache = {}


def matrix(sym, name):
    key = (sym, name)
    if key not in _cache:
        gen, opts = (SYMMETRIC if sym else GENERAL)[name]
        _cache[key] = (gen(), opts)
    return _cache[key]


def owned_entries(csr, sym, lo, hi, perm=None, row0=0):
    """Entries a process that owns the tuned rows [lo, hi) holds: the entries of those rows; symmetric: the ones on
    and below the diagonal."""
    r, c = vc.coords(csr)
    r = r + row0
    if perm is not None:
        r, c = perm[r], perm[c]
    own = (r >= lo) & (r < hi)
    return own & (c <= r) if sym else own


def full_check(A, csr, sym, tmp_path, seed=1, perm=None):
    """plan, counts, an update checked by both decoders, a single set_entry on top, and back again"""
    rp, ci, va, n = csr
    inf = A.info()
    A.values_plan(rp, ci)
    info = A.values_plan_info()
    assert info["plan_bytes"] == 0 and info["n_diag"] == (inf.row_hi - inf.row_lo if sym else 0)
    cnt = vc.destinations(info, va.size)
    own = owned_entries(csr, sym, inf.row_lo, inf.row_hi, perm)
    assert info["n_sources"] == int(own.sum()) == int((cnt > 0).sum())
    assert info["n_dest"] == int(cnt.sum())
    assert np.array_equal(cnt > 0, own), "the sources are not the entries the process owns"
    r, c = vc.coords(csr)
    if sym:
        assert set(cnt[own & (r == c)].tolist()) <= {1}
        assert set(cnt[own & (r != c)].tolist()) <= {1, 2}
    else:
        assert info["n_dest"] == info["n_sources"]
    first = str(tmp_path / "v0.spx")
    A.save(first)
    v1 = vc.new_values(csr, sym, seed)
    A.set_values(v1)
    m1 = vc.to_scipy(vc.with_values(csr, v1), ncols=A.ncols)
    vc.check_stream(A, m1, tmp_path, sym, perm)
    vc.check_entries(A, m1)
    changed = str(tmp_path / "v1.spx")
    A.save(changed)
    assert va.size == 0 or not filecmp.cmp(first, changed, shallow=False)
    # the values of the tune again: every bit of the file as it was (padding included)
    A.set_values(va)
    again = str(tmp_path / "v0-again.spx")
    A.save(again)
    assert filecmp.cmp(first, again, shallow=False)
    A.set_values(v1)
    # one spx_mat_set_entry finds the copies the plan writes: the same file either way (both saved after the
    # call, which also edits the encoded partitions the file carries)
    if va.size:
        k = va.size // 2
        A.set_entry(int(r[k]), int(c[k]), 3.25)
        edited = str(tmp_path / "edit.spx")
        A.save(edited)
        v2 = v1.copy()
        v2[(r == r[k]) & (c == c[k])] = 3.25
        if sym:
            v2[(r == c[k]) & (c == r[k])] = 3.25
        A.set_values(v2)
        planned = str(tmp_path / "plan.spx")
        A.save(planned)
        assert filecmp.cmp(edited, planned, shallow=False), "set_entry and the plan write different positions"
        vc.check_entries(A, vc.to_scipy(vc.with_values(csr, v2), ncols=A.ncols), limit=300)
    return info


@pytest.mark.parametrize("name", list(GENERAL))
def test_general_matrices(tmp_path, name):
    csr, opts = matrix(False, name)
    A = vc.tune(csr, opts, host_only=True, ncols=int(csr[1].max()) + 1 if name.startswith("wide") else None)
    full_check(A, csr, False, tmp_path)
    A.destroy()


@pytest.mark.parametrize("name", list(SYMMETRIC))
def test_symmetric_matrices(tmp_path, name):
    csr, opts = matrix(True, name)
    A = vc.tune(csr, opts, sym=True, host_only=True)
    full_check(A, csr, True, tmp_path)
    A.destroy()


@pytest.mark.parametrize("mode", list(GENERAL_OPTIONS))
@pytest.mark.parametrize("name", ["nlpkkt", "cant", "webbase"])
def test_general_option_sets(tmp_path, name, mode):
    csr, _ = matrix(False, name)
    A = vc.tune(csr, GENERAL_OPTIONS[mode], host_only=True)
    full_check(A, csr, False, tmp_path)
    A.destroy()


@pytest.mark.parametrize("mode", list(SYMMETRIC_OPTIONS))
@pytest.mark.parametrize("name", ["nlpkkt", "cant", "nd24k"])
def test_symmetric_option_sets(tmp_path, name, mode):
    csr, _ = matrix(True, name)
    A = vc.tune(csr, SYMMETRIC_OPTIONS[mode], sym=True, host_only=True)
    info = full_check(A, csr, True, tmp_path)
    if mode == "mirrored":
        # (the mirror image is stored: two destinations for every off-diagonal entry)
        r, c = vc.coords(csr)
        assert info["n_dest"] == int((c < r).sum()) * 2 + csr[3]
    A.destroy()


@pytest.mark.parametrize("sym", [False, True])
def test_reordered_matrix(tmp_path, sym):
    csr, _ = matrix(sym, "cant")
    A = vc.tune(csr, {}, sym=sym, host_only=True, reorder=True)
    perm = A.get_perm()
    assert perm is not None and not np.array_equal(perm, np.arange(csr[3]))
    full_check(A, csr, sym, tmp_path, perm=perm.astype(np.int64))
    A.destroy()


@pytest.mark.parametrize("sym", [False, True])
@pytest.mark.parametrize("world", [2, 3])
def test_ranks_of_a_whole_matrix(tmp_path, world, sym):
    """spx.rt.gpu_rank/world: every rank plans from the whole CSR and owns its rows; together they own everything"""
    csr, _ = matrix(sym, "nlpkkt")
    rp, ci, va, n = csr
    v1 = vc.new_values(csr, sym, 5)
    m1 = vc.to_scipy(vc.with_values(csr, v1))
    owned = np.zeros(va.size, dtype=np.int64)
    for rank in range(world):
        A = dc.tune_rank(csr, rank, world, dc.NOSAMPLE, sym, host_only=True)
        inf = A.info()
        A.values_plan(rp, ci)
        info = A.values_plan_info()
        cnt = vc.destinations(info, va.size)
        own = owned_entries(csr, sym, inf.row_lo, inf.row_hi)
        assert np.array_equal(cnt > 0, own) and info["n_sources"] == int(own.sum())
        owned += own
        A.set_values(v1)
        vc.check_stream(A, m1, tmp_path, sym)
        vc.check_entries(A, m1, rows=(inf.row_lo, inf.row_hi), sym=sym, limit=400)
        A.destroy()
    r, c = vc.coords(csr)
    assert np.array_equal(owned, (c <= r).astype(np.int64) if sym else np.ones(va.size, dtype=np.int64))


def _slice_csr(csr, lo, hi):
    rp, ci, va, n = csr
    return ((rp[lo:hi + 1] - rp[lo]).astype(np.int32), ci[rp[lo]:rp[hi]].copy(), va[rp[lo]:rp[hi]].copy(), n)


@pytest.mark.parametrize("sym", [False, True])
@pytest.mark.parametrize("kind", ["balanced", "one-row"])
def test_row_offset_slices(tmp_path, kind, sym):
    """spx.rt.row_offset/global_rows: the CSR arrays hold the slice's rows; the last slice of "one-row" is one row"""
    csr, _ = matrix(sym, "nlpkkt")
    n = csr[3]
    cuts = dc.cut(csr, 3, kind)
    for lo, hi in zip(cuts, cuts[1:]):
        A = dc.tune_rows(csr, lo, hi, dc.NOSAMPLE, sym, host_only=True)
        part = _slice_csr(csr, lo, hi)
        A.values_plan(part[0], part[1])
        info = A.values_plan_info()
        r, c = vc.coords(part)
        own = (c <= r + lo) if sym else np.ones(r.size, dtype=bool)
        assert info["n_sources"] == int(own.sum())
        assert np.array_equal(vc.destinations(info, r.size) > 0, own)
        v1 = vc.new_values(part, sym, 9, row0=lo)
        A.set_values(v1)
        m1 = vc.to_scipy(vc.with_values(part, v1), row0=lo, nrows=n)
        if sym:
            low = sp.tril(m1).tocsr()
            m1 = (low + sp.tril(low, -1).T).tocsr()
        vc.check_stream(A, m1, tmp_path, sym)
        vc.check_entries(A, vc.to_scipy(vc.with_values(part, v1), row0=lo, nrows=n), rows=(lo, hi), sym=sym, limit=300)
        A.destroy()


def test_symmetric_slice_with_a_thin_mirror_list(tmp_path):
    csr = dc.matrix(dc.THIN_MIRROR)
    n = csr[3]
    cuts = dc.bounds(dc.THIN_MIRROR, csr)
    lo, hi = cuts[-2], cuts[-1]
    A = dc.tune_rows(csr, lo, hi, dc.family_options(dc.THIN_MIRROR, "lists", True), True, host_only=True)
    part = _slice_csr(csr, lo, hi)
    A.values_plan(part[0], part[1])
    info = A.values_plan_info()
    assert info["n_mirror"] > 0 and (info["src_mirror"] != NONE).all()
    v1 = vc.new_values(part, True, 11, row0=lo)
    A.set_values(v1)
    low = sp.tril(vc.to_scipy(vc.with_values(part, v1), row0=lo, nrows=n)).tocsr()
    s = vc.check_stream(A, (low + sp.tril(low, -1).T).tocsr(), tmp_path, True)
    r, c = dc.thin_mirror_entry(csr, lo, s.mirror_rows)
    assert A.get_entry(r, c) == low[r, c] == A.get_entry(c, r)
    # (the list's values are the new ones)
    rows = np.repeat(s.mirror_rows.astype(np.int64), np.diff(s.mirror_ptr.astype(np.int64)))
    assert np.array_equal(s.mirror_val, np.asarray(low[s.mirror_col.astype(np.int64), rows]).ravel())
    A.destroy()


def _csr_of(m):
    m = sp.csr_matrix(m)
    m.sort_indices()
    return (m.indptr.astype(np.int32), m.indices.astype(np.int32), m.data.copy(), m.shape[0])


def test_columns_in_descending_order(tmp_path):
    csr, _ = matrix(False, "cant")
    rp, ci, va, n = csr
    # every row back to front: the loader sorts, the plan must find the entries where the caller keeps them
    order = np.concatenate([np.arange(rp[i + 1] - 1, rp[i] - 1, -1) for i in range(n)]) if n else np.zeros(0, int)
    rev = (rp, ci[order].copy(), va[order].copy(), n)
    A = vc.tune(rev, {}, host_only=True)
    A.values_plan(rev[0], rev[1])
    v1 = vc.new_values(rev, False, 2)
    A.set_values(v1)
    m1 = vc.to_scipy(vc.with_values(rev, v1))
    vc.check_stream(A, m1, tmp_path)
    vc.check_entries(A, m1, limit=300)
    A.destroy()


def test_one_based_arrays(tmp_path):
    csr, _ = matrix(False, "nlpkkt")
    one = ((csr[0] + 1).astype(np.int32), (csr[1] + 1).astype(np.int32), csr[2], csr[3])
    A = vc.tune(one, {}, host_only=True, indexing=SPX_INDEX_ONE_BASED)
    A.values_plan(one[0], one[1], indexing=SPX_INDEX_ONE_BASED)
    v1 = vc.new_values(csr, False, 3)
    A.set_values(v1)
    vc.check_stream(A, vc.to_scipy(vc.with_values(csr, v1)), tmp_path)
    # (the wrong indexing is a pattern the matrix was not tuned from)
    with pytest.raises(SpxError):
        A.values_plan(one[0], one[1])
    A.destroy()


def test_explicit_zeros_among_the_tuned_values(tmp_path):
    csr, _ = matrix(False, "nlpkkt")
    va = csr[2].copy()
    va[::3] = 0.0
    zeroed = vc.with_values(csr, va)
    A = vc.tune(zeroed, {}, host_only=True)
    full_check(A, zeroed, False, tmp_path)
    A.destroy()
    B = vc.tune(zeroed, {}, sym=True, host_only=True)
    B.values_plan(csr[0], csr[1])
    v1 = vc.new_values(csr, True, 4)
    B.set_values(v1)
    vc.check_stream(B, vc.to_scipy(vc.with_values(csr, v1)), tmp_path, True)
    B.destroy()


def test_empty_rows_one_by_one_and_rectangular(tmp_path):
    rng = np.random.RandomState(5)
    m = sp.random(300, 300, density=0.02, random_state=rng, format="lil")
    m[10:40] = 0
    m[299] = 0
    hollow = _csr_of(sp.csr_matrix(m))
    A = vc.tune(hollow, {}, host_only=True)
    full_check(A, hollow, False, tmp_path)
    A.destroy()
    one = (np.array([0, 1], np.int32), np.array([0], np.int32), np.array([2.5]), 1)
    for sym in (False, True):
        A = vc.tune(one, {}, sym=sym, host_only=True)
        A.values_plan(one[0], one[1])
        A.set_values(np.array([-7.0]))
        assert A.get_entry(0, 0) == -7.0
        info = A.values_plan_info()
        assert info["n_sources"] == info["n_dest"] == 1
        A.destroy()
    rect = sp.random(257, 1031, density=0.01, random_state=rng, format="csr")
    rcsr = _csr_of(rect)
    A = vc.tune(rcsr, {}, host_only=True, ncols=1031)
    A.values_plan(rcsr[0], rcsr[1])
    v1 = vc.new_values(rcsr, False, 6)
    A.set_values(v1)
    m1 = sp.csr_matrix((v1, rcsr[1], rcsr[0]), shape=(257, 1031))
    vc.check_stream(A, m1, tmp_path)
    vc.check_entries(A, m1, limit=300)
    A.destroy()


def _broken_patterns(csr, sym):
    """name -> (rowptr, colind) that are not the tuned pattern"""
    rp, ci, va, n = csr
    row = int(np.flatnonzero(np.diff(rp) >= 3)[-1])
    a = int(rp[row])
    if ci[a + 1] == row:
        a += 1
    free = int(np.setdiff1d(np.arange(n), ci[rp[row]:rp[row + 1]])[0])
    out = {}
    moved = ci.copy()
    moved[a + 1] = free
    out["one column changed"] = (rp, moved)
    # (a symmetric plan falls back on the transposed position: both are taken away)
    less = sp.csr_matrix((np.ones(ci.size), ci, rp), shape=(n, n)).tolil()
    less[row, int(ci[a + 1])] = 0
    if sym:
        less[int(ci[a + 1]), row] = 0
    less = _csr_of(less.tocsr())
    assert less[1].size == ci.size - (2 if sym else 1)
    out["one entry removed"] = (less[0], less[1])
    rp_more = rp.copy()
    rp_more[row + 1:] += 1
    out["one entry added"] = (rp_more, np.insert(ci, a + 1, free).astype(np.int32))
    twice = ci.copy()
    twice[a + 1] = twice[a]
    out["a repeated column"] = (rp, twice)
    return out


@pytest.mark.parametrize("sym", [False, True])
def test_patterns_that_are_not_the_tuned_one(tmp_path, sym, capfd):
    csr, _ = matrix(sym, "nlpkkt")
    rp, ci, va, n = csr
    A = vc.tune(csr, {}, sym=sym, host_only=True)
    A.values_plan(rp, ci)
    v1 = vc.new_values(csr, sym, 7)
    A.set_values(v1)
    m1 = vc.to_scipy(vc.with_values(csr, v1))
    kept = str(tmp_path / "kept.spx")
    A.save(kept)
    for name, (brp, bci) in _broken_patterns(csr, sym).items():
        A.values_plan(rp, ci)
        capfd.readouterr()
        with pytest.raises(SpxError):
            A.values_plan(brp.astype(np.int32), bci.astype(np.int32))
        err = capfd.readouterr().err
        assert "row " in err and "column " in err, (name, err)
        # no plan is left behind, and nothing was written
        with pytest.raises(SpxError):
            A.values_plan_info()
        assert sx.lib().spx_hip_mat_set_values_host(A.handle, v1.ctypes.data) != 0
        now = str(tmp_path / "now.spx")
        A.save(now)
        assert filecmp.cmp(kept, now, shallow=False), name
    vc.check_entries(A, m1, limit=200)
    A.destroy()


def test_calls_without_a_plan_and_bad_arguments(tmp_path, capfd):
    csr, _ = matrix(False, "nlpkkt")
    rp, ci, va, n = csr
    L = sx.lib()
    A = vc.tune(csr, {}, host_only=True)
    ok = 0
    # before any plan
    assert L.spx_hip_mat_set_values_host(A.handle, va.ctypes.data) != ok
    with pytest.raises(SpxError):
        A.set_values(va)
    with pytest.raises(SpxError):
        A.values_plan_info()
    A.values_plan(rp, ci)
    # a host-only matrix has no device path
    assert L.spx_hip_mat_set_values(A.handle, va.ctypes.data, None) != ok
    # NULL arguments
    assert L.spx_hip_mat_values_plan(None, rp.ctypes.data, ci.ctypes.data, 0) != ok
    assert L.spx_hip_mat_values_plan(A.handle, None, ci.ctypes.data, 0) != ok
    A.values_plan(rp, ci)
    assert L.spx_hip_mat_values_plan(A.handle, rp.ctypes.data, None, 0) != ok
    A.values_plan(rp, ci)
    assert L.spx_hip_mat_set_values_host(None, va.ctypes.data) != ok
    assert L.spx_hip_mat_set_values_host(A.handle, None) != ok
    assert L.spx_hip_mat_set_values(None, va.ctypes.data, None) != ok
    assert L.spx_hip_mat_values_plan_get(A.handle, None) != ok
    assert L.spx_hip_mat_values_plan_get(None, None) != ok
    assert L.spx_hip_mat_values_plan_drop(None) != ok
    # after the drop
    v1 = vc.new_values(csr, False, 8)
    A.set_values(v1)
    A.values_plan_drop()
    assert L.spx_hip_mat_set_values_host(A.handle, va.ctypes.data) != ok
    with pytest.raises(SpxError):
        A.set_values(va)
    vc.check_entries(A, vc.to_scipy(vc.with_values(csr, v1)), limit=200)
    # a second plan replaces the first
    A.values_plan(rp, ci)
    A.values_plan(rp, ci)
    A.set_values(va)
    vc.check_entries(A, vc.to_scipy(csr), limit=200)
    capfd.readouterr()
    A.destroy()


@pytest.mark.parametrize("sym", [False, True])
def test_the_csx_export_goes_stale(sym, capfd):
    csr, _ = matrix(sym, "nlpkkt")
    A = vc.tune(csr, {}, sym=sym, host_only=True)
    assert A.export_csx(0)["nnz"] > 0
    units = A.export_units(0)
    A.values_plan(csr[0], csr[1])
    assert A.export_csx(0)["nnz"] > 0            # (a plan alone changes nothing)
    A.set_values(vc.new_values(csr, sym, 12))
    capfd.readouterr()
    with pytest.raises(SpxError):
        A.export_csx(0)
    assert "stale" in capfd.readouterr().err
    assert A.export_units(0) == units
    A.destroy()


@pytest.mark.parametrize("sym", [False, True])
def test_a_file_saved_after_an_update_carries_no_stale_partitions(tmp_path, sym, capfd):
    """spx.rt.keep_encoded=true (the default): tune, update, save, restore -- the restored matrix shows the new
    values and exports nothing; the old values come from no call."""
    csr, _ = matrix(sym, "nlpkkt")
    A = vc.tune(csr, {}, sym=sym, host_only=True)
    before = A.export_csx(0)
    A.values_plan(csr[0], csr[1])
    v1 = vc.new_values(csr, sym, 14)
    A.set_values(v1)
    f = str(tmp_path / "after.spx")
    A.save(f)
    sx.options_reset()
    sx.option_set("spx.rt.host_only", "true")
    B = sx.mat_restore(f)
    m1 = vc.to_scipy(vc.with_values(csr, v1))
    vc.check_entries(B, m1, limit=300)
    vc.check_stream(B, m1, tmp_path, sym)
    with pytest.raises(SpxError):
        B.export_csx(0)
    # an edit of a stale matrix stays out of its partitions, and the file still carries none
    r, c = vc.coords(csr)
    A.set_entry(int(r[5]), int(c[5]), 9.5)
    A.save(f)
    C_ = sx.mat_restore(f)
    assert C_.get_entry(int(r[5]), int(c[5])) == 9.5
    with pytest.raises(SpxError):
        C_.export_csx(0)
    # the values of the tune put back bit for bit: after that edit the partitions stay refused ...
    A.set_values(csr[2])
    with pytest.raises(SpxError):
        A.export_csx(0)
    capfd.readouterr()
    for M in (A, B, C_):
        M.destroy()
    # ... without one they are true again, exported and saved again
    D = vc.tune(csr, {}, sym=sym, host_only=True)
    D.values_plan(csr[0], csr[1])
    D.set_values(v1)
    D.set_values(csr[2])
    again = D.export_csx(0)
    assert np.array_equal(again["values"], before["values"]) and np.array_equal(again["ctl"], before["ctl"])
    D.save(f)
    E = sx.mat_restore(f)
    assert np.array_equal(E.export_csx(0)["values"], before["values"])
    D.destroy()
    E.destroy()


@pytest.mark.parametrize("sym", [False, True])
def test_restored_row_offset_slice(tmp_path, sym):
    """A slice tuned from its own rows (spx.rt.row_offset), saved and restored: the plan takes the slice's arrays"""
    csr, _ = matrix(sym, "nlpkkt")
    n = csr[3]
    cuts = dc.cut(csr, 3, "balanced")
    for k, (lo, hi) in enumerate(zip(cuts, cuts[1:])):
        A = dc.tune_rows(csr, lo, hi, dc.NOSAMPLE, sym, host_only=True)
        f = str(tmp_path / ("slice%d.spx" % k))
        A.save(f)
        A.destroy()
        sx.options_reset()
        sx.option_set("spx.rt.host_only", "true")
        B = sx.mat_restore(f)
        part = _slice_csr(csr, lo, hi)
        B.values_plan(part[0], part[1])
        v1 = vc.new_values(part, sym, 15, row0=lo)
        B.set_values(v1)
        m1 = vc.to_scipy(vc.with_values(part, v1), row0=lo, nrows=n)
        if sym:
            low = sp.tril(m1).tocsr()
            m1 = (low + sp.tril(low, -1).T).tocsr()
        vc.check_stream(B, m1, tmp_path, sym)
        vc.check_entries(B, vc.to_scipy(vc.with_values(part, v1), row0=lo, nrows=n), rows=(lo, hi), sym=sym, limit=200)
        # (the whole matrix' arrays are not this slice's; those of the first slice are their beginning)
        if lo > 0:
            with pytest.raises(SpxError):
                B.values_plan(csr[0], csr[1])
        B.destroy()


@pytest.mark.parametrize("sym", [False, True])
def test_restored_matrix(tmp_path, sym):
    csr, _ = matrix(sym, "cant")
    # (spx.rt.keep_encoded=false: the file then holds no encoded partitions)
    A = vc.tune(csr, {"spx.rt.keep_encoded": "false"}, sym=sym, host_only=True)
    f = str(tmp_path / "saved.spx")
    A.save(f)
    A.destroy()
    sx.options_reset()
    sx.option_set("spx.rt.host_only", "true")
    B = sx.mat_restore(f)
    with pytest.raises(SpxError):
        B.values_plan_info()                              # the plan is not part of the file
    B.values_plan(csr[0], csr[1])
    v1 = vc.new_values(csr, sym, 13)
    B.set_values(v1)
    m1 = vc.to_scipy(vc.with_values(csr, v1))
    vc.check_stream(B, m1, tmp_path, sym)
    vc.check_entries(B, m1, limit=400)
    B.destroy()
