"""Row / column norms and diagonal scaling of a tuned matrix on the host copy of the stream (host-only tunes:
spx_hip_mat_norms_host, spx_hip_mat_scale_host through mat_scale.cpp): the norms against numpy over the untuned CSR
arrays, the scaled values bit for bit in every stored copy (the arithmetic is fl(fl(dr[r] * a) * dc[c])), padding
untouched, the other entry points and the stale-partition rule of the value refresh.  No GPU."""
import numpy as np
import pytest

import sparsex_amd as sx
from sparsex_amd.api import SpxError

import scale_cases as sc
import values_cases as vc
from diag_cases import matrix, bits

# name -> (matrix, options, reorder)
TUNES = {
    "cant": ("cant", {}, False),
    "nlpkkt": ("nlpkkt", {}, False),
    "webbase": ("webbase", {}, False),
    "rect": ("rect", {}, False),
    "rect-t": ("rect-t", {}, False),
    "cant-reorder": ("cant", {}, True),
    "cant-c2": ("cant", {"spx.gpu.col_phases": "c2"}, False),
    "cant-f32": ("cant", {"spx.gpu.values_f32": "true"}, False),
}
SLICES = ("rank", "row-offset")


def norms_into_sentinels(t):
    def norms_of(kind):
        rows, cols = np.full(t.nrows, sc.SENTINEL), np.full(t.ncols, sc.SENTINEL)
        out = t.A.norms_host(kind, rows, cols)
        assert out[0] is rows and out[1] is cols
        return rows, cols
    return norms_of


@pytest.fixture(params=list(TUNES) + list(SLICES))
def tuned(request):
    name = request.param
    t = sc.tune_slice(name, host_only=True) if name in SLICES else sc.tune_matrix(*TUNES[name], host_only=True)
    assert not t.A.info().on_device
    t.name = name
    yield t
    t.A.destroy()
    sx.options_reset()


def test_norms_against_numpy(tuned):
    t = tuned
    if t.name in SLICES:
        assert 0 < t.lo < t.hi < t.nrows
    t.check_norms(norms_into_sentinels(t), t.csr[2])
    # one output at a time: the other is not computed
    for kind in sc.KINDS:
        want_r, want_c, nr, nc = sc.expected_norms(t.csr, kind, t.nrows, t.ncols, t.lo, t.hi, t.perm, t.row0)
        rows = np.full(t.nrows, sc.SENTINEL)
        assert t.A.norms_host(kind, rows, False)[1] is None
        sc.check_norms(kind, rows, want_r, nr, "rows alone")
        cols = np.full(t.ncols, sc.SENTINEL)
        assert t.A.norms_host(kind, False, cols)[0] is None
        sc.check_norms(kind, cols, want_c, nc, "cols alone")
    # new arrays: zeros outside the own rows
    rows, cols = t.A.norms_host(sx.NORM_MAX_ABS)
    assert rows.shape == (t.nrows,) and cols.shape == (t.ncols,)
    assert not rows[:t.lo].any() and not rows[t.hi:].any()


def test_scaled_values_in_every_stored_copy(tuned, tmp_path):
    t = tuned
    A = t.A
    A.values_plan(t.csr[0], t.csr[1])
    plan = A.values_plan_info()["src_values"]
    before = vc.decoded(A, tmp_path, "before.spx")
    dr, dcv = sc.vector(t.nrows, 1), sc.vector(t.ncols, 2)
    assert (np.abs(dr) > 0.5).all() and (np.abs(dr) < 2).all() and (dr < 0).any() and (dr > 0).any()
    A.scale(dr, dcv)
    v1 = sc.scaled_values(t.csr, dr, dcv, t.perm, t.row0)
    assert not np.array_equal(bits(v1), bits(t.csr[2]))
    m1 = t.scipy(v1)
    after = vc.check_stream(A, m1, tmp_path, perm=t.perm)
    n_pad = sc.untouched_positions(before, after, plan)
    print("%s: %d of %d positions hold no entry" % (t.name, n_pad, plan.size))
    # the other entry points see the scaled matrix
    rows = (t.lo, t.hi) if t.name in SLICES else None
    assert vc.check_entries(A, m1, rows=rows, limit=300) > 0
    A.diag_plan()
    r, c = sc.tuned_coords(t.csr, t.perm, t.row0)
    on = (r == c) & (r >= t.lo) & (r < t.hi)
    want_d = np.zeros(t.nrows)
    want_d[r[on]] = v1[on]
    got_d = A.get_diag_host()
    assert np.array_equal(bits(got_d[t.lo:t.hi]), bits(want_d[t.lo:t.hi]))
    t.check_norms(norms_into_sentinels(t), v1)
    # the encoded partitions are stale, the pattern is still handed out
    inf = A.info()
    with pytest.raises(SpxError):
        A.export_csx(inf.first_partition)
    # each vector alone: one product, rounded once
    A.scale(dr=dr)
    v2 = sc.scaled_values(vc.with_values(t.csr, v1), dr, None, t.perm, t.row0)
    vc.check_stream(A, t.scipy(v2), tmp_path, perm=t.perm)
    A.scale(dc=dcv)
    v3 = sc.scaled_values(vc.with_values(t.csr, v2), None, dcv, t.perm, t.row0)
    after3 = vc.check_stream(A, t.scipy(v3), tmp_path, perm=t.perm)
    sc.untouched_positions(before, after3, plan)
    # a refresh overwrites with what the caller hands over
    A.set_values(t.csr[2].copy())
    back = vc.check_stream(A, t.scipy(t.csr[2]), tmp_path, perm=t.perm)
    assert np.array_equal(bits(back.values), bits(before.values))


def test_power_of_two_round_trip_saves_the_same_file(tuned, tmp_path):
    t = tuned
    A = t.A
    A.values_plan(t.csr[0], t.csr[1])
    A.set_values(t.csr[2].copy())              # (no-op: both files are written under the same stale-partition rule)
    f0, f1 = str(tmp_path / "f0.spx"), str(tmp_path / "f1.spx")
    A.save(f0)
    pr, pc = sc.pow2_vector(t.nrows, 3), sc.pow2_vector(t.ncols, 4)
    assert set(np.unique(pr)) <= set(2.0 ** np.arange(-3, 4)) and np.unique(pr).size > 3
    A.scale(pr, pc)
    vc.check_stream(A, t.scipy(sc.scaled_values(t.csr, pr, pc, t.perm, t.row0)), tmp_path, perm=t.perm)
    A.scale(1.0 / pr, 1.0 / pc)
    A.save(f1)
    with open(f0, "rb") as a, open(f1, "rb") as b:
        assert a.read() == b.read()


def test_refusals_leave_everything_alone(tmp_path, capfd):
    csr = matrix("nlpkkt")
    n = csr[3]
    L = sx.lib()
    dr = sc.vector(n, 1)
    rows, cols = np.full(n, sc.SENTINEL), np.full(n, sc.SENTINEL)

    def outputs_untouched():
        return (rows == sc.SENTINEL).all() and (cols == sc.SENTINEL).all()

    A = vc.tune(csr, host_only=True)
    before = vc.decoded(A, tmp_path, "a.spx")
    capfd.readouterr()
    # a NULL handle, a kind out of range, both outputs NULL, both vectors NULL, the device forms on a host-only matrix
    assert L.spx_hip_mat_norms_host(None, 0, rows.ctypes.data, cols.ctypes.data) == sx.SPX_FAILURE
    assert L.spx_hip_mat_scale_host(None, dr.ctypes.data, None) == sx.SPX_FAILURE
    assert L.spx_hip_mat_norms(None, 0, rows.ctypes.data, None, None) == sx.SPX_FAILURE
    assert L.spx_hip_mat_scale(None, dr.ctypes.data, None, None) == sx.SPX_FAILURE
    for kind in (-1, 3):
        assert L.spx_hip_mat_norms_host(A.handle, kind, rows.ctypes.data, cols.ctypes.data) == sx.SPX_FAILURE
    assert "kind" in capfd.readouterr().err
    assert L.spx_hip_mat_norms_host(A.handle, 0, None, None) == sx.SPX_FAILURE
    assert L.spx_hip_mat_scale_host(A.handle, None, None) == sx.SPX_FAILURE
    assert "both NULL" in capfd.readouterr().err
    # (host addresses: a device form that went on would fault, it must refuse before it looks at them)
    assert L.spx_hip_mat_norms(A.handle, 0, rows.ctypes.data, cols.ctypes.data, None) == sx.SPX_FAILURE
    assert L.spx_hip_mat_scale(A.handle, dr.ctypes.data, dr.ctypes.data, None) == sx.SPX_FAILURE
    assert "host_only" in capfd.readouterr().err
    assert outputs_untouched()
    assert np.array_equal(bits(vc.decoded(A, tmp_path, "b.spx").values), bits(before.values))
    A.export_csx(A.info().first_partition)                      # nothing went stale
    A.destroy()
    # a symmetric tune
    S = vc.tune(csr, sym=True, host_only=True)
    before = vc.decoded(S, tmp_path, "s0.spx")
    capfd.readouterr()
    with pytest.raises(SpxError):
        S.norms_host(sx.NORM_MAX_ABS, rows, cols)
    with pytest.raises(SpxError):
        S.scale(dr, dr)
    assert "symmetric" in capfd.readouterr().err
    assert outputs_untouched()
    after = vc.decoded(S, tmp_path, "s1.spx")
    assert np.array_equal(bits(after.values), bits(before.values)) and np.array_equal(bits(after.dvalues), bits(before.dvalues))
    S.destroy()
    sx.options_reset()
