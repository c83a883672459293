"""Norms and the scaling D * A * D of a matrix tuned as a symmetric one, on the host copy of the stream (host-only
tunes: spx_hip_mat_sym_norms_host, spx_hip_mat_sym_scale_host through mat_scale.cpp): the norms against numpy over the
full symmetric CSR arrays, the scaled values bit for bit in every stored copy -- lower triangle, mirror image, tiles,
read-once segments, thin mirror list, diagonal; the arithmetic is fl(fl(d[max(r,c)] * a) * d[min(r,c)]) -- the
positions without a source in the values plan untouched, the other entry points and the stale-partition rule of the
value refresh.  No GPU."""
import numpy as np
import pytest

import sparsex_amd as sx
from sparsex_amd import synth
from sparsex_amd.api import SpxError

import dist_cases as dc
import limit_cases as lc
import scale_cases as sc
import sym_scale_cases as ssc
import values_cases as vc
import test_gpu_sym_pipeline as tsp
import test_gpu_transpose as tt
from diag_cases import matrix, bits

# name -> (generator, options, reorder)
TUNES = {
    "cant": (lambda: matrix("cant"), {}, False),
    "nlpkkt": (lambda: matrix("nlpkkt"), {}, False),
    "nd24k": (dc.MATRICES["nd24k"], {}, False),                      # 8x8 tiles
    "kkt44-pipeline": (lambda: synth.syn_nlpkkt(44), dict(tsp.ON), False),   # read-once segments, inline headers
    "kkt20-no-once": (tt.SYM_CASES["no-once"][0], dict(tt.SYM_CASES["no-once"][1]), False),
    "nd24k-f32": (dc.MATRICES["nd24k"], {"spx.gpu.values_f32": "all"}, False),
    "cant-reorder": (lambda: matrix("cant"), {}, True),
}
TUNES.update({"nd24k-" + f: (dc.MATRICES["nd24k"], dict(o), False) for f, o in lc.SYM_FAMILIES.items()})
TUNES.update({"nlpkkt-" + f: (lambda: matrix("nlpkkt"), dict(o), False) for f, o in lc.SYM_FAMILIES.items()})
# case of dist_cases -> how the slice is made
SLICES = {"thin-mirror-w3-balanced": "row-offset", "nd24k-w3-shifted": "rank"}


def norms_into_sentinels(A, n):
    def norms_of(kind):
        out = np.full(n, ssc.SENTINEL)
        assert A.sym_norms_host(kind, out) is out
        return out
    return norms_of


def scale_and_check(A, csr, tmp_path, perm=None, lo=0, hi=None, plan_csr=None):
    """sym_scale with a vector of mixed signs: every stored copy, the untouched positions, the other readers, the
    norms of the scaled matrix, the stale partitions.  Returns (stream before, scaled values)."""
    n = csr[3]
    hi = n if hi is None else hi
    plan_csr = csr if plan_csr is None else plan_csr
    A.values_plan(plan_csr[0], plan_csr[1])
    plan = A.values_plan_info()["src_values"]
    before = vc.decoded(A, tmp_path, "before.spx")
    d = ssc.vector(n, 1)
    assert (np.abs(d) > 0.5).all() and (np.abs(d) < 2).all() and (d < 0).any() and (d > 0).any()
    A.sym_scale(d)
    v1, m1 = ssc.scaled_matrix(csr, d, perm)
    assert not np.array_equal(bits(v1), bits(csr[2]))
    after = vc.check_stream(A, m1, tmp_path, sym=True, perm=perm)
    n_pad = sc.untouched_positions(before, after, plan)
    print("%d of %d positions hold no entry, LDS of a norms launch %d doubles" % (n_pad, plan.size, ssc.lds_doubles(after)))
    whole = lo == 0 and hi == n
    assert vc.check_entries(A, m1, rows=None if whole else (lo, hi), limit=300, sym=True) > 0     # (caller's numbering)
    want_d = m1.diagonal() if perm is None else m1.diagonal()[np.argsort(perm)]
    got_d = A.get_diag_host()
    assert np.array_equal(bits(got_d[lo:hi]), bits(want_d[lo:hi]))
    ssc.check_all_norms(norms_into_sentinels(A, n), vc.with_values(csr, v1), lo, hi, perm)
    with pytest.raises(SpxError):
        A.export_csx(A.info().first_partition)
    return before, v1


@pytest.fixture(params=list(TUNES))
def tuned(request):
    gen, opts, reorder = TUNES[request.param]
    csr = gen()
    A = vc.tune(csr, opts, sym=True, host_only=True, reorder=reorder)
    inf = A.info()
    assert inf.symmetric and not inf.on_device
    yield request.param, A, csr, (A.get_perm().astype(np.int64) if reorder else None)
    A.destroy()
    sx.options_reset()


def test_norms_and_scaled_values_in_every_stored_copy(tuned, tmp_path):
    name, A, csr, perm = tuned
    n = csr[3]
    ssc.check_all_norms(norms_into_sentinels(A, n), csr, perm=perm)
    out = A.sym_norms_host(sx.NORM_MAX_ABS)                       # a new array
    assert out.shape == (n,) and np.array_equal(bits(out), bits(ssc.expected_norms(csr, sx.NORM_MAX_ABS, perm=perm)[0]))
    before, v1 = scale_and_check(A, csr, tmp_path, perm)
    # the stream holds what the case is there for
    kinds = set(int(k) for k in np.unique(before.passes["kind"]))
    print("%s: pass kinds %r" % (name, sorted(kinds)))
    if name.startswith("nd24k"):
        assert 3 in kinds, "no pass of 8x8 tiles"
    if name == "kkt44-pipeline":
        assert 5 in kinds and (before.passes["flags"][before.passes["kind"] == 5] & 1).any(), "no read-once segments with inline headers"
    if name == "kkt20-no-once":
        assert not kinds & {3, 5}
    # a refresh overwrites with what the caller hands over
    A.set_values(csr[2].copy())
    back = vc.check_stream(A, vc.to_scipy(csr), tmp_path, sym=True, perm=perm)
    assert np.array_equal(bits(back.values), bits(before.values)) and np.array_equal(bits(back.dvalues), bits(before.dvalues))


def test_power_of_two_round_trip_saves_the_same_file(tuned, tmp_path):
    name, A, csr, perm = tuned
    n = csr[3]
    A.values_plan(csr[0], csr[1])
    A.set_values(csr[2].copy())              # (no-op: both files are written under the same stale-partition rule)
    f0, f1 = str(tmp_path / "f0.spx"), str(tmp_path / "f1.spx")
    A.save(f0)
    p = ssc.pow2_vector(n, 3)
    assert set(np.unique(p)) <= set(2.0 ** np.arange(-3, 4)) and np.unique(p).size > 3
    A.sym_scale(p)
    vc.check_stream(A, ssc.scaled_matrix(csr, p, perm)[1], tmp_path, sym=True, perm=perm)
    with pytest.raises(SpxError):
        A.export_csx(A.info().first_partition)
    A.sym_scale(1.0 / p)
    A.save(f1)
    with open(f0, "rb") as a, open(f1, "rb") as b:
        assert a.read() == b.read()
    A.export_csx(A.info().first_partition)                      # the first values are back: nothing is stale


@pytest.mark.parametrize("case", list(SLICES))
def test_three_slices_and_their_joined_norms(case, tmp_path):
    how = SLICES[case]
    mname, world, kind, extra, _, _ = dc.CASES[case]
    assert world == 3
    csr = dc.matrix(case)
    rp, ci, va, n = csr
    cuts = dc.cut(csr, world, kind)
    opts = dict(dc.NOSAMPLE, **extra)
    parts = {k: [] for k in ssc.KINDS}
    counts = {k: [] for k in ssc.KINDS}
    mirror = []
    for rank in range(world):
        if how == "rank":
            A = dc.tune_rank(csr, rank, world, opts, symmetric=True, host_only=True)
            plan_csr = csr
        else:
            lo, hi = cuts[rank], cuts[rank + 1]
            A = dc.tune_rows(csr, lo, hi, opts, symmetric=True, host_only=True)
            plan_csr = ((rp[lo:hi + 1] - rp[lo]).astype(np.int32), ci[rp[lo]:rp[hi]].copy(), None, n)
        inf = A.info()
        lo, hi = inf.row_lo, inf.row_hi
        assert inf.symmetric and not inf.on_device and 0 <= lo < hi <= n and hi - lo < n
        ssc.check_all_norms(norms_into_sentinels(A, n), csr, lo, hi)
        for k in ssc.KINDS:
            parts[k].append(A.sym_norms_host(k))
            counts[k].append(ssc.expected_norms(csr, k, lo, hi)[1])
        before, _ = scale_and_check(A, csr, tmp_path, None, lo, hi, plan_csr)
        mirror.append(int(before.mirror_rows.size))
        A.destroy()
    sx.options_reset()
    print("%s (%s): rows in the thin mirror lists %r" % (case, how, mirror))
    if case == dc.THIN_MIRROR:
        assert mirror[-1] > 0, "the last slice has no thin mirror list"
    for k in ssc.KINDS:
        ssc.check_joined(k, parts[k], counts[k], csr)
