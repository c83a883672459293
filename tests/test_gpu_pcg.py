"""A diagonal preconditioner on the device: the elementwise helpers (spx_hip_vec_mul_elem, spx_hip_vec_reciprocal)
and the fused Jacobi-PCG step (spx_hip_vec_pcg_update, spx_hip_vec_pcg_direction).  The elementwise results are
pinned bitwise to numpy and to the calls the fused ones replace, r.r to spx_hip_vec_cg_update; a captured solve of
a badly scaled SPD system converges where plain CG does not."""
import functools
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import sparsex_amd as sx
from sparsex_amd import synth
from helpers import ROOT, FP64_BOUND_FACTOR, tune

pytestmark = pytest.mark.gpu

# the sizes of test_gpu_vec_scalars.py: the odd tail, one chunk, a chunk boundary, all eight XCD lists, several chunks
SIZES = [1, 2, 3, 63, 64, 2047, 2048, 2049, 8193, 16 * 2048 + 1, (1 << 20) + 2049]
SENTINEL = 7.0


@functools.lru_cache(maxsize=None)
def _host(n, seed=0):
    """x, p, r, ap in (-1, 1) and minv in (0.25, 4) (shared by the tests of one size; never written to)."""
    rng = np.random.RandomState(n % 97 + 1000 * seed)
    vs = tuple(rng.uniform(-1, 1, n) for _ in range(4)) + (2.0 ** rng.uniform(-2, 2, n),)
    for v in vs:
        v.setflags(write=False)
    return vs


def _dev(*arrs):
    return [sx.DeviceVector(host=np.ascontiguousarray(a)) for a in arrs]


def _scalars(*vals):
    return sx.DeviceVector(host=np.array(vals, dtype=np.float64))


def _bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


# ---- 1. elementwise helpers -----------------------------------------------------------------------------------

@pytest.mark.parametrize("n", SIZES)
def test_mul_elem_is_numpys_product(n):
    a, b, _, _, _ = _host(n)
    A, B = _dev(a, b)
    D = sx.DeviceVector(n)
    A.mul_elem_into(B, D)
    assert _same_bits(D.download(), a * b)
    assert _same_bits(A.download(), a) and _same_bits(B.download(), b)
    A.mul_elem_into(B, A)                                 # dst aliasing either operand
    assert _same_bits(A.download(), a * b)
    A2, = _dev(a)
    A2.mul_elem_into(B, B)
    assert _same_bits(B.download(), a * b)
    A2.mul_elem_into(A2, D)                               # a square
    assert _same_bits(D.download(), a * a)


@pytest.mark.parametrize("n", SIZES)
def test_reciprocal_is_one_division(n):
    a = _host(n)[0].copy()
    a[::7] = 0.0
    a[3::11] = -0.0
    A, = _dev(a)
    D = sx.DeviceVector(n)
    for if_zero in (0.0, 1.0, -2.5):
        A.reciprocal_into(D, if_zero)
        with np.errstate(divide="ignore"):
            want = np.where(a == 0.0, if_zero, 1.0 / a)
        assert _same_bits(D.download(), want), if_zero
    assert _same_bits(A.download(), a)
    A.reciprocal_into(A, 1.0)                             # in place
    with np.errstate(divide="ignore"):
        assert _same_bits(A.download(), np.where(a == 0.0, 1.0, 1.0 / a))


# ---- 2. the fused update -------------------------------------------------------------------------------------------

def _run_pcg_update(n, rz, pap, hs=None):
    xh, ph, rh, aph, mh = hs or _host(n)
    x, p, r, ap, m = _dev(xh, ph, rh, aph, mh)
    S = _scalars(rz, pap, SENTINEL, SENTINEL, SENTINEL)
    sx.pcg_update(x, p, r, ap, m, S)
    return x.download(), r.download(), S.download(), p.download(), ap.download(), m.download()


def _run_cg_update(n, rr, pap, hs=None):
    xh, ph, rh, aph, _ = hs or _host(n)
    x, p, r, ap = _dev(xh, ph, rh, aph)
    S = _scalars(rr, pap, SENTINEL)
    sx.cg_update(x, p, r, ap, S)
    return x.download(), r.download(), S.download()


def _check_update(n, rz, pap, hs=None):
    _, ph, _, aph, mh = hs or _host(n)
    xg, rg, s, pg, apg, mg = _run_pcg_update(n, rz, pap, hs)
    xc, rc, sc = _run_cg_update(n, rz, pap, hs)           # the same ratio a = rz / pap
    assert _same_bits(xg, xc) and _same_bits(rg, rc)
    assert _same_bits(s[3], sc[0])                         # rr: the bits the CG update leaves
    assert _same_bits(pg, ph) and _same_bits(apg, aph) and _same_bits(mg, mh)
    exact = float(np.dot(mh * rg, rg))
    scale = float(np.sum(np.abs(mh * rg * rg)))
    print("n=%d rz_new=%.17g numpy=%.17g |diff|/sum=%.3e" % (n, s[0], exact, abs(s[0] - exact) / scale))
    assert abs(s[0] - exact) <= FP64_BOUND_FACTOR * 2.0 ** -53 * scale
    assert _same_bits(s[2], s[0] / rz)                     # beta = rz_new / rz_old, one division
    assert s[1] == pap and s[4] == SENTINEL
    return xg, rg, s


@pytest.mark.parametrize("n", SIZES)
def test_pcg_update_matches_the_cg_update(n):
    rz, pap = 0.37 * n, 1.3 * n / 7.0
    xg, rg, s = _check_update(n, rz, pap)
    # a second run on the same inputs: the same bits everywhere
    xg2, rg2, s2, _, _, _ = _run_pcg_update(n, rz, pap)
    assert _same_bits(xg2, xg) and _same_bits(rg2, rg) and _same_bits(s2, s)


def test_pcg_update_with_a_long_chunk():
    """2048 chunks of 2048 pairs of doubles and an odd last element: the size at which the chunk grows"""
    n = 2 * 2048 * 2048 + 5
    rng = np.random.RandomState(5)
    hs = tuple(rng.uniform(-1, 1, n) for _ in range(4)) + (2.0 ** rng.uniform(-2, 2, n),)
    _check_update(n, 0.37 * n, 1.3 * n / 7.0, hs)


@pytest.mark.parametrize("n", SIZES)
def test_pcg_update_zero_rules_and_start_up(n):
    xh, ph, rh, aph, mh = _host(n)
    exact_rr, exact_rz = float(np.dot(rh, rh)), float(np.dot(mh * rh, rh))
    scale = float(np.sum(np.abs(mh * rh * rh)))
    tol_rr, tol_rz = FP64_BOUND_FACTOR * 2.0 ** -53 * exact_rr, FP64_BOUND_FACTOR * 2.0 ** -53 * scale
    # pap == 0: a = 0, x and r stay; rz, rr and beta are still those of r
    xg, rg, s, _, _, _ = _run_pcg_update(n, 2.5, 0.0)
    assert _same_bits(xg, xh) and _same_bits(rg, rh)
    assert abs(s[0] - exact_rz) <= tol_rz and abs(s[3] - exact_rr) <= tol_rr and _same_bits(s[2], s[0] / 2.5)
    # rz == 0: a = 0 and beta = 0
    xg, rg, s, _, _, _ = _run_pcg_update(n, 0.0, 1.5)
    assert _same_bits(xg, xh) and _same_bits(rg, rh)
    assert s[2] == 0.0 and abs(s[0] - exact_rz) <= tol_rz and abs(s[3] - exact_rr) <= tol_rr
    # both: the start-up call -- x and r alone, rz0 and rr0 written, beta = 0; then p0 = minv .* r
    x, p, r, ap, m = _dev(xh, ph, rh, aph, mh)
    S = _scalars(0.0, 0.0, SENTINEL, SENTINEL, SENTINEL)
    sx.pcg_update(x, p, r, ap, m, S)
    sx.pcg_direction(p, r, m)
    s = S.download()
    assert _same_bits(x.download(), xh) and _same_bits(r.download(), rh)
    assert abs(s[0] - exact_rz) <= tol_rz and abs(s[3] - exact_rr) <= tol_rr
    assert s[1] == 0.0 and s[2] == 0.0 and s[4] == SENTINEL
    assert _same_bits(p.download(), mh * rh)
    # r = p = 0: nothing becomes NaN, whatever the scalars
    zero = np.zeros(n)
    for rz, pap in [(0.0, 0.0), (2.5, 0.0), (0.0, 1.5), (2.5, 1.5)]:
        x, p, r, ap, m = _dev(xh, zero, zero, zero, mh)
        S = _scalars(rz, pap, SENTINEL, SENTINEL)
        sx.pcg_update(x, p, r, ap, m, S)
        sx.pcg_direction(p, r, m, S)
        s = S.download()
        assert _same_bits(x.download(), xh) and not r.download().any() and not p.download().any()
        assert s[0] == 0.0 and s[2] == 0.0 and s[3] == 0.0 and s[1] == pap


# ---- 3. the search direction ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", SIZES)
def test_pcg_direction_matches_mul_elem_and_scale_add(n):
    _, ph, rh, _, mh = _host(n)
    for beta in (0.8125 + 1.0 / 3.0, -1.7 / 9.0, 0.0):
        p, r, m = _dev(ph, rh, mh)
        z = sx.DeviceVector(n)
        m.mul_elem_into(r, z)
        zh = z.download()
        z.scale_add_into(p, p, beta)                      # p <- z + beta p
        want = p.download()
        p2, = _dev(ph)
        S = _scalars(SENTINEL, SENTINEL, beta, SENTINEL)
        sx.pcg_direction(p2, r, m, S)
        assert _same_bits(p2.download(), want), beta
        assert _same_bits(r.download(), rh) and _same_bits(m.download(), mh)
        assert _same_bits(S.download(), [SENTINEL, SENTINEL, beta, SENTINEL])
    p3, = _dev(ph)
    sx.pcg_direction(p3, r, m)                            # no beta: the bits of z
    assert _same_bits(p3.download(), zh) and _same_bits(zh, mh * rh)


# ---- 4. refused calls change nothing ------------------------------------------------------------------------------

def test_refused_calls_leave_their_inputs_alone():
    n = 2049
    hs = _host(n)
    x, p, r, ap, m = _dev(*hs)
    short = sx.DeviceVector(host=np.arange(5.0))
    sh = np.array([2.0, 3.0, SENTINEL, SENTINEL])
    S = sx.DeviceVector(host=sh.copy())
    vs = (x, p, r, ap, m)

    def unchanged():
        return (all(_same_bits(v.download(), h) for v, h in zip(vs, hs)) and _same_bits(S.download(), sh) and
                _same_bits(short.download(), np.arange(5.0)))

    def ptrs(*slots):
        return [S.slot_ptr(k) for k in slots]

    refused = [
        # size mismatch
        lambda: sx.pcg_update(short, p, r, ap, m, S),
        lambda: sx.pcg_update(x, p, r, short, m, S),
        lambda: sx.pcg_update(x, p, r, ap, short, S),
        lambda: sx.pcg_direction(p, short, m, S),
        lambda: sx.pcg_direction(p, r, short),
        lambda: x.mul_elem_into(short, x),
        lambda: x.mul_elem_into(p, short),
        lambda: x.reciprocal_into(short),
        # the same vector twice
        lambda: sx.pcg_update(x, x, r, ap, m, S),
        lambda: sx.pcg_update(x, p, r, r, m, S),
        lambda: sx.pcg_update(x, p, p, ap, m, S),
        lambda: sx.pcg_update(x, p, r, ap, r, S),
        lambda: sx.pcg_update(x, p, r, ap, p, S),
        lambda: sx.pcg_update(m, p, r, ap, m, S),
        lambda: sx.pcg_direction(p, p, m, S),
        lambda: sx.pcg_direction(p, r, r, S),
        lambda: sx.pcg_direction(p, r, p),
        # the four scalars are not four addresses
        lambda: sx.pcg_update(x, p, r, ap, m, ptrs(0, 0, 2, 3)),
        lambda: sx.pcg_update(x, p, r, ap, m, ptrs(0, 1, 1, 3)),
        lambda: sx.pcg_update(x, p, r, ap, m, ptrs(0, 1, 2, 2)),
        lambda: sx.pcg_update(x, p, r, ap, m, ptrs(0, 1, 2, 0)),
        # a scalar inside a vector the call writes
        lambda: sx.pcg_update(x, p, r, ap, m, r),
        lambda: sx.pcg_update(x, p, r, ap, m, x),
        lambda: sx.pcg_update(x, p, r, ap, m, ptrs(0, 1, 2) + [x.slot_ptr(n - 1)]),
        lambda: sx.pcg_update(x, p, r, ap, m, ptrs(0) + [r.slot_ptr(0)] + ptrs(2, 3)),
        lambda: sx.pcg_direction(p, r, m, p),
        lambda: sx.pcg_direction(p, r, m, p.slot_ptr(n - 1)),
        # a NULL scalar
        lambda: sx.pcg_update(x, p, r, ap, m, None),
        lambda: sx.pcg_update(x, p, r, ap, m, ptrs(0, 1, 2) + [None]),
        lambda: sx.pcg_update(x, p, r, ap, m, [None] + ptrs(1, 2, 3)),
    ]
    for k, call in enumerate(refused):
        with pytest.raises(sx.SpxError):
            call()
        assert unchanged(), k
    L = sx.lib()
    assert L.spx_hip_vec_pcg_update(None, p.handle, r.handle, ap.handle, m.handle, *ptrs(0, 1, 2, 3), None) == sx.SPX_FAILURE
    assert L.spx_hip_vec_pcg_direction(p.handle, None, m.handle, None, None) == sx.SPX_FAILURE
    assert L.spx_hip_vec_mul_elem(x.handle, None, x.handle, None) == sx.SPX_FAILURE
    assert L.spx_hip_vec_reciprocal(None, x.handle, 0.0, None) == sx.SPX_FAILURE
    assert unchanged()


# ---- 5. a captured solve ---------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _scaled_system():
    """syn-cant scaled as D A D, d = 10^uniform(-1, 1): SPD, diagonal entries over four decades.  The product in
    floating point is symmetric only to 1e-14, so the lower triangle is mirrored: one matrix for both tunes."""
    rp, ci, va, n = synth.syn_cant(0.05)
    a = sp.csr_matrix((va, ci, rp), shape=(n, n))
    d = sp.diags(10.0 ** np.random.RandomState(11).uniform(-1, 1, n))
    low = sp.tril(d @ a @ d).tocsr()
    m = (low + sp.tril(low, -1).T).tocsr()
    m.sort_indices()
    assert (m != m.T).nnz == 0
    b = m @ np.random.RandomState(3).uniform(-1, 1, n)
    return m, (m.indptr.astype(np.int32), m.indices.astype(np.int32), m.data.copy(), n), b


class _Pcg:
    """Jacobi-PCG with the scalars rz, pap, beta, rr in the device vector S; and plain CG on the same system."""

    def __init__(self, sym, opts):
        self.a, csr, self.bh = _scaled_system()
        self.n = n = csr[3]
        self.M = tune(csr, opts, sym=sym)
        self.M.diag_plan()
        self.minv = sx.DeviceVector(n)
        self.M.get_diag(self.minv)
        assert _same_bits(self.minv.download(), self.a.diagonal())
        self.minv.reciprocal_into(self.minv)
        self.b = sx.DeviceVector(host=self.bh)
        self.x, self.r, self.p, self.ap = (sx.DeviceVector(n) for _ in range(4))
        self.S = sx.DeviceVector(4)

    def reset(self):
        """x0 = 0, r0 = b, then the start-up idiom; returns r0 . r0"""
        for v in (self.x, self.p, self.ap, self.S):
            v.init(0.0)
        self.b.copy_into(self.r)
        sx.pcg_update(self.x, self.p, self.r, self.ap, self.minv, self.S)
        sx.pcg_direction(self.p, self.r, self.minv)
        return self.S.download()[3]

    def iteration(self, stream=0):
        sx.matvec_kernel_vec(self.M, 1.0, self.p, 0.0, self.ap, stream)
        self.p.dot_into(self.ap, self.S, 1, stream)
        sx.pcg_update(self.x, self.p, self.r, self.ap, self.minv, self.S, stream)
        sx.pcg_direction(self.p, self.r, self.minv, self.S, stream)

    def plain_cg(self, iterations):
        """the unpreconditioned device-scalar loop of test_gpu_vec_scalars.py; returns rr / rr0 after `iterations`"""
        S = sx.DeviceVector(3)
        self.x.init(0.0)
        self.b.copy_into(self.r)
        self.r.copy_into(self.p)
        self.r.dot_into(self.r, S, 0)
        rr0 = S.download()[0]
        for _ in range(iterations):
            sx.matvec_kernel_vec(self.M, 1.0, self.p, 0.0, self.ap)
            self.p.dot_into(self.ap, S, 1)
            sx.cg_update(self.x, self.p, self.r, self.ap, S)
            self.r.scale_add_ratio_into(self.p, self.p, 1.0, (S, 2))
        return S.download()[0] / rr0


@pytest.mark.parametrize("sym,opts,bitwise", [
    (False, {"spx.gpu.deterministic": "true", "spx.preproc.sampling": "none"}, True),
    (True, {}, False),                        # global atomics: the order of addition is not fixed
], ids=["general-deterministic", "symmetric-default"])
def test_captured_pcg_converges_where_cg_does_not(sym, opts, bitwise):
    """Five iterations captured into a graph and replayed.  The numpy reference of this system reaches
    rr <= 1e-20 rr0 at iteration 13; plain CG has reduced rr by 1.8e-5 after 40.  The fixed point of the zero rules
    is rz == 0 (r underflows after some 200 iterations): ten replays beyond it must leave x bit-identical."""
    import torch
    K = 5
    cg = _Pcg(sym, opts)
    cg.reset()
    cg.iteration()                            # warm-up outside the capture
    torch.cuda.synchronize()
    rr0 = cg.reset()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = torch.cuda.current_stream().cuda_stream
        for _ in range(K):
            cg.iteration(cap)
    # (the capture ran nothing; the state is still the reset one)
    replays, rr = 0, rr0
    while rr > 1e-20 * rr0 and replays < 40 // K:
        g.replay()
        torch.cuda.synchronize()
        rr = cg.S.download()[3]
        replays += 1
    print("%d replays of %d iterations, rr/rr0=%.3e" % (replays, K, rr / rr0))
    assert rr <= 1e-20 * rr0
    xg = cg.x.download()
    bnorm = np.linalg.norm(cg.bh)
    print("|Ax-b|/|b|=%.3e" % (np.linalg.norm(cg.a @ xg - cg.bh) / bnorm))
    assert np.linalg.norm(cg.a @ xg - cg.bh) <= 1e-9 * bnorm
    # on to the fixed point, then ten replays beyond it
    more, rz = 0, cg.S.download()[0]
    while rz != 0.0 and more < 400:
        g.replay()
        torch.cuda.synchronize()
        rz = cg.S.download()[0]
        more += 1
    assert rz == 0.0, (more, rz)
    xfix = cg.x.download()
    for _ in range(10):
        g.replay()
    torch.cuda.synchronize()
    xend, s = cg.x.download(), cg.S.download()
    print("rz == 0 after %d further replays; scalars then %s" % (more, s))
    assert np.isfinite(xend).all() and np.isfinite(s).all()
    assert _same_bits(xend, xfix)
    assert np.linalg.norm(cg.a @ xend - cg.bh) <= 1e-9 * bnorm
    # the same number of iterations issued on the stream, no graph
    cg.reset()
    for _ in range(K * replays):
        cg.iteration()
    xs = cg.x.download()
    if bitwise:
        assert _same_bits(xs, xg)
    assert np.linalg.norm(cg.a @ xs - cg.bh) <= 1e-9 * bnorm
    # plain CG on the same system, 40 iterations
    left = cg.plain_cg(40)
    print("plain CG: rr/rr0 after 40 iterations = %.3e" % left)
    assert left > 1e-10


# ---- 6. the plain C client ---------------------------------------------------------------------------------------

def test_c_example_compiles_and_solves(tmp_path):
    """examples/pcg_device.c: diag_plan + get_diag_vec + reciprocal, then the four-call loop."""
    exe = str(tmp_path / "pcg_device")
    subprocess.check_call(["gcc", "-std=gnu99", "-Wall", "-Werror", os.path.join(ROOT, "examples", "pcg_device.c"),
                           "-I" + os.path.join(ROOT, "include"), "-L" + os.path.dirname(sx.lib_path()),
                           "-lsparsex", "-Wl,-rpath," + os.path.dirname(sx.lib_path()), "-lm", "-o", exe])
    out = subprocess.check_output([exe, "60"]).decode()     # exit status 0: max |x - 1| < 1e-6
    assert "PCG iterations" in out
