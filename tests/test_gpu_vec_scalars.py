"""Device-side scalars (spx_hip_vec_mul_dev, spx_hip_vec_scale_add_ratio) and the fused CG update
(spx_hip_vec_cg_update): a solver loop whose scalars never leave HBM, so that it neither stalls the stream nor
refuses to be captured into a graph.  The elementwise results are pinned bitwise to the host-scalar calls they
replace, the dot product to spx_hip_vec_mul."""
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

# the odd tail, one chunk (1024 pairs of doubles where a kernel writes), a chunk boundary, all eight XCD lists,
# several chunks per workgroup of the dot product
SIZES = [1, 2, 3, 63, 64, 2047, 2048, 2049, 8193, 16 * 2048 + 1, (1 << 20) + 2049]
SENTINEL = 7.0


@functools.lru_cache(maxsize=None)
def _host(n):
    """Four host vectors of n doubles (shared by the tests of one size; never written to)."""
    rng = np.random.RandomState(n % 97)
    vs = tuple(rng.uniform(-1, 1, n) for _ in range(4))
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


# ---- 1. the dot product into a device scalar ------------------------------------------------------------------

@pytest.mark.parametrize("n", SIZES)
def test_dot_into_returns_the_bits_of_dot(n):
    a, b, _, _ = _host(n)
    A, B = _dev(a, b)
    S = _scalars(SENTINEL, SENTINEL, SENTINEL)
    A.dot_into(B, S, 1)
    s = S.download()
    assert _same_bits(s[1], A.dot(B))
    assert s[0] == SENTINEL and s[2] == SENTINEL          # the neighbours are not touched
    A.dot_into(A, S, 2)                                   # (a norm: the kernel that loads every line once)
    s = S.download()
    assert _same_bits(s[2], A.dot(A)) and s[0] == SENTINEL


def test_dot_into_of_empty_vectors_is_zero():
    A, B = sx.DeviceVector(0), sx.DeviceVector(0)
    S = _scalars(SENTINEL, SENTINEL)
    A.dot_into(B, S, 0)
    assert list(S.download()) == [0.0, SENTINEL]


# ---- 2. axpy with a coefficient formed on the device ----------------------------------------------------------

@pytest.mark.parametrize("n", SIZES)
def test_scale_add_ratio_matches_host_coefficient(n):
    a, b, _, _ = _host(n)
    num, den = 0.8125 + 1.0 / 3.0, 1.7 / 9.0
    S = _scalars(num, den, 0.0)
    A, B = _dev(a, b)
    got, ref = sx.DeviceVector(n), sx.DeviceVector(n)
    # scale = -1 (r -= alpha * Ap), a scale that rounds, and no denominator
    for scale, d in [(-1.0, (S, 1)), (0.3, (S, 1)), (-1.0, None), (0.75, None)]:
        A.scale_add_ratio_into(B, got, scale, (S, 0), d)
        A.scale_add_into(B, ref, scale * (num / den) if d else scale * num)
        assert _same_bits(got.download(), ref.download()), (scale, d is not None)
    # a zero denominator: coefficient 0, dst == self exactly
    A.scale_add_ratio_into(B, got, -1.0, (S, 0), (S, 2))
    assert _same_bits(got.download(), a)
    # dst aliasing self, dst aliasing other
    A.scale_add_into(B, ref, -(num / den))
    A2, = _dev(a)
    A2.scale_add_ratio_into(B, A2, -1.0, (S, 0), (S, 1))
    assert _same_bits(A2.download(), ref.download())
    B2, = _dev(b)
    A.scale_add_ratio_into(B2, B2, -1.0, (S, 0), (S, 1))
    assert _same_bits(B2.download(), ref.download())
    assert _same_bits(S.download(), [num, den, 0.0])      # the scalars are only read


# ---- 3. the fused CG update --------------------------------------------------------------------------------------

def _run_cg_update(n, rr, pap):
    xh, ph, rh, aph = _host(n)
    x, p, r, ap = _dev(xh, ph, rh, aph)
    S = _scalars(rr, pap, SENTINEL, SENTINEL)
    sx.cg_update(x, p, r, ap, S)
    return x.download(), r.download(), S.download(), p.download(), ap.download()


@pytest.mark.parametrize("n", SIZES)
def test_cg_update_matches_two_scale_adds(n):
    xh, ph, rh, aph = _host(n)
    rr, pap = 0.37 * n, 1.3 * n / 7.0
    alpha = rr / pap
    x, p, r, ap = _dev(xh, ph, rh, aph)
    x.scale_add_into(p, x, alpha)
    r.scale_add_into(ap, r, -alpha)
    xref, rref = x.download(), r.download()
    xg, rg, s, pg, apg = _run_cg_update(n, rr, pap)
    assert _same_bits(xg, xref) and _same_bits(rg, rref)
    assert _same_bits(pg, ph) and _same_bits(apg, aph)
    exact = float(np.dot(rg, rg))
    print("n=%d rr_new=%.17g numpy=%.17g |diff|/sum=%.3e" % (n, s[0], exact, abs(s[0] - exact) / exact))
    assert abs(s[0] - exact) <= FP64_BOUND_FACTOR * 2.0 ** -53 * exact
    assert _same_bits(s[2], s[0] / rr)                    # beta = rr_new / rr_old, one division
    assert s[1] == pap and s[3] == SENTINEL
    # a second run on the same inputs: the same bits everywhere
    xg2, rg2, s2, _, _ = _run_cg_update(n, rr, pap)
    assert _same_bits(xg2, xg) and _same_bits(rg2, rg) and _same_bits(s2, s)


# (the fused kernel's chunk is 1024 pairs of doubles below 2048 chunks of twice that: the sizes at which it first takes
# 2048 and 4096 pairs per workgroup, with an odd last element)
@pytest.mark.parametrize("n", [2 * 2048 * 2048 + 5, 4 * 2048 * 2048 + 5])
def test_cg_update_with_long_chunks(n):
    rng = np.random.RandomState(5)
    hs = [rng.uniform(-1, 1, n) for _ in range(4)]
    rr, pap = 0.37 * n, 1.3 * n / 7.0
    alpha = rr / pap
    x, p, r, ap = _dev(*hs)
    S = _scalars(rr, pap, SENTINEL)
    sx.cg_update(x, p, r, ap, S)
    xg, rg, s = x.download(), r.download(), S.download()
    x.upload(hs[0])
    r.upload(hs[2])
    x.scale_add_into(p, x, alpha)
    r.scale_add_into(ap, r, -alpha)
    assert _same_bits(xg, x.download()) and _same_bits(rg, r.download())
    exact = float(np.dot(rg, rg))
    print("n=%d rr_new=%.17g numpy=%.17g |diff|/sum=%.3e" % (n, s[0], exact, abs(s[0] - exact) / exact))
    assert abs(s[0] - exact) <= FP64_BOUND_FACTOR * 2.0 ** -53 * exact
    assert _same_bits(s[2], s[0] / rr) and s[1] == pap
    x.upload(hs[0])
    r.upload(hs[2])
    S.upload(np.array([rr, pap, SENTINEL]))
    sx.cg_update(x, p, r, ap, S)                          # again: the same bits
    assert _same_bits(x.download(), xg) and _same_bits(r.download(), rg) and _same_bits(S.download(), s)


@pytest.mark.parametrize("n", SIZES)
def test_cg_update_zero_denominators(n):
    xh, _, rh, _ = _host(n)
    # pap == 0: alpha = 0, x and r stay; rr and beta are still those of r
    xg, rg, s, _, _ = _run_cg_update(n, 2.5, 0.0)
    assert _same_bits(xg, xh) and _same_bits(rg, rh)
    exact = float(np.dot(rh, rh))
    assert abs(s[0] - exact) <= FP64_BOUND_FACTOR * 2.0 ** -53 * exact
    assert _same_bits(s[2], s[0] / 2.5)
    # rr == 0: alpha = 0 and beta = 0, nothing is NaN
    xg, rg, s, _, _ = _run_cg_update(n, 0.0, 1.5)
    assert _same_bits(xg, xh) and _same_bits(rg, rh)
    assert s[2] == 0.0 and abs(s[0] - exact) <= FP64_BOUND_FACTOR * 2.0 ** -53 * exact
    # both
    xg, rg, s, _, _ = _run_cg_update(n, 0.0, 0.0)
    assert _same_bits(xg, xh) and _same_bits(rg, rh) and s[2] == 0.0 and np.isfinite(s).all()


# ---- 4. refused calls change nothing ------------------------------------------------------------------------------

def test_refused_calls_leave_their_inputs_alone():
    n = 2049
    xh, ph, rh, aph = _host(n)
    x, p, r, ap = _dev(xh, ph, rh, aph)
    short = sx.DeviceVector(host=np.arange(5.0))
    sh = np.array([2.0, 3.0, SENTINEL])
    S = sx.DeviceVector(host=sh.copy())

    def unchanged():
        return (_same_bits(x.download(), xh) and _same_bits(p.download(), ph) and _same_bits(r.download(), rh) and
                _same_bits(ap.download(), aph) and _same_bits(S.download(), sh) and
                _same_bits(short.download(), np.arange(5.0)))

    refused = [
        # size mismatch
        lambda: x.dot_into(short, S, 0),
        lambda: x.scale_add_ratio_into(short, x, 1.0, (S, 0), (S, 1)),
        lambda: x.scale_add_ratio_into(p, short, 1.0, (S, 0), (S, 1)),
        lambda: sx.cg_update(x, p, r, short, S),
        lambda: sx.cg_update(short, p, r, ap, S),
        # the same vector twice
        lambda: sx.cg_update(x, x, r, ap, S),
        lambda: sx.cg_update(x, p, r, r, S),
        lambda: sx.cg_update(x, p, p, ap, S),
        # a scalar inside a vector the call writes
        lambda: sx.cg_update(x, p, r, ap, r),
        lambda: sx.cg_update(x, p, r, ap, x),
        lambda: r.scale_add_ratio_into(p, p, 1.0, (p, 5)),
        lambda: r.scale_add_ratio_into(p, x, 1.0, (S, 0), (x, n - 1)),
        # a NULL scalar
        lambda: r.scale_add_ratio_into(p, p, 1.0, None),
        lambda: sx.cg_update(x, p, r, ap, None),
        # a slot that the scalar vector does not have
        lambda: x.dot_into(p, S, 3),
    ]
    for k, call in enumerate(refused):
        with pytest.raises(sx.SpxError):
            call()
        assert unchanged(), k
    L = sx.lib()
    assert L.spx_hip_vec_mul_dev(x.handle, p.handle, None, None) == sx.SPX_FAILURE
    # rr, pap and beta have to be three addresses
    assert L.spx_hip_vec_cg_update(x.handle, p.handle, r.handle, ap.handle, S.slot_ptr(0), S.slot_ptr(1),
                                   S.slot_ptr(1), None) == sx.SPX_FAILURE
    assert unchanged()


# ---- 5. a captured CG ----------------------------------------------------------------------------------------------

class _Cg:
    """CG on syn-cant with the scalars rr, pap, beta in the device vector S."""

    def __init__(self, sym, opts):
        csr = synth.syn_cant(0.05)            # symmetric, strictly diagonally dominant => SPD
        rp, ci, va, n = csr
        self.n = n
        self.M = tune(csr, opts, sym=sym)
        self.a = sp.csr_matrix((va, ci, rp), shape=(n, n))
        self.bh = self.a @ np.random.RandomState(3).uniform(-1, 1, n)
        self.b = sx.DeviceVector(host=self.bh)
        self.x, self.r, self.p, self.ap = (sx.DeviceVector(n) for _ in range(4))
        self.S = sx.DeviceVector(3)

    def reset(self):
        self.x.init(0.0)
        self.b.copy_into(self.r)              # x0 = 0  =>  r0 = b
        self.r.copy_into(self.p)
        self.S.init(0.0)
        self.r.dot_into(self.r, self.S, 0)
        return self.S.download()[0]

    def iteration(self, stream=0):
        sx.matvec_kernel_vec(self.M, 1.0, self.p, 0.0, self.ap, stream)
        self.p.dot_into(self.ap, self.S, 1, stream)
        sx.cg_update(self.x, self.p, self.r, self.ap, self.S, stream)
        self.r.scale_add_ratio_into(self.p, self.p, 1.0, (self.S, 2), stream=stream)

    def host_scalar_solution(self):
        """The loop of test_cg_on_device_matches_host_solver: two downloads per iteration."""
        x, r, p, ap = self.x, self.r, self.p, self.ap
        rr = rr0 = self.reset()
        its = 0
        while rr > 1e-24 * rr0 and its < 500:
            sx.matvec_kernel_vec(self.M, 1.0, p, 0.0, ap)
            alpha = rr / p.dot(ap)
            x.scale_add_into(p, x, alpha)
            r.scale_add_into(ap, r, -alpha)
            rr_new = r.dot(r)
            r.scale_add_into(p, p, rr_new / rr)
            rr = rr_new
            its += 1
        assert its < 500
        return x.download()


@pytest.mark.parametrize("sym,opts,bitwise", [
    (False, {"spx.gpu.deterministic": "true", "spx.preproc.sampling": "none"}, True),
    (True, {}, False),                        # global atomics: the order of addition is not fixed
], ids=["general-deterministic", "symmetric-default"])
def test_captured_cg_converges_and_replays_past_convergence(sym, opts, bitwise):
    """Five iterations captured into a graph and replayed until rr <= 1e-24 rr0.

    "Beyond convergence": at rr = 1e-24 rr0 the search direction is still some 1e-12 of x, so further iterations
    of any correct CG keep moving the last bits of x; the state that the zero-denominator rules make a fixed point
    is the one the recursion ends in, r.r == 0 (r underflows after some 300 iterations here).  The graph is
    therefore replayed until the downloaded rr is exactly 0, and the ten replays after that must leave x
    bit-identical and finite (without the rules the first of them divides 0 by 0)."""
    import torch
    K = 5
    cg = _Cg(sym, opts)
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
    while rr > 1e-24 * rr0 and replays < 100:
        g.replay()
        torch.cuda.synchronize()
        rr = cg.S.download()[0]
        replays += 1
    assert rr <= 1e-24 * rr0
    xg = cg.x.download()
    bnorm = np.linalg.norm(cg.bh)
    print("%d replays of %d iterations, rr/rr0=%.3e, |Ax-b|/|b|=%.3e" % (
        replays, K, rr / rr0, np.linalg.norm(cg.a @ xg - cg.bh) / bnorm))
    assert np.linalg.norm(cg.a @ xg - cg.bh) <= 1e-10 * bnorm
    # on to the fixed point, then ten replays beyond it
    more = 0
    while rr != 0.0 and more < 400:
        g.replay()
        torch.cuda.synchronize()
        rr = cg.S.download()[0]
        more += 1
    assert rr == 0.0, (more, rr)
    xfix = cg.x.download()
    for _ in range(10):
        g.replay()
    torch.cuda.synchronize()
    xend, s = cg.x.download(), cg.S.download()
    print("rr == 0 after %d further replays; scalars then %s" % (more, s))
    assert np.isfinite(xend).all() and np.isfinite(s).all()
    assert _same_bits(xend, xfix)
    assert np.linalg.norm(cg.a @ xend - cg.bh) <= 1e-10 * bnorm
    # the same number of iterations issued on the stream, no graph
    cg.reset()
    for _ in range(K * replays):
        cg.iteration()
    xs = cg.x.download()
    if bitwise:
        assert _same_bits(xs, xg)
    assert np.linalg.norm(cg.a @ xs - cg.bh) <= 1e-10 * bnorm
    # the host-scalar loop
    xh = cg.host_scalar_solution()
    print("max |x_graph - x_host| / |x_host| = %.3e" % np.max(np.abs(xg - xh) / np.abs(xh)))
    assert np.allclose(xg, xh, rtol=1e-8, atol=0.0)
    assert np.allclose(xs, xh, rtol=1e-8, atol=0.0)


# ---- 6. the plain C client ---------------------------------------------------------------------------------------

def test_async_c_example_compiles_and_solves(tmp_path):
    """examples/cg_device_async.c: the loop of cg_device.c with the device-scalar calls."""
    exe = str(tmp_path / "cg_device_async")
    subprocess.check_call(["gcc", "-std=gnu99", "-Wall", "-Werror", os.path.join(ROOT, "examples", "cg_device_async.c"),
                           "-I" + os.path.join(ROOT, "include"), "-L" + os.path.dirname(sx.lib_path()),
                           "-lsparsex", "-Wl,-rpath," + os.path.dirname(sx.lib_path()), "-lm", "-o", exe])
    out = subprocess.check_output([exe, "60"]).decode()     # exit status 0: max |x - 1| < 1e-6
    assert "CG iterations" in out
