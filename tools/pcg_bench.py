"""Time per Jacobi-PCG iteration, fused against pieced together, next to the unpreconditioned CG iteration.

  (a) fused  : the product, spx_hip_vec_mul_dev(p, ap), spx_hip_vec_pcg_update, spx_hip_vec_pcg_direction
               (11 vector passes in the two new calls, no z vector)
  (b) pieced : the same step from the calls that were there before plus spx_hip_vec_mul_elem --
               spx_hip_vec_scale_add_ratio twice (x, r), mul_elem (z), spx_hip_vec_mul_dev twice (z.r, r.r) and
               spx_hip_vec_scale_add_ratio (p): 15 passes
  (c) CG     : the unpreconditioned device-scalar iteration of tools/cg_bench.py, form (b) there

The protocol of tools/cg_bench.py: HIP-event time over a batch of iterations after a warm-up, the median of 5
batches, min .. max of the batches as the spread, the forms alternating batch by batch.  Also timed alone: the
product, and spx_hip_mat_get_diag.  Last, the iterations plain CG and Jacobi-PCG need on syn-cant scaled as D A D
(d = 10^uniform(-1, 1)) for r.r <= 1e-20 of its start.  Prints markdown tables.

    python tools/pcg_bench.py [--iters 50] [--edge 120] [--scale 1.0] [--skip-matrices] [--skip-counts] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np
import scipy.sparse as sp
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sparsex_amd as sx  # noqa: E402
from sparsex_amd import synth  # noqa: E402

BATCHES = 5


def timed(fn):
    """HIP-event seconds of fn() (which only enqueues) on the current stream."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3


def stats(ts):
    return float(np.median(ts)), float(min(ts)), float(max(ts))


class Solver:
    def __init__(self, A, n, b=None):
        self.A, self.n = A, n
        self.b = sx.DeviceVector(host=np.random.RandomState(1).uniform(-1, 1, n) if b is None else b)
        self.x, self.r, self.p, self.ap, self.z, self.minv = (sx.DeviceVector(n) for _ in range(6))
        self.S = sx.DeviceVector(5)          # rz, pap, beta, rr and (pieced form) the other rz
        A.diag_plan()
        A.get_diag(self.minv)
        self.minv.reciprocal_into(self.minv, 1.0)

    def reset_pcg(self):
        for v in (self.x, self.p, self.ap, self.S):
            v.init(0.0)
        self.b.copy_into(self.r)
        sx.pcg_update(self.x, self.p, self.r, self.ap, self.minv, self.S)     # the start-up call: rz, rr
        sx.pcg_direction(self.p, self.r, self.minv)
        torch.cuda.synchronize()

    def reset_cg(self):
        self.x.init(0.0)
        self.b.copy_into(self.r)
        self.r.copy_into(self.p)
        self.r.dot_into(self.r, self.S, 0)
        torch.cuda.synchronize()

    def fused_iters(self, k, stream=0):
        x, r, p, ap, m, S = self.x, self.r, self.p, self.ap, self.minv, self.S
        for _ in range(k):
            sx.matvec_kernel_vec(self.A, 1.0, p, 0.0, ap, stream)
            p.dot_into(ap, S, 1, stream)
            sx.pcg_update(x, p, r, ap, m, S, stream)
            sx.pcg_direction(p, r, m, S, stream)

    def pieced_iters(self, k, stream=0):
        """rz lives in slot 0 and slot 4 in turn (k even: it ends where it began)"""
        x, r, p, ap, z, m, S = self.x, self.r, self.p, self.ap, self.z, self.minv, self.S
        old, new = 0, 4
        for _ in range(k):
            sx.matvec_kernel_vec(self.A, 1.0, p, 0.0, ap, stream)
            p.dot_into(ap, S, 1, stream)
            x.scale_add_ratio_into(p, x, 1.0, (S, old), (S, 1), stream=stream)
            r.scale_add_ratio_into(ap, r, -1.0, (S, old), (S, 1), stream=stream)
            m.mul_elem_into(r, z, stream)
            z.dot_into(r, S, new, stream)
            r.dot_into(r, S, 3, stream)
            z.scale_add_ratio_into(p, p, 1.0, (S, new), (S, old), stream=stream)
            old, new = new, old

    def cg_iters(self, k, stream=0):
        x, r, p, ap, S = self.x, self.r, self.p, self.ap, self.S
        for _ in range(k):
            sx.matvec_kernel_vec(self.A, 1.0, p, 0.0, ap, stream)
            p.dot_into(ap, S, 1, stream)
            sx.cg_update(x, p, r, ap, S, stream)
            r.scale_add_ratio_into(p, p, 1.0, (S, 2), stream=stream)


def tuned(csr, sym=False, opts=None):
    rp, ci, va, n = csr
    sx.options_reset()
    for k, v in (opts or {}).items():
        sx.option_set(k, v)
    if sym:
        sx.option_set("spx.matrix.symmetric", "true")
    inp = sx.input_load_csr(rp, ci, va, n, n)
    A = sx.mat_tune(inp)
    A._input = inp
    return A


def bench_matrix(name, csr, iters):
    n = csr[3]
    A = tuned(csr)
    s = Solver(A, n)
    iters += iters & 1
    s.reset_pcg()
    s.fused_iters(2)                           # warm-up of every kernel used below
    s.pieced_iters(2)
    s.cg_iters(2)
    A.get_diag(s.z)
    torch.cuda.synchronize()
    forms = {"a": (s.reset_pcg, lambda: s.fused_iters(iters)), "b": (s.reset_pcg, lambda: s.pieced_iters(iters)),
             "c": (s.reset_cg, lambda: s.cg_iters(iters))}
    ts = {k: [] for k in forms}
    spmv, diag = [], []
    for _ in range(BATCHES):
        for k, (reset, fn) in forms.items():
            reset()
            ts[k].append(timed(fn) / iters)
        spmv.append(timed(lambda: [sx.matvec_kernel_vec(A, 1.0, s.p, 0.0, s.ap) for _ in range(iters)]) / iters)
        diag.append(timed(lambda: [A.get_diag(s.z) for _ in range(iters)]) / iters)
    rows = []
    for k, label in [("a", "(a) PCG, fused update and direction"), ("b", "(b) PCG, pieced from eight calls"),
                     ("c", "(c) CG, device scalars")]:
        med, lo, hi = stats(ts[k])
        rows.append("| %s | %d | %s | %.1f | %.1f .. %.1f | %.3f |" % (name, n, label, med * 1e6, lo * 1e6, hi * 1e6,
                                                                       med / stats(ts["b"])[0]))
    for label, t in (("the product alone", spmv), ("spx_hip_mat_get_diag alone", diag)):
        med, lo, hi = stats(t)
        rows.append("| %s | %d | %s | %.1f | %.1f .. %.1f | |" % (name, n, label, med * 1e6, lo * 1e6, hi * 1e6))
    pm = stats(spmv)[0]
    rows.append("| %s | %d | BLAS-1 part, (a) / (b) | %.3f | | (11 / 15 = 0.733 by bytes) |" % (
        name, n, (stats(ts["a"])[0] - pm) / (stats(ts["b"])[0] - pm)))
    A.destroy()
    return rows


def iteration_counts(scale, limit):
    """plain CG against Jacobi-PCG on syn-cant scaled as D A D: iterations until r.r <= 1e-20 of its start"""
    rp, ci, va, n = synth.syn_cant(scale)
    a = sp.csr_matrix((va, ci, rp), shape=(n, n))
    d = sp.diags(10.0 ** np.random.RandomState(11).uniform(-1, 1, n))
    low = sp.tril(d @ a @ d).tocsr()
    m = (low + sp.tril(low, -1).T).tocsr()
    m.sort_indices()
    csr = (m.indptr.astype(np.int32), m.indices.astype(np.int32), m.data.copy(), n)
    A = tuned(csr)
    s = Solver(A, n, m @ np.random.RandomState(3).uniform(-1, 1, n))
    rows = []
    for label, reset, step, slot in (("Jacobi-PCG", s.reset_pcg, s.fused_iters, 3), ("CG", s.reset_cg, s.cg_iters, 0)):
        reset()
        rr0 = rr = s.S.download()[slot]
        its = 0
        while rr > 1e-20 * rr0 and its < limit:
            step(1)
            rr = s.S.download()[slot]
            its += 1
        res = np.linalg.norm(m @ s.x.download() - s.b.download()) / np.linalg.norm(s.b.download())
        rows.append("| syn-cant x %.2g, D A D | %d | %s | %d%s | %.2e | %.2e |" % (
            scale, n, label, its, "" if rr <= 1e-20 * rr0 else " (limit)", rr / rr0, res))
    A.destroy()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50, help="iterations per batch (at least 50 for a record)")
    ap.add_argument("--edge", type=int, default=120, help="grid edge of syn-nlpkkt")
    ap.add_argument("--scale", type=float, default=1.0, help="size factor of syn-cant")
    ap.add_argument("--count-scale", type=float, default=0.05, help="size factor of the scaled syn-cant of the iteration counts")
    ap.add_argument("--count-limit", type=int, default=2000)
    ap.add_argument("--skip-matrices", action="store_true")
    ap.add_argument("--skip-counts", action="store_true")
    ap.add_argument("--out", default=None, help="also write the tables to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("pcg_bench.py measures on the GPU; there is none")
    torch.cuda.set_device(0)
    out = ["| matrix | rows | form | us / iteration (median of %d batches x %d) | min .. max | this / (b) |" % (
        BATCHES, args.iters), "|---|---|---|---|---|---|"]
    if not args.skip_matrices:
        for name, gen in (("syn-cant", lambda: synth.syn_cant(args.scale)),
                          ("syn-nlpkkt edge %d" % args.edge, lambda: synth.syn_nlpkkt_rows(args.edge))):
            out += bench_matrix(name, gen(), args.iters)
            print("\n".join(out[-6:]), flush=True)
    if not args.skip_counts:
        out += ["", "| system | rows | method | iterations to r.r <= 1e-20 r0.r0 | r.r / r0.r0 | \\|Ax-b\\| / \\|b\\| |",
                "|---|---|---|---|---|---|"]
        out += iteration_counts(args.count_scale, args.count_limit)
    text = "\n".join(out)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
