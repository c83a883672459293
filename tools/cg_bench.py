"""Time per CG iteration in three forms, and the fused CG update against the three calls it replaces.

  (a) host scalars : the loop of examples/cg_device.c -- spx_hip_vec_mul downloads p.Ap and r.r, the host
                     divides, spx_hip_vec_scale_add takes the quotient (two stream synchronisations per iteration)
  (b) device scalars on a stream : spx_hip_vec_mul_dev, spx_hip_vec_cg_update, spx_hip_vec_scale_add_ratio
  (c) the calls of (b) captured into a graph of 10 iterations

Every figure is HIP-event time over a batch of iterations after a warm-up, the median of 5 batches (as bench.py);
the min..max of the batches is printed next to it as the spread.  The forms alternate batch by batch so that
they meet the same machine.  Prints a markdown table.

    python tools/cg_bench.py [--iters 50] [--edge 120] [--n 27993600] [--symmetric] [--skip-matrices] [--skip-update] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sparsex_amd as sx  # noqa: E402
from sparsex_amd import synth  # noqa: E402

BATCHES = 5
GRAPH_ITERS = 10


def timed(fn):
    """HIP-event seconds of fn() (which only enqueues, or synchronises by itself) on the current stream."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3


def stats(ts):
    return float(np.median(ts)), float(min(ts)), float(max(ts))


class Cg:
    def __init__(self, A, n):
        self.A, self.n = A, n
        self.b = sx.DeviceVector(host=np.random.RandomState(1).uniform(-1, 1, n))
        self.x, self.r, self.p, self.ap = (sx.DeviceVector(n) for _ in range(4))
        self.S = sx.DeviceVector(3)          # rr, pap, beta

    def reset(self):
        self.x.init(0.0)
        self.b.copy_into(self.r)
        self.r.copy_into(self.p)
        self.r.dot_into(self.r, self.S, 0)
        torch.cuda.synchronize()

    def host_iters(self, k):
        x, r, p, ap = self.x, self.r, self.p, self.ap
        rr = r.dot(r)
        for _ in range(k):
            sx.matvec_kernel_vec(self.A, 1.0, p, 0.0, ap)
            pap = p.dot(ap)
            alpha = rr / pap if pap != 0.0 else 0.0
            x.scale_add_into(p, x, alpha)
            r.scale_add_into(ap, r, -alpha)
            rr_new = r.dot(r)
            r.scale_add_into(p, p, rr_new / rr if rr != 0.0 else 0.0)
            rr = rr_new

    def dev_iters(self, k, stream=0):
        x, r, p, ap, S = self.x, self.r, self.p, self.ap, self.S
        for _ in range(k):
            sx.matvec_kernel_vec(self.A, 1.0, p, 0.0, ap, stream)
            p.dot_into(ap, S, 1, stream)
            sx.cg_update(x, p, r, ap, S, stream)
            r.scale_add_ratio_into(p, p, 1.0, (S, 2), stream=stream)


def bench_matrix(name, csr, sym, iters):
    rp, ci, va, n = csr
    sx.options_reset()
    if sym:
        sx.option_set("spx.matrix.symmetric", "true")
    inp = sx.input_load_csr(rp, ci, va, n, n)
    A = sx.mat_tune(inp)
    cg = Cg(A, n)
    iters = -(-iters // GRAPH_ITERS) * GRAPH_ITERS
    cg.reset()
    cg.host_iters(3)                           # warm-up of every kernel used below
    cg.dev_iters(3)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cg.dev_iters(GRAPH_ITERS, torch.cuda.current_stream().cuda_stream)
    spmv = []
    forms = {"a": lambda: cg.host_iters(iters), "b": lambda: cg.dev_iters(iters),
             "c": lambda: [g.replay() for _ in range(iters // GRAPH_ITERS)]}
    ts = {k: [] for k in forms}
    for _ in range(BATCHES):
        for k, fn in forms.items():
            cg.reset()
            ts[k].append(timed(fn) / iters)
        spmv.append(timed(lambda: [sx.matvec_kernel_vec(A, 1.0, cg.p, 0.0, cg.ap) for _ in range(iters)]) / iters)
    rows = []
    for k, label in [("a", "(a) host scalars"), ("b", "(b) device scalars, stream"),
                     ("c", "(c) device scalars, graph of %d" % GRAPH_ITERS)]:
        med, lo, hi = stats(ts[k])
        rows.append("| %s%s | %d | %s | %.1f | %.1f .. %.1f | %.2f |" % (
            name, " (symmetric)" if sym else "", n, label, med * 1e6, lo * 1e6, hi * 1e6,
            stats(ts["a"])[0] / med))
    med, lo, hi = stats(spmv)
    rows.append("| %s%s | %d | the product alone | %.1f | %.1f .. %.1f | |" % (
        name, " (symmetric)" if sym else "", n, med * 1e6, lo * 1e6, hi * 1e6))
    return rows


def bench_update(n, reps):
    x, p, r, ap = (sx.DeviceVector(n) for _ in range(4))
    S = sx.DeviceVector(3)
    for v, val in ((x, 0.5), (p, 0.25), (r, 1.0), (ap, 0.125)):
        v.init(val)

    def three(k):
        for _ in range(k):
            x.scale_add_into(p, x, 1e-3)
            r.scale_add_into(ap, r, -1e-3)
            r.dot(r)

    def three_nosync(k):                       # ... with the dot product left on the device: the kernels alone
        for _ in range(k):
            x.scale_add_into(p, x, 1e-3)
            r.scale_add_into(ap, r, -1e-3)
            r.dot_into(r, S, 0)

    def fused(k):
        for _ in range(k):
            S.init(1e-3)                       # rr = pap: alpha = 1 (a tiny kernel, counted against the fused form)
            sx.cg_update(x, p, r, ap, S)

    forms = {"scale_add + scale_add + mul (host result)": (three, 7),
             "scale_add + scale_add + mul_dev": (three_nosync, 7),
             "cg_update": (fused, 6)}
    for fn, _ in forms.values():
        fn(3)
    ts = {k: [] for k in forms}
    for _ in range(BATCHES):
        for k, (fn, _) in forms.items():
            r.init(1.0)
            ts[k].append(timed(lambda: fn(reps)) / reps)
    rows = []
    for k, (_, passes) in forms.items():
        med, lo, hi = stats(ts[k])
        rows.append("| %d | %s | %d | %.1f | %.1f .. %.1f | %.2f |" % (
            n, k, passes, med * 1e6, lo * 1e6, hi * 1e6, passes * 8.0 * n / med / 1e12))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50, help="CG iterations per batch (at least 50 for a record)")
    ap.add_argument("--edge", type=int, default=120, help="grid edge of syn-nlpkkt")
    ap.add_argument("--scale", type=float, default=1.0, help="size factor of syn-cant")
    ap.add_argument("--n", type=int, default=27993600, help="vector length of the cg_update comparison")
    ap.add_argument("--symmetric", action="store_true", help="tune the matrices as symmetric ones")
    ap.add_argument("--skip-matrices", action="store_true")
    ap.add_argument("--skip-update", action="store_true")
    ap.add_argument("--out", default=None, help="also write the tables to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("cg_bench.py measures on the GPU; there is none")
    torch.cuda.set_device(0)
    out = ["| matrix | rows | form | us / iteration (median of %d batches x %d) | min .. max | (a) / this |" % (
        BATCHES, args.iters), "|---|---|---|---|---|---|"]
    if not args.skip_matrices:
        for name, gen in (("syn-cant", lambda: synth.syn_cant(args.scale)),
                          ("syn-nlpkkt edge %d" % args.edge, lambda: synth.syn_nlpkkt_rows(args.edge))):
            out += bench_matrix(name, gen(), args.symmetric, args.iters)
            print("\n".join(out[-4:]), flush=True)
    if not args.skip_update:
        out += ["", "| doubles | form | vector passes | us (median of %d batches x %d) | min .. max | TB/s |" % (
            BATCHES, args.iters), "|---|---|---|---|---|---|"]
        out += bench_update(args.n, args.iters)
    text = "\n".join(out)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
