#!/usr/bin/env python3
"""The row-major (interleaved) multi-vector product against its two yardsticks, in ONE process on ONE handle:

  (a) spx_hip_matmat_rm_kernel on an (n, k) row-major block,
  (b) spx_hip_matmat_kernel on the (k, n) column-major block of the same numbers,
  (c) k back-to-back spx_hip_matvec_kernel calls on its columns,

for k = 1, 2, 4, 8 on general tunes (bench.py's protocol: the synth generators, random_x seeds, alpha = 0.5,
beta = 0, warm-up calls, hipEvent timing).  The three are timed in ALTERNATING batches -- a, b, c, a, b, c, ...,
five rounds -- so that a drift of the clock or the machine lands on all of them alike; the median of the five and
their spread ((max - min) / median) are reported.  Every column of (a) and of (b) is gated on (c) before anything
is timed (relative 1e-6, the reference's criterion).  One JSON line per config:

    python3 tools/matmat_rm_bench.py [--configs cant,nd24k,webbase,e240] [--edge 240]

--f32: spx_hip_matmat_rm_kernel_f32 (the float copy of the values, spx.gpu.values_f32=true) against
spx_hip_matmat_rm_kernel on one handle, at the handle's group (or --k), with the variants, gates and protocol of
tools/matmat_bench.py --f32 (whose code runs), itself that of tools/f32_bench.py.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (make_workload, tune, ALPHA, BATCHES: the bench protocol)
import matmat_bench  # noqa: E402  (run_f32: the --f32 variant of both tools)

KS = (1, 2, 4, 8)

# name -> workload (all tuned as general matrices: the row-major product refuses symmetric handles)
CONFIGS = {
    "cant": "syn-cant",
    "nd24k": "syn-nd24k",
    "webbase": "syn-webbase",
    "e240": "syn-nlpkkt",
}


def workload(name, edge):
    from sparsex_amd import synth
    if name == "syn-nlpkkt":
        return synth.syn_nlpkkt_rows(edge)
    return bench.make_workload(name, 1.0)


def batch(torch, fn, reps):
    """hipEvent seconds per call of one batch of `reps` calls."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return 1e-3 * e0.elapsed_time(e1) / reps


def alternate(torch, fns, reps, rounds):
    """name -> (median, spread) over `rounds` batches of each function, the batches taken in turn."""
    per = {name: [] for name in fns}
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for name, fn in fns.items():
            per[name].append(batch(torch, fn, reps))
    out = {}
    for name, t in per.items():
        med = float(np.median(t))
        out[name] = (med, (max(t) - min(t)) / med)
    return out


def run(torch, cfg, edge, threads):
    from sparsex_amd import synth
    wl = CONFIGS[cfg]
    csr = workload(wl, edge)
    n, nnz = csr[3], int(csr[0][-1])
    opts = {"spx.rt.nr_threads": threads, "spx.rt.device": torch.cuda.current_device(),
            "spx.matrix.symmetric": "false", "spx.rt.keep_encoded": "false"}
    t0 = time.perf_counter()
    A = bench.tune(csr, opts)
    tune_s = time.perf_counter() - t0
    del csr
    dev = torch.device("cuda", torch.cuda.current_device())
    kmax = max(KS)
    X = torch.stack([torch.from_numpy(synth.random_x(n, seed=42 + j)) for j in range(kmax)]).to(dev)
    stream = torch.cuda.current_stream().cuda_stream
    rows, parity = {}, True
    for k in KS:
        Xc = X[:k].contiguous()                                    # (k, n): column-major block
        Xr = Xc.t().contiguous()                                   # (n, k): the same numbers, interleaved
        Yr = torch.full((n, k), float("nan"), dtype=torch.float64, device=dev)
        Yc = torch.full((k, n), float("nan"), dtype=torch.float64, device=dev)
        Y1 = torch.full((k, n), float("nan"), dtype=torch.float64, device=dev)

        def rm():
            A.hip_matmat_rm_kernel(bench.ALPHA, Xr.data_ptr(), k, k, 0.0, Yr.data_ptr(), k, stream)

        def cm():
            A.hip_matmat_kernel(bench.ALPHA, Xc.data_ptr(), n, k, 0.0, Yc.data_ptr(), n, stream)

        def singles():
            for j in range(k):
                A.hip_matvec_kernel(bench.ALPHA, Xc[j].data_ptr(), 0.0, Y1[j].data_ptr(), stream)
        rm()
        cm()
        singles()
        torch.cuda.synchronize()
        bound = 1e-6 * Y1.abs() + 1e-300
        err_rm, err_cm = (Yr.t() - Y1).abs(), (Yc - Y1).abs()
        ok = bool(torch.isfinite(Yr).all()) and bool((err_rm <= bound).all()) and \
            bool(torch.isfinite(Yc).all()) and bool((err_cm <= bound).all())
        parity &= ok
        # (a few milliseconds of work per batch, at least one call)
        t_est = batch(torch, singles, 1)
        reps = int(min(max(0.02 / max(t_est, 1e-7), 1), 200))
        t = alternate(torch, {"rm": rm, "cm": cm, "singles": singles}, reps, bench.BATCHES)
        rows[str(k)] = {
            "us_rm": round(1e6 * t["rm"][0], 2), "us_cm": round(1e6 * t["cm"][0], 2),
            "us_k_single": round(1e6 * t["singles"][0], 2),
            "spread_rm": round(t["rm"][1], 3), "spread_cm": round(t["cm"][1], 3),
            "spread_k_single": round(t["singles"][1], 3),
            "us_per_vector_rm": round(1e6 * t["rm"][0] / k, 2), "us_per_vector_cm": round(1e6 * t["cm"][0] / k, 2),
            "rm_vs_cm": round(t["rm"][0] / t["cm"][0], 3), "rm_vs_k_single": round(t["rm"][0] / t["singles"][0], 3),
            "cm_vs_k_single": round(t["cm"][0] / t["singles"][0], 3),
            "gflops_rm": round(2.0 * nnz * k / t["rm"][0] / 1e9, 1), "reps": reps,
            "max_rel_err_rm_vs_single": float((err_rm / Y1.abs().clamp_min(1e-300)).max()), "parity": ok}
        del Xc, Xr, Yr, Yc, Y1
    info = A.info()
    out = {"config": cfg, "workload": wl, "edge": edge if wl == "syn-nlpkkt" else None, "nrows": n, "nnz": nnz,
           "matmat_rm_group": A.matmat_rm_group(), "matmat_group": A.matmat_group(), "waves": int(info.waves),
           "col_slices": int(info.col_slices), "wave_tiles": int(info.wave_tiles), "k": rows, "parity": parity,
           "tune_seconds": round(tune_s, 2),
           "protocol": "alpha=%g beta=0, warm-up calls, hipEvent time, alternating batches rm/cm/singles, median of %d "
                       "and (max - min) / median; GFLOP/s = 2*nnz*k/t" % (bench.ALPHA, bench.BATCHES)}
    A.destroy()
    del A, X
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--edge", type=int, default=bench.DEFAULT_EDGE)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--f32", action="store_true",
                    help="the float row-major block product against the fp64 one on one handle (see above)")
    ap.add_argument("--no-plain", action="store_true", help="--f32: no second handle tuned without the copy")
    ap.add_argument("--first", choices=["without", "with"], default="without",
                    help="--f32: which handle is tuned first and whose fp64 block is timed first in every round")
    ap.add_argument("--k", default=None, help="--f32: comma-separated block widths instead of the handle's group")
    args = ap.parse_args()
    import torch
    torch.cuda.set_device(0)
    ok = True
    for cfg in args.configs.split(","):
        if args.f32:
            ks = tuple(int(k) for k in args.k.split(",")) if args.k else None
            line = json.dumps(matmat_bench.run_f32(torch, cfg, CONFIGS[cfg], False, {}, args.edge, args.threads, "rm", ks,
                                                   not args.no_plain, args.first))
        else:
            line = json.dumps(run(torch, cfg, args.edge, args.threads))
        print(line, flush=True)
        ok &= json.loads(line)["parity"]
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
