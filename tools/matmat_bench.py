#!/usr/bin/env python3
"""The multi-vector product against k single-vector products (bench.py's protocol: the synth generators,
random_x seeds, alpha = 0.5, a warm-up call, hipEvent timing, the median of 5 outer loops).

For every config and k = 1, 2, 4, 8: one spx_hip_matmat_kernel over a (k, n) block against k back-to-back
spx_hip_matvec_kernel calls on the same columns; every column of the block product is gated on the single
products (relative 1e-6, the reference's criterion).  One JSON line per config:

    python3 tools/matmat_bench.py [--configs cant,nd24k,webbase,e240,nd24k-sym,e240-sym,nd24k-sym-mv,e240-sym-mv] [--edge 240]

The configs of one run share a process, so their times compare (A/B inside one process: separate processes differ
by up to 15 % on syn-nlpkkt).
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

KS = (1, 2, 4, 8)

# name -> (workload, symmetric path, extra options)
CONFIGS = {
    "cant": ("syn-cant", False, {}),
    "nd24k": ("syn-nd24k", False, {}),
    "webbase": ("syn-webbase", False, {}),
    "e240": ("syn-nlpkkt", False, {}),
    "nd24k-sym": ("syn-nd24k", True, {}),
    "e240-sym": ("syn-nlpkkt", True, {}),
    # the symmetric tune with spx.gpu.sym_matmat: its read-once passes serve groups of vectors
    "nd24k-sym-mv": ("syn-nd24k", True, {"spx.gpu.sym_matmat": "true"}),
    "e240-sym-mv": ("syn-nlpkkt", True, {"spx.gpu.sym_matmat": "true"}),
}


def workload(name, edge):
    from sparsex_amd import synth
    if name == "syn-nlpkkt":
        return synth.syn_nlpkkt_rows(edge)
    return bench.make_workload(name, 1.0)


def time_call(torch, fn, reps):
    """Median over BATCHES outer loops of the hipEvent time per call (reps calls per loop)."""
    fn()
    torch.cuda.synchronize()
    per = []
    for _ in range(bench.BATCHES):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        per.append(1e-3 * e0.elapsed_time(e1) / reps)
    return float(np.median(per))


def run(torch, cfg, edge, threads):
    from sparsex_amd import synth
    wl, sym, extra = CONFIGS[cfg]
    csr = workload(wl, edge)
    rp, ci, va, n = csr
    nnz = int(rp[-1])
    opts = {"spx.rt.nr_threads": threads, "spx.rt.device": torch.cuda.current_device(),
            "spx.matrix.symmetric": "true" if sym else "false", "spx.rt.keep_encoded": "false"}
    opts.update(extra)
    t0 = time.perf_counter()
    A = bench.tune(csr, opts)
    tune_s = time.perf_counter() - t0
    del csr, rp, ci, va
    dev = torch.device("cuda", torch.cuda.current_device())
    kmax = max(KS)
    X = torch.stack([torch.from_numpy(synth.random_x(n, seed=42 + j)) for j in range(kmax)]).to(dev)
    Y = torch.full((kmax, n), float("nan"), dtype=torch.float64, device=dev)
    Y1 = torch.full((kmax, n), float("nan"), dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    t_one = None
    rows = {}
    parity = True
    for k in KS:
        Xk, Yk, Y1k = X[:k], Y[:k], Y1[:k]

        def block():
            A.hip_matmat_kernel(bench.ALPHA, Xk.data_ptr(), n, k, 0.0, Yk.data_ptr(), n, stream)

        def singles():
            for j in range(k):
                A.hip_matvec_kernel(bench.ALPHA, Xk[j].data_ptr(), 0.0, Y1k[j].data_ptr(), stream)
        block()
        singles()
        torch.cuda.synchronize()
        err = (Yk - Y1k).abs()
        ok = bool(torch.isfinite(Yk).all()) and bool((err <= 1e-6 * Y1k.abs() + 1e-300).all())
        parity &= ok
        # (a few milliseconds of work per outer loop, at least one call)
        t_est = time_call(torch, singles, 1)
        reps = int(min(max(0.02 / max(t_est, 1e-7), 1), 200))
        t_mm = time_call(torch, block, reps)
        t_mv = time_call(torch, singles, reps)
        if k == 1:
            t_one = t_mv
        rows[str(k)] = {"us_per_call": round(1e6 * t_mm, 2), "us_per_vector": round(1e6 * t_mm / k, 2),
                        "us_k_single": round(1e6 * t_mv, 2), "ratio_vs_k_single": round(t_mm / t_mv, 3),
                        "gflops": round(2.0 * nnz * k / t_mm / 1e9, 1),
                        "gflops_k_single": round(2.0 * nnz * k / t_mv / 1e9, 1),
                        "max_rel_err_vs_single": float((err / Y1k.abs().clamp_min(1e-300)).max()), "parity": ok}
    info = A.info()
    out = {"config": cfg, "workload": wl, "edge": edge if wl == "syn-nlpkkt" else None, "symmetric_path": sym,
           "nrows": n, "nnz": nnz, "matmat_group": A.matmat_group(), "waves": int(info.waves),
           "sym_tiles": int(info.sym_tiles), "sym_segments": int(info.sym_segments), "col_slices": int(info.col_slices),
           "wave_tiles": int(info.wave_tiles), "unit_windows": int(info.unit_windows),
           "us_single": round(1e6 * t_one, 2), "k": rows, "parity": parity, "tune_seconds": round(tune_s, 2),
           "protocol": "alpha=%g beta=0, warm-up call, hipEvent time, median of %d outer loops; GFLOP/s = 2*nnz*k/t"
                       % (bench.ALPHA, bench.BATCHES)}
    A.destroy()
    del A, X, Y, Y1
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--edge", type=int, default=bench.DEFAULT_EDGE)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    import torch
    torch.cuda.set_device(0)
    ok = True
    for cfg in args.configs.split(","):
        line = json.dumps(run(torch, cfg, args.edge, args.threads))
        print(line, flush=True)
        ok &= json.loads(line)["parity"]
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
