#!/usr/bin/env python3
"""What new values for a tuned pattern cost (spx_hip_mat_values_plan + spx_hip_mat_set_values) against what a
client paid before: a new tune.  All in one process, one matrix after the other:

    python3 tools/refresh_bench.py [--edges 60,120,150] [--webbase] [--symmetric] [--out FILE]

Per matrix (syn-nlpkkt at every grid edge named, syn-webbase), one JSON line:
    set_values_us    spx_hip_mat_set_values from a value array in HBM: HIP events around single calls after three
                     warm-up calls, the median of seven
    copy_us          a device-to-device hipMemcpyAsync of value_bytes, timed the same way: the floor of any
                     rewrite of the values
    tune_s, emit_s   spx_hip_mat_info's tune_seconds and emit_seconds of the tune that made the matrix: what the
                     update replaces
    plan_s           spx_hip_mat_values_plan, wall clock (the host walk and the upload)
    product_us       one spx_hip_matvec_kernel, for scale
The update is gated: the product after it against the CSR arrays with the new values (relative 1e-6), and a
sample of spx_mat_get_entry.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (tune, make_workload, ALPHA)

WARM, CALLS = 3, 7


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--edges", default="60,120,%d" % bench.SAMPLE_EDGE, help="grid edges of syn-nlpkkt, in turn")
    ap.add_argument("--webbase", action="store_true", help="syn-webbase as well")
    ap.add_argument("--symmetric", action="store_true", help="symmetric tunes of syn-nlpkkt as well")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    import torch
    import scipy.sparse as sp
    from sparsex_amd import synth
    if not torch.cuda.is_available():
        sys.exit("refresh_bench.py needs a HIP device")
    torch.cuda.set_device(0)
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    D2D = 3                                   # hipMemcpyDeviceToDevice

    def note(msg):
        print("[refresh_bench] " + msg, file=sys.stderr, flush=True)

    def timed(fn):
        """median and spread of CALLS single calls, each between two HIP events, after WARM calls"""
        for _ in range(WARM):
            fn()
        torch.cuda.synchronize()
        t = []
        for _ in range(CALLS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            t.append(1e3 * e0.elapsed_time(e1))
        return float(np.median(t)), [round(min(t), 1), round(max(t), 1)]

    work = [("syn-nlpkkt", int(e), False) for e in args.edges.split(",") if e]
    if args.symmetric:
        work += [("syn-nlpkkt", int(e), True) for e in args.edges.split(",") if e]
    if args.webbase:
        work.append(("syn-webbase", None, False))
    status = 0
    for name, edge, sym in work:
        csr = synth.syn_nlpkkt_rows(edge) if edge else bench.make_workload(name, 1.0)
        rp, ci, va, n = csr
        nnz = int(rp[-1])
        note("%s%s%s: %d rows, %d nonzeros" % (name, " edge %d" % edge if edge else "", " symmetric" if sym else "", n, nnz))
        opts = {"spx.rt.nr_threads": args.threads, "spx.rt.device": 0, "spx.rt.keep_encoded": "false"}
        if sym:
            opts["spx.matrix.symmetric"] = "true"
        t0 = time.perf_counter()
        A = bench.tune(csr, opts)
        tune_wall = time.perf_counter() - t0
        inf = A.info()
        t0 = time.perf_counter()
        A.values_plan(rp, ci)
        plan_wall = time.perf_counter() - t0
        plan = A.values_plan_info()
        # new values: the old ones scaled entry by entry (symmetric input stays symmetric: the factor depends on
        # the unordered pair)
        r = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
        new = va * (1.0 + ((np.minimum(r, ci) * 31 + np.maximum(r, ci) * 17) % 1000) / 1000.0)
        del r
        src = torch.from_numpy(new).cuda()
        st = torch.cuda.current_stream().cuda_stream
        set_us, set_spread = timed(lambda: A.hip_set_values(src.data_ptr(), st))
        nval = int(inf.value_bytes) // 8
        a, b = torch.empty(nval, dtype=torch.float64, device="cuda"), torch.zeros(nval, dtype=torch.float64, device="cuda")
        copy_us, copy_spread = timed(lambda: hip.hipMemcpyAsync(a.data_ptr(), b.data_ptr(), nval * 8, D2D, st))
        del a, b
        x = torch.from_numpy(synth.random_x(n, seed=42)).cuda()
        y = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
        prod_us, _ = timed(lambda: A.hip_matvec_kernel(bench.ALPHA, x.data_ptr(), 0.0, y.data_ptr(), st))
        # the gate
        ref = bench.ALPHA * (sp.csr_matrix((new, ci, rp), shape=(n, n)) @ x.cpu().numpy())
        yh = y.cpu().numpy()
        parity = bool(np.isfinite(yh).all() and (np.abs(yh - ref) <= 1e-6 * np.abs(ref) + 1e-12 * np.abs(ref).max()).all())
        rng = np.random.RandomState(7)
        for k in rng.choice(nnz, 64, replace=False):
            row = int(np.searchsorted(rp, k, side="right") - 1)
            parity = parity and bool(A.get_entry(row, int(ci[k])) == new[k])
        moved = int(plan["n_dest"]) * 20
        out = {"matrix": name, "edge": edge, "symmetric": sym, "nrows": int(n), "nnz": nnz,
               "value_mb": round(int(inf.value_bytes) / 1e6, 1), "plan_mb": round(plan["plan_bytes"] / 1e6, 1),
               "n_dest": int(plan["n_dest"]), "n_sources": int(plan["n_sources"]),
               "set_values_us": round(set_us, 1), "set_values_us_spread": set_spread,
               "set_values_gb_per_s": round(moved / (set_us * 1e-6) / 1e9, 1),
               "copy_us": round(copy_us, 1), "copy_us_spread": copy_spread,
               "product_us": round(prod_us, 1),
               "tune_s": round(float(inf.tune_seconds), 3), "emit_s": round(float(inf.emit_seconds), 3),
               "tune_wall_s": round(tune_wall, 3), "plan_s": round(plan_wall, 3),
               "retune_over_update": round((float(inf.tune_seconds) + float(inf.emit_seconds)) / (set_us * 1e-6), 0),
               "parity": parity,
               "protocol": "%d warm-up calls, then %d single calls between HIP events, median; 20 B per destination "
                           "(4 plan + 8 gather + 8 store) for the rate" % (WARM, CALLS)}
        line = json.dumps(out)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
        status = status or (0 if parity else 1)
        A.destroy()
        del src, x, y, csr, rp, ci, va, new
        torch.cuda.empty_cache()
    return status


if __name__ == "__main__":
    sys.exit(main())
