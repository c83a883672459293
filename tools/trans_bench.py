#!/usr/bin/env python3
"""The transposed product y <- alpha*A^T*x against the forward product and against the alternative a client had
before it: the forward product of a separately tuned A^T.  One matrix per process:

    python3 tools/trans_bench.py --matrix nlpkkt [--edge 150] | --matrix cant | --matrix webbase  [--out FILE]

Variants, timed with HIP events on one stream after a warm-up call, alternating inside every one of the 5
batches (bench.py's BATCHES; the median per variant is reported):
    forward      spx_hip_matvec_kernel on A
    trans-1      spx_hip_matvec_trans_kernel, spx.gpu.trans_windows=false: one atomic add per nonzero
    trans-2      ... =true: unit windows accumulate in LDS, each goes to y once
    forward-At   spx_hip_matvec_kernel on a tune of A^T (a second matrix in HBM, a second tune)
trans-1 and trans-2 need a handle each (the option is read at tune time).  Per transposed variant the flushed
atomic bytes per second: nnz * 8, or (staged doubles + nonzeros outside the windows) * 8, over its time.  The
three transposed results are gated on each other (relative 1e-6, the reference's criterion).  One JSON line.
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

MATRICES = {"nlpkkt": "syn-nlpkkt", "cant": "syn-cant", "webbase": "syn-webbase"}


def workload(name, edge):
    from sparsex_amd import synth
    if name == "nlpkkt":
        return synth.syn_nlpkkt_rows(edge)
    return bench.make_workload(MATRICES[name], 1.0)


def transpose(csr):
    import scipy.sparse as sp
    rp, ci, va, n = csr
    t = sp.csr_matrix((va, ci, rp), shape=(n, n)).T.tocsr()
    t.sort_indices()
    return t.indptr.astype(np.int32), t.indices.astype(np.int32), t.data, n


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--matrix", choices=list(MATRICES), required=True)
    ap.add_argument("--edge", type=int, default=bench.SAMPLE_EDGE, help="grid edge of syn-nlpkkt")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=None, help="also append the JSON line to this file")
    args = ap.parse_args()
    import torch
    from sparsex_amd import synth
    if not torch.cuda.is_available():
        sys.exit("trans_bench.py needs a HIP device")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)

    def note(msg):
        print("[trans_bench] " + msg, file=sys.stderr, flush=True)
    csr = workload(args.matrix, args.edge)
    n, nnz = csr[3], int(csr[0][-1])
    note("%s: %d rows, %d nonzeros" % (MATRICES[args.matrix], n, nnz))
    base = {"spx.rt.nr_threads": args.threads, "spx.rt.device": 0, "spx.rt.keep_encoded": "false"}
    tunes = {}

    def tuned(name, c, extra):
        t0 = time.perf_counter()
        A = bench.tune(c, dict(base, **extra))
        tunes[name] = round(time.perf_counter() - t0, 2)
        note("tuned %s in %.1f s" % (name, tunes[name]))
        return A
    A1 = tuned("A trans_windows=false", csr, {"spx.gpu.trans_windows": "false"})
    A2 = tuned("A trans_windows=true", csr, {"spx.gpu.trans_windows": "true"})
    csr_t = transpose(csr)
    del csr
    note("transposed on the host")
    At = tuned("A^T", csr_t, {})
    del csr_t
    x = torch.from_numpy(synth.random_x(n, seed=42)).to(dev)
    ys = {k: torch.full((n,), float("nan"), dtype=torch.float64, device=dev) for k in ("forward", "trans-1", "trans-2", "forward-At")}
    st = torch.cuda.current_stream().cuda_stream
    calls = {
        "forward": lambda: A1.hip_matvec_kernel(bench.ALPHA, x.data_ptr(), 0.0, ys["forward"].data_ptr(), st),
        "trans-1": lambda: A1.hip_matvec_trans_kernel(bench.ALPHA, x.data_ptr(), 0.0, ys["trans-1"].data_ptr(), st),
        "trans-2": lambda: A2.hip_matvec_trans_kernel(bench.ALPHA, x.data_ptr(), 0.0, ys["trans-2"].data_ptr(), st),
        "forward-At": lambda: At.hip_matvec_kernel(bench.ALPHA, x.data_ptr(), 0.0, ys["forward-At"].data_ptr(), st),
    }
    for fn in calls.values():          # warm-up
        fn()
    torch.cuda.synchronize()
    ref = ys["forward-At"]
    tol = 1e-6 * ref.abs() + 1e-12 * ref.abs().max()
    parity = all(bool(torch.isfinite(ys[k]).all()) and bool(((ys[k] - ref).abs() <= tol).all()) for k in ("trans-1", "trans-2"))

    def once(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return 1e-3 * e0.elapsed_time(e1) / reps
    reps = {k: int(min(max(0.05 / max(once(fn, 1), 1e-7), 1), 500)) for k, fn in calls.items()}
    per = {k: [] for k in calls}
    for _ in range(bench.BATCHES):
        for k, fn in calls.items():    # (alternating: every batch times every variant)
            per[k].append(once(fn, reps[k]))
    t = {k: float(np.median(v)) for k, v in per.items()}
    i1, i2 = A1.info(), A2.info()
    bytes_1 = 8 * nnz
    bytes_2 = 8 * (int(i2.unit_window_staged) + int(i2.nnz_stored) - int(i2.unit_window_elems)) if A2.trans_mode() == 2 else bytes_1
    out = {"matrix": MATRICES[args.matrix], "edge": args.edge if args.matrix == "nlpkkt" else None, "nrows": n, "nnz": nnz,
           "value_mb": round(int(i1.value_bytes) / 1e6, 1), "waves": int(i1.waves),
           "forward_unit_windows": int(i1.unit_windows), "modes": {"trans-1": A1.trans_mode(), "trans-2": A2.trans_mode()},
           "window_nonzeros": int(i2.unit_window_elems), "staged_doubles": int(i2.unit_window_staged),
           "us": {k: round(1e6 * v, 2) for k, v in t.items()},
           "us_spread": {k: [round(1e6 * min(v), 2), round(1e6 * max(v), 2)] for k, v in per.items()},
           "ratio_to_forward": {k: round(t[k] / t["forward"], 3) for k in t},
           "atomic_gb_per_s": {"trans-1": round(bytes_1 / t["trans-1"] / 1e9, 1), "trans-2": round(bytes_2 / t["trans-2"] / 1e9, 1)},
           "atomic_mb": {"trans-1": round(bytes_1 / 1e6, 2), "trans-2": round(bytes_2 / 1e6, 2)},
           "parity": parity, "tune_seconds": tunes,
           "protocol": "alpha=%g beta=0, warm-up call, hipEvent time per batch of calls, median of %d batches, variants "
                       "alternating inside every batch" % (bench.ALPHA, bench.BATCHES)}
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")
    return 0 if parity else 1


if __name__ == "__main__":
    sys.exit(main())
