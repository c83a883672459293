#!/usr/bin/env python3
"""The product with the float copy of the values (spx.gpu.values_f32, spx_hip_matvec_kernel_f32) against the fp64
product in the same process.  One matrix per process:

    python3 tools/f32_bench.py --matrix nlpkkt [--edge 150] | --matrix cant | --matrix webbase  [--out FILE]
    python3 tools/f32_bench.py --symmetric --matrix nlpkkt [--edge 150] | --matrix nd24k | --matrix cant  [--out FILE]

--symmetric tunes the matrix as a symmetric one (spx.matrix.symmetric=true) and asks for the copy with
spx.gpu.values_f32=all ("true" where it is not given); the bytes are then those of the stored triangle and the diagonal.

Variants, timed with HIP events on one stream after a warm-up call, alternating inside every one of the 5 batches
(bench.py's BATCHES; about 50 ms of work per batch and variant; the median per variant is reported):
    f64-plain    spx_hip_matvec_kernel on a handle tuned WITHOUT the option
    f64          spx_hip_matvec_kernel on a handle tuned WITH it (the same unchanged kernel: must agree with f64-plain
                 within the batches' spread, unless the launch tuner settled the two handles differently -- the
                 launch forms of both are in the line)
    f32          spx_hip_matvec_kernel_f32 on that handle
Timed once each: the kernel that builds the copy (csx_narrow_values_kernel), and spx_hip_mat_set_values on both
handles (one gather pass over the values; with the copy it writes both arrays).
Gates: f64 against the CSR product of the values, f32 against the CSR product of the values rounded to float, both
relative 1e-6 (the reference's criterion).  Algorithmic bytes per product as bench.py counts them (every stored
value once, x once, y once) for 8- and 4-byte values, and what fraction of 8 TB/s each product reaches with them.
One JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (make_workload, tune, ALPHA, BATCHES, HBM_PEAK_GBS: the bench protocol)

MATRICES = {"nlpkkt": "syn-nlpkkt", "cant": "syn-cant", "webbase": "syn-webbase", "nd24k": "syn-nd24k"}


def workload(name, edge):
    from sparsex_amd import synth
    if name == "nlpkkt":
        return synth.syn_nlpkkt_rows(edge)
    return bench.make_workload(MATRICES[name], 1.0)


def csr_product(csr, values, x):
    import scipy.sparse as sp
    rp, ci, _, n = csr
    return sp.csr_matrix((values, ci, rp), shape=(n, n)) @ x


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--matrix", choices=list(MATRICES), required=True)
    ap.add_argument("--edge", type=int, default=bench.SAMPLE_EDGE, help="grid edge of syn-nlpkkt")
    ap.add_argument("--symmetric", action="store_true",
                    help="tune as a symmetric matrix, the copy asked for with spx.gpu.values_f32=all")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--first", choices=["without", "with"], default="without",
                    help="which handle is tuned first and whose fp64 product is timed first in every batch (the two run "
                         "the same kernel: a difference that follows the order is the order's, not the option's)")
    ap.add_argument("--out", default=None, help="also append the JSON line to this file")
    args = ap.parse_args()
    import torch
    import sparsex_amd as sx
    from sparsex_amd import synth
    if not torch.cuda.is_available():
        sys.exit("f32_bench.py needs a HIP device")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)

    def note(msg):
        print("[f32_bench] " + msg, file=sys.stderr, flush=True)
    csr = workload(args.matrix, args.edge)
    n, nnz = csr[3], int(csr[0][-1])
    note("%s: %d rows, %d nonzeros" % (MATRICES[args.matrix], n, nnz))
    base = {"spx.rt.nr_threads": args.threads, "spx.rt.device": 0, "spx.rt.keep_encoded": "false"}
    if args.symmetric:
        base["spx.matrix.symmetric"] = "true"
    on = "all" if args.symmetric else "true"
    tunes = {}

    def tuned(name, extra):
        t0 = time.perf_counter()
        A = bench.tune(csr, dict(base, **extra))
        tunes[name] = round(time.perf_counter() - t0, 2)
        note("tuned %s in %.1f s" % (name, tunes[name]))
        return A
    if args.first == "without":
        A0 = tuned("values_f32=false", {"spx.gpu.values_f32": "false"})
        A1 = tuned("values_f32=" + on, {"spx.gpu.values_f32": on})
    else:
        A1 = tuned("values_f32=" + on, {"spx.gpu.values_f32": on})
        A0 = tuned("values_f32=false", {"spx.gpu.values_f32": "false"})
    assert bool(A0.info().symmetric) == bool(A1.info().symmetric) == args.symmetric
    assert A0.values_f32_bytes() == 0 and A1.values_f32_bytes() > 0
    xh = synth.random_x(n, seed=42)
    x = torch.from_numpy(xh).to(dev)
    ys = {k: torch.full((n,), float("nan"), dtype=torch.float64, device=dev) for k in ("f64-plain", "f64", "f32")}
    st = torch.cuda.current_stream().cuda_stream
    calls = {
        "f64-plain": lambda: A0.hip_matvec_kernel(bench.ALPHA, x.data_ptr(), 0.0, ys["f64-plain"].data_ptr(), st),
        "f64": lambda: A1.hip_matvec_kernel(bench.ALPHA, x.data_ptr(), 0.0, ys["f64"].data_ptr(), st),
        "f32": lambda: A1.hip_matvec_kernel_f32(bench.ALPHA, x.data_ptr(), 0.0, ys["f32"].data_ptr(), st),
    }
    if args.first == "with":
        calls = {k: calls[k] for k in ("f64", "f64-plain", "f32")}
    for fn in calls.values():          # warm-up
        fn()
    torch.cuda.synchronize()

    def gate(y, values):
        ref = torch.from_numpy(bench.ALPHA * csr_product(csr, values, xh)).to(dev)
        tol = 1e-6 * ref.abs() + 1e-12 * ref.abs().max()
        return bool(torch.isfinite(y).all()) and bool(((y - ref).abs() <= tol).all())
    v32 = csr[2].astype(np.float32).astype(np.float64)
    parity = {"f64-plain": gate(ys["f64-plain"], csr[2]), "f64": gate(ys["f64"], csr[2]), "f32": gate(ys["f32"], v32)}
    # (and the float product is not the fp64 one: the two differ by about 2^-24 of the row sums)
    differs = float((ys["f32"] - ys["f64"]).abs().max()) > 0.0
    del v32

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

    # once each: the narrowing kernel, and the value refresh with and without the copy
    narrow_s = float(sx.lib().spx_hip_mat_values_f32_narrow_seconds(A1.handle))
    src = torch.from_numpy(np.array(csr[2], dtype=np.float64)).to(dev)
    set_values = {}
    for name, A in (("without", A0), ("with", A1)):
        A.values_plan(csr[0], csr[1])
        A.hip_set_values(src.data_ptr(), st)       # warm-up (the same values again)
        torch.cuda.synchronize()
        set_values[name] = once(lambda: A.hip_set_values(src.data_ptr(), st), 1)
    # (the refreshed arrays still multiply right)
    calls["f32"]()
    torch.cuda.synchronize()
    parity["f32 after set_values"] = gate(ys["f32"], csr[2].astype(np.float32).astype(np.float64))

    i0, i1 = A0.info(), A1.info()

    def form(i):
        return {"waves": int(i.waves), "unit_windows": int(i.unit_windows), "wave_tiles": int(i.wave_tiles),
                "col_slices": int(i.col_slices), "rowblocks": int(i.n_rowblocks), "sym_tiles": int(i.sym_tiles),
                "sym_segments": int(i.sym_segments), "sym_pipeline": int(i.sym_pipeline)}
    # (symmetric: the strictly lower values and the diagonal are stored; the float product reads the former as
    # floats, the diagonal stays an array of doubles)
    lower = (nnz - n) // 2
    bytes_64 = bench.algorithmic_bytes(args.symmetric, nnz, n, n, lower)
    bytes_32 = bytes_64 - 4.0 * (lower if args.symmetric else nnz)
    spread = {k: [round(1e6 * min(v), 2), round(1e6 * max(v), 2)] for k, v in per.items()}
    out = {"matrix": MATRICES[args.matrix], "symmetric": bool(args.symmetric), "edge": args.edge if args.matrix == "nlpkkt" else None, "nrows": n, "nnz": nnz,
           "value_mb": round(int(i1.value_bytes) / 1e6, 1), "values_f32_mb": round(A1.values_f32_bytes() / 1e6, 1),
           "launch_form": {"f64-plain": form(i0), "f64": form(i1)}, "order": list(calls),
           "us": {k: round(1e6 * v, 2) for k, v in t.items()}, "us_spread": spread,
           "ratio_f32_to_f64": round(t["f32"] / t["f64"], 3),
           "ratio_f64_to_f64_plain": round(t["f64"] / t["f64-plain"], 3),
           "algorithmic_mb": {"f64": round(bytes_64 / 1e6, 1), "f32": round(bytes_32 / 1e6, 1)},
           "fraction_of_hbm_peak": {"f64": round(bytes_64 / t["f64"] / 1e9 / bench.HBM_PEAK_GBS, 3),
                                    "f32": round(bytes_32 / t["f32"] / 1e9 / bench.HBM_PEAK_GBS, 3)},
           "narrow_kernel_us": round(1e6 * narrow_s, 1),
           "narrow_gb_per_s": round(12.0 * int(i1.value_bytes) / 8 / max(narrow_s, 1e-9) / 1e9, 1),
           "set_values_us": {k: round(1e6 * v, 1) for k, v in set_values.items()},
           "parity": parity, "f32_differs_from_f64": differs, "tune_seconds": tunes,
           "protocol": "alpha=%g beta=0, warm-up call, hipEvent time per batch of calls, median of %d batches, variants "
                       "alternating inside every batch; narrowing kernel and set_values: one timed call each after a "
                       "warm-up" % (bench.ALPHA, bench.BATCHES)}
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")
    return 0 if all(parity.values()) and differs else 1


if __name__ == "__main__":
    sys.exit(main())
