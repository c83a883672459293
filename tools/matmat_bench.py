#!/usr/bin/env python3
"""The multi-vector product against k single-vector products (bench.py's protocol: the synth generators,
random_x seeds, alpha = 0.5, a warm-up call, hipEvent timing, the median of 5 outer loops).

For every config and k = 1, 2, 4, 8: one spx_hip_matmat_kernel over a (k, n) block against k back-to-back
spx_hip_matvec_kernel calls on the same columns; every column of the block product is gated on the single
products (relative 1e-6, the reference's criterion).  One JSON line per config:

    python3 tools/matmat_bench.py [--configs cant,nd24k,webbase,e240,nd24k-sym,e240-sym,nd24k-sym-mv,e240-sym-mv] [--edge 240]

The configs of one run share a process, so their times compare (A/B inside one process: separate processes differ
by up to 15 % on syn-nlpkkt).

--f32: the block product with the float copy of the values (spx.gpu.values_f32, spx_hip_matmat_kernel_f32) against
the fp64 block product, with the protocol of tools/f32_bench.py: per config one handle tuned WITH the copy and
(unless --no-plain) one WITHOUT, in one process; for k = 2, 4, 8 the variants
    f64-plain    spx_hip_matmat_kernel on the handle without the copy
    f64          spx_hip_matmat_kernel on the handle with it (the same unchanged kernel: must agree with f64-plain
                 within the batches' spread, unless the launch tuner settled the two handles differently)
    f32          spx_hip_matmat_kernel_f32 on that handle
    f64-single   k back-to-back spx_hip_matvec_kernel calls on it
    f32-single   k back-to-back spx_hip_matvec_kernel_f32 calls on it
timed with HIP events in alternating batches, five rounds; the median and the spread (max - min) / median of each.
--first with: the handle with the copy is tuned first and its fp64 block timed in front of the plain handle's.
Gates, before anything is timed: every column of the float block product against the CSR product of the values
rounded to float, relative 1e-6 (f32_bench.py's gate); the fp64 block products against the single fp64 products.
Symmetric configs ask for the copy with spx.gpu.values_f32=all.  (tools/matmat_rm_bench.py --f32: the same for
row-major blocks, at the handle's group.)
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


def alternate(torch, fns, reps, rounds):
    """name -> (median, (max - min) / median) over `rounds` batches of each function, the batches taken in turn."""
    per = {name: [] for name in fns}
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for name, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            e1.synchronize()
            per[name].append(1e-3 * e0.elapsed_time(e1) / reps)
    return {name: (float(np.median(t)), (max(t) - min(t)) / float(np.median(t))) for name, t in per.items()}


def run_f32(torch, cfg, workload_name, sym, extra, edge, threads, layout="cm", ks=None, plain=True, first="without"):
    """The --f32 variant (see the module's docstring) for one config.  layout "cm": column-major blocks, k in `ks`
    (default 2, 4, 8); "rm": row-major blocks with ldx == ldy == k, k the handle's group unless `ks` is given."""
    import scipy.sparse as sp
    from sparsex_amd import synth
    csr = workload(workload_name, edge)
    rp, ci, va, n = csr
    nnz = int(rp[-1])
    base = {"spx.rt.nr_threads": threads, "spx.rt.device": torch.cuda.current_device(),
            "spx.matrix.symmetric": "true" if sym else "false", "spx.rt.keep_encoded": "false"}
    base.update(extra)
    on = "all" if sym else "true"
    tunes = {}

    def note(msg):
        print("[matmat_bench --f32] %s: %s" % (cfg, msg), file=sys.stderr, flush=True)
    note("%s, %d rows, %d nonzeros" % (workload_name, n, nnz))

    def tuned(name, value):
        t0 = time.perf_counter()
        A = bench.tune(csr, dict(base, **{"spx.gpu.values_f32": value}))
        tunes[name] = round(time.perf_counter() - t0, 2)
        note("tuned with %s in %.1f s" % (name, tunes[name]))
        return A
    # `first`: which handle is tuned first and whose fp64 block is timed first in every round (the two run the same
    # kernel: a difference that follows the order is the order's, not the option's)
    A0 = tuned("values_f32=false", "false") if plain and first == "without" else None
    A1 = tuned("values_f32=" + on, on)
    if plain and first != "without":
        A0 = tuned("values_f32=false", "false")
    assert A1.values_f32_bytes() > 0 and (A0 is None or A0.values_f32_bytes() == 0)
    group = A1.matmat_group_f32() if layout == "cm" else A1.matmat_rm_group()
    if ks is None:
        ks = (2, 4, 8) if layout == "cm" else (group,)
    kmax = max(ks)
    dev = torch.device("cuda", torch.cuda.current_device())
    Xh = np.stack([synth.random_x(n, seed=42 + j) for j in range(kmax)])
    # the gate's reference: the CSR product of the values rounded to float, all columns at once
    m32 = sp.csr_matrix((va.astype(np.float32).astype(np.float64), ci, rp), shape=(n, n))
    ref32 = torch.from_numpy(np.ascontiguousarray((bench.ALPHA * (m32 @ Xh.T)).T)).to(dev)      # (kmax, n)
    del m32
    note("reference products of %d columns done" % kmax)
    X = torch.from_numpy(Xh).to(dev)
    del Xh, csr, rp, ci, va
    stream = torch.cuda.current_stream().cuda_stream
    rows, parity = {}, True
    for k in ks:
        rm = layout == "rm"
        Xc = X[:k].contiguous()
        Xb = Xc.t().contiguous() if rm else Xc
        shape = (n, k) if rm else (k, n)
        Y = {v: torch.full(shape, float("nan"), dtype=torch.float64, device=dev) for v in ("f64-plain", "f64", "f32")}
        Y1 = {v: torch.full((k, n), float("nan"), dtype=torch.float64, device=dev) for v in ("f64-single", "f32-single")}
        ld = k if rm else n

        def block(A, name, yname):
            fn = getattr(A, name)
            y = Y[yname]
            return lambda: fn(bench.ALPHA, Xb.data_ptr(), ld, k, 0.0, y.data_ptr(), ld, stream)

        def singles(name, yname):
            fn = getattr(A1, name)
            y = Y1[yname]

            def run_them():
                for j in range(k):
                    fn(bench.ALPHA, Xc[j].data_ptr(), 0.0, y[j].data_ptr(), stream)
            return run_them
        f64_name = "hip_matmat_rm_kernel" if rm else "hip_matmat_kernel"
        fns = {}
        if A0 is not None and first == "without":
            fns["f64-plain"] = block(A0, f64_name, "f64-plain")
        fns["f64"] = block(A1, f64_name, "f64")
        if A0 is not None and first != "without":
            fns["f64-plain"] = block(A0, f64_name, "f64-plain")
        fns["f32"] = block(A1, f64_name + "_f32", "f32")
        fns["f64-single"] = singles("hip_matvec_kernel", "f64-single")
        fns["f32-single"] = singles("hip_matvec_kernel_f32", "f32-single")
        for fn in fns.values():
            fn()
        torch.cuda.synchronize()

        def columns(y):
            return y.t() if rm else y
        ref = ref32[:k]
        y32 = columns(Y["f32"])
        ok32 = bool(torch.isfinite(y32).all()) and \
            bool(((y32 - ref).abs() <= 1e-6 * ref.abs() + 1e-12 * ref.abs().max()).all())
        y1 = Y1["f64-single"]
        ok64 = all(bool(torch.isfinite(columns(Y[v])).all()) and
                   bool(((columns(Y[v]) - y1).abs() <= 1e-6 * y1.abs() + 1e-300).all()) for v in ("f64-plain", "f64") if v in fns)
        differs = float((y32 - columns(Y["f64"])).abs().max()) > 0.0
        ok = ok32 and ok64 and differs
        parity &= ok
        t_est = alternate(torch, {"f64": fns["f64"]}, 1, 1)["f64"][0]
        reps = int(min(max(0.02 / max(t_est, 1e-7), 1), 200))
        t = alternate(torch, fns, reps, bench.BATCHES)
        row = {"us": {v: round(1e6 * t[v][0], 2) for v in t}, "spread": {v: round(t[v][1], 3) for v in t},
               "f32_vs_f64": round(t["f32"][0] / t["f64"][0], 3),
               "f32_vs_k_f64_single": round(t["f32"][0] / t["f64-single"][0], 3),
               "f32_vs_k_f32_single": round(t["f32"][0] / t["f32-single"][0], 3),
               "f64_vs_k_f64_single": round(t["f64"][0] / t["f64-single"][0], 3),
               "reps": reps, "parity_f32_vs_rounded_csr": ok32, "parity_f64_vs_single": ok64,
               "f32_differs_from_f64": differs}
        if "f64-plain" in t:
            row["f64_vs_f64_plain"] = round(t["f64"][0] / t["f64-plain"][0], 3)
        rows[str(k)] = row
        note("k = %d: f32 / f64 %.3f" % (k, row["f32_vs_f64"]))
        del Y, Y1, Xc, Xb, fns
    i1 = A1.info()

    def form(A):
        i = A.info()
        return {"waves": int(i.waves), "wave_tiles": int(i.wave_tiles), "col_slices": int(i.col_slices),
                "rowblocks": int(i.n_rowblocks), "unit_windows": int(i.unit_windows), "sym_tiles": int(i.sym_tiles),
                "sym_segments": int(i.sym_segments), "matmat_group": A.matmat_group(), "matmat_rm_group": A.matmat_rm_group()}
    out = {"config": cfg, "f32": True, "layout": layout, "first": first if plain else None, "workload": workload_name,
           "edge": edge if workload_name == "syn-nlpkkt" else None, "symmetric_path": sym, "nrows": n, "nnz": nnz,
           "group_f32": group, "value_mb": round(int(i1.value_bytes) / 1e6, 1),
           "values_f32_mb": round(A1.values_f32_bytes() / 1e6, 1),
           "launch_form": dict({"f64": form(A1)}, **({"f64-plain": form(A0)} if A0 is not None else {})),
           "k": rows, "parity": parity, "tune_seconds": tunes,
           "protocol": "alpha=%g beta=0, warm-up calls, hipEvent time per batch of calls, variants alternating inside "
                       "every one of %d rounds, median and (max - min) / median" % (bench.ALPHA, bench.BATCHES)}
    for A in (A0, A1):
        if A is not None:
            A.destroy()
    del X, ref32
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--edge", type=int, default=bench.DEFAULT_EDGE)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--f32", action="store_true",
                    help="the float block product against the fp64 one on one handle (see above)")
    ap.add_argument("--no-plain", action="store_true", help="--f32: no second handle tuned without the copy")
    ap.add_argument("--first", choices=["without", "with"], default="without",
                    help="--f32: which handle is tuned first and whose fp64 block is timed first in every round")
    args = ap.parse_args()
    import torch
    torch.cuda.set_device(0)
    ok = True
    for cfg in args.configs.split(","):
        if args.f32:
            wl, sym, extra = CONFIGS[cfg]
            line = json.dumps(run_f32(torch, cfg, wl, sym, extra, args.edge, args.threads, "cm", None, not args.no_plain,
                                      args.first))
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
