#!/usr/bin/env python3
"""Diagonal scaling and norms of a tuned matrix next to the products and the value refresh, on ONE handle in one
process (bench.py's protocol: the synth generators, a warm-up call, hipEvent timing; the variants alternate inside
every one of 5 rounds -- tools/matmat_bench.py --f32's `alternate` -- and each reports its median and the spread
(max - min) / median):

    scale             spx_hip_mat_scale(dr, dc)      scale-dr / scale-dc: one vector only
    norms-<kind>-rows / -cols / -both                spx_hip_mat_norms, kind sum-abs, sum-sq, max-abs
    forward           spx_hip_matvec_kernel          (alpha = 0.5, beta = 0)
    transposed        spx_hip_matvec_trans_kernel
    set-values        spx_hip_mat_set_values         (needs a values plan: --no-set-values leaves it out)

    python3 tools/scale_bench.py [--configs e240,cant,webbase] [--edge 240] [--values-f32]
    python3 tools/scale_bench.py --sym [--configs e240,cant,nd24k]

--sym: the same workloads tuned as symmetric ones AND as general ones, both handles in the process, the variants of the
two alternating in the same rounds:

    sym-forward       spx_hip_matvec_kernel on the symmetric tune (what the ratios are taken against)
    sym-scale         spx_hip_mat_sym_scale(d)
    sym-norms-<kind>  spx_hip_mat_sym_norms
    forward, scale (dr = dc = d), norms-<kind>-both   the general tune of the same matrix, for comparison

Its gates: the max-abs norms of the symmetric handle against numpy bit for bit, its sum-abs norms against |A| 1
(relative 1e-9), and after one scaling the symmetric forward product against the CSR product of the scaled matrix.

The scale vectors hold +1 and -1 (a hash of the index): every multiplication is done, and a matrix scaled any
number of times keeps its magnitudes.  Gates, before anything is timed: the max-abs norms of the handle against
numpy over the CSR arrays bit for bit (rows) and the sum-abs norms against |A| 1 and |A|^T 1 (relative 1e-9),
and after one scaling the forward product against the CSR product of the
scaled matrix (relative 1e-6).  One JSON line per config; the configs of one run share a process, so their times
compare."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bench  # noqa: E402  (make_workload, tune, ALPHA, BATCHES: the bench protocol)
from matmat_bench import CONFIGS, workload, alternate  # noqa: E402

KINDS = (("sum-abs", 0), ("sum-sq", 1), ("max-abs", 2))


def signs(n, seed):
    """+1 / -1 from a hash of the index"""
    with np.errstate(over="ignore"):
        x = (np.arange(n, dtype=np.uint64) + np.uint64(seed)) * np.uint64(0x9E3779B97F4A7C15)
        x ^= x >> np.uint64(29)
    return np.where((x & np.uint64(1)) == 1, -1.0, 1.0)


def run(torch, cfg, edge, threads, values_f32, with_set_values):
    import scipy.sparse as sp
    from sparsex_amd import synth
    wl, sym, extra = CONFIGS[cfg]
    if sym:
        raise SystemExit("scale_bench: %s is a symmetric config; norms and scaling serve general tunes" % cfg)

    def note(msg):
        print("[scale_bench] %s: %s" % (cfg, msg), file=sys.stderr, flush=True)
    csr = workload(wl, edge)
    rp, ci, va, n = csr
    nnz = int(rp[-1])
    note("%s, %d rows, %d nonzeros" % (wl, n, nnz))
    opts = {"spx.rt.nr_threads": threads, "spx.rt.device": torch.cuda.current_device(),
            "spx.matrix.symmetric": "false", "spx.rt.keep_encoded": "false"}
    if values_f32:
        opts["spx.gpu.values_f32"] = "true"
    opts.update(extra)
    t0 = time.perf_counter()
    A = bench.tune(csr, opts)
    tune_s = time.perf_counter() - t0
    note("tuned in %.1f s" % tune_s)
    plan_s = None
    if with_set_values:
        t0 = time.perf_counter()
        A.values_plan(rp, ci)
        plan_s = time.perf_counter() - t0
    dev = torch.device("cuda", torch.cuda.current_device())
    stream = torch.cuda.current_stream().cuda_stream
    dr_h, dc_h = signs(n, 1), signs(n, 2)
    dr, dc = torch.from_numpy(dr_h).to(dev), torch.from_numpy(dc_h).to(dev)
    xh = synth.random_x(n, seed=42)
    x = torch.from_numpy(xh).to(dev)
    y = torch.full((n,), float("nan"), dtype=torch.float64, device=dev)
    yt = torch.full((n,), float("nan"), dtype=torch.float64, device=dev)
    rows = torch.full((n,), float("nan"), dtype=torch.float64, device=dev)
    cols = torch.full((n,), float("nan"), dtype=torch.float64, device=dev)
    vals = torch.from_numpy(va).to(dev) if with_set_values else None

    # gates (formed without a second copy of the index arrays: the bench matrix holds 769 M nonzeros)
    absa = np.abs(va)
    absm = sp.csr_matrix((absa, ci, rp), shape=(n, n))
    ones = np.ones(n)
    A.hip_mat_norms(0, rows.data_ptr(), cols.data_ptr(), stream)
    torch.cuda.synchronize()
    ok_norms = True
    for got, want in ((rows, absm @ ones), (cols, absm.T @ ones)):
        ok_norms &= bool((np.abs(got.cpu().numpy() - want) <= 1e-9 * want).all())
    A.hip_mat_norms(2, rows.data_ptr(), None, stream)
    torch.cuda.synchronize()
    want = np.maximum.reduceat(np.append(absa, 0.0), rp[:-1].astype(np.int64))       # (the last row's run takes the 0 in)
    want[np.diff(rp) == 0] = 0.0
    ok_norms &= bool(np.array_equal(rows.cpu().numpy(), want))
    del absa, absm, want
    A.hip_mat_scale(dr.data_ptr(), dc.data_ptr(), stream)
    A.hip_matvec_kernel(bench.ALPHA, x.data_ptr(), 0.0, y.data_ptr(), stream)
    torch.cuda.synchronize()
    # (factors of +-1 scale exactly: D_r A D_c x = dr .* (A (dc .* x)))
    ref = bench.ALPHA * (dr_h * (sp.csr_matrix((va, ci, rp), shape=(n, n)) @ (dc_h * xh)))
    yh = y.cpu().numpy()
    ok_scale = bool(np.isfinite(yh).all()) and bool((np.abs(yh - ref) <= 1e-6 * np.abs(ref) + 1e-12 * np.abs(ref).max()).all())
    del ref, yh
    note("gates: norms %s, scaled product %s" % (ok_norms, ok_scale))
    A.hip_mat_scale(dr.data_ptr(), dc.data_ptr(), stream)         # (and back: the signs square to one)
    torch.cuda.synchronize()

    fns = {
        "forward": lambda: A.hip_matvec_kernel(bench.ALPHA, x.data_ptr(), 0.0, y.data_ptr(), stream),
        "transposed": lambda: A.hip_matvec_trans_kernel(bench.ALPHA, x.data_ptr(), 0.0, yt.data_ptr(), stream),
        "scale": lambda: A.hip_mat_scale(dr.data_ptr(), dc.data_ptr(), stream),
        "scale-dr": lambda: A.hip_mat_scale(dr.data_ptr(), None, stream),
        "scale-dc": lambda: A.hip_mat_scale(None, dc.data_ptr(), stream),
    }
    for name, kind in KINDS:
        fns["norms-%s-rows" % name] = lambda kind=kind: A.hip_mat_norms(kind, rows.data_ptr(), None, stream)
        fns["norms-%s-cols" % name] = lambda kind=kind: A.hip_mat_norms(kind, None, cols.data_ptr(), stream)
        fns["norms-%s-both" % name] = lambda kind=kind: A.hip_mat_norms(kind, rows.data_ptr(), cols.data_ptr(), stream)
    if with_set_values:
        fns["set-values"] = lambda: A.hip_set_values(vals.data_ptr(), stream)
    # (a few milliseconds of work per batch, at least one call, an even count: the signs cancel)
    t_est = alternate(torch, {"forward": fns["forward"]}, 1, 1)["forward"][0]
    reps = int(min(max(0.02 / max(t_est, 1e-7), 2), 200)) & ~1
    t = alternate(torch, fns, reps, bench.BATCHES)
    fwd = t["forward"][0]
    info = A.info()
    n_values = int(info.value_bytes) // 8
    out = {"config": cfg, "workload": wl, "edge": edge if wl == "syn-nlpkkt" else None, "nrows": n, "nnz": nnz,
           "stream_values": n_values, "values_f32_mb": round(max(A.values_f32_bytes(), 0) / 1e6, 1),
           "waves": int(info.waves), "col_slices": int(info.col_slices), "unit_windows": int(info.unit_windows),
           "wave_tiles": int(info.wave_tiles), "rowblocks": int(info.n_rowblocks), "trans_mode": A.trans_mode(),
           "us": {k: round(1e6 * v[0], 2) for k, v in t.items()}, "spread": {k: round(v[1], 3) for k, v in t.items()},
           "vs_forward": {k: round(v[0] / fwd, 3) for k, v in t.items()},
           "scale_gb_per_s": round(16.0 * n_values / t["scale"][0] / 1e9, 1),
           "reps": reps, "gate_norms": ok_norms, "gate_scaled_product": ok_scale,
           "parity": ok_norms and ok_scale, "tune_seconds": round(tune_s, 2),
           "values_plan_seconds": None if plan_s is None else round(plan_s, 2),
           "protocol": "warm-up calls, hipEvent time per batch of calls, variants alternating inside every one of %d "
                       "rounds, median and (max - min) / median; scale vectors of +-1; scale_gb_per_s = 16 B per "
                       "stream value over the time of scale" % bench.BATCHES}
    A.destroy()
    del x, y, yt, rows, cols, dr, dc, vals
    torch.cuda.empty_cache()
    return out


def run_sym(torch, cfg, edge, threads, values_f32):
    """--sym: the symmetric and the general tune of one workload side by side"""
    import scipy.sparse as sp
    from sparsex_amd import synth
    wl = CONFIGS[cfg][0]

    def note(msg):
        print("[scale_bench --sym] %s: %s" % (cfg, msg), file=sys.stderr, flush=True)
    csr = workload(wl, edge)
    rp, ci, va, n = csr
    nnz = int(rp[-1])
    note("%s, %d rows, %d nonzeros" % (wl, n, nnz))
    base = {"spx.rt.nr_threads": threads, "spx.rt.device": torch.cuda.current_device(), "spx.rt.keep_encoded": "false"}
    t0 = time.perf_counter()
    S = bench.tune(csr, dict(base, **{"spx.matrix.symmetric": "true",
                                      **({"spx.gpu.values_f32": "all"} if values_f32 else {})}))
    G = bench.tune(csr, dict(base, **{"spx.matrix.symmetric": "false",
                                      **({"spx.gpu.values_f32": "true"} if values_f32 else {})}))
    tune_s = time.perf_counter() - t0
    note("both tuned in %.1f s" % tune_s)
    dev = torch.device("cuda", torch.cuda.current_device())
    stream = torch.cuda.current_stream().cuda_stream
    d_h = signs(n, 1)
    d = torch.from_numpy(d_h).to(dev)
    xh = synth.random_x(n, seed=42)
    x = torch.from_numpy(xh).to(dev)
    y, out, rows, cols = (torch.full((n,), float("nan"), dtype=torch.float64, device=dev) for _ in range(4))

    absa = np.abs(va)
    absm = sp.csr_matrix((absa, ci, rp), shape=(n, n))
    S.hip_mat_sym_norms(0, out.data_ptr(), stream)
    torch.cuda.synchronize()
    want = absm @ np.ones(n)
    ok_norms = bool((np.abs(out.cpu().numpy() - want) <= 1e-9 * want).all())
    S.hip_mat_sym_norms(2, out.data_ptr(), stream)
    torch.cuda.synchronize()
    want = np.maximum.reduceat(np.append(absa, 0.0), rp[:-1].astype(np.int64))
    want[np.diff(rp) == 0] = 0.0
    ok_norms &= bool(np.array_equal(out.cpu().numpy(), want))
    del absa, absm, want
    S.hip_mat_sym_scale(d.data_ptr(), stream)
    S.hip_matvec_kernel(bench.ALPHA, x.data_ptr(), 0.0, y.data_ptr(), stream)
    torch.cuda.synchronize()
    ref = bench.ALPHA * (d_h * (sp.csr_matrix((va, ci, rp), shape=(n, n)) @ (d_h * xh)))
    yh = y.cpu().numpy()
    ok_scale = bool(np.isfinite(yh).all()) and bool((np.abs(yh - ref) <= 1e-6 * np.abs(ref) + 1e-12 * np.abs(ref).max()).all())
    del ref, yh
    note("gates: norms %s, scaled product %s" % (ok_norms, ok_scale))
    S.hip_mat_sym_scale(d.data_ptr(), stream)                     # (and back: the signs square to one)
    torch.cuda.synchronize()

    fns = {
        "sym-forward": lambda: S.hip_matvec_kernel(bench.ALPHA, x.data_ptr(), 0.0, y.data_ptr(), stream),
        "sym-scale": lambda: S.hip_mat_sym_scale(d.data_ptr(), stream),
        "forward": lambda: G.hip_matvec_kernel(bench.ALPHA, x.data_ptr(), 0.0, y.data_ptr(), stream),
        "scale": lambda: G.hip_mat_scale(d.data_ptr(), d.data_ptr(), stream),
    }
    for name, kind in KINDS:
        fns["sym-norms-%s" % name] = lambda kind=kind: S.hip_mat_sym_norms(kind, out.data_ptr(), stream)
        fns["norms-%s-both" % name] = lambda kind=kind: G.hip_mat_norms(kind, rows.data_ptr(), cols.data_ptr(), stream)
    t_est = alternate(torch, {"sym-forward": fns["sym-forward"]}, 1, 1)["sym-forward"][0]
    reps = int(min(max(0.02 / max(t_est, 1e-7), 2), 200)) & ~1
    t = alternate(torch, fns, reps, bench.BATCHES)
    fwd = t["sym-forward"][0]
    si, gi = S.info(), G.info()
    s_values, g_values = int(si.value_bytes) // 8, int(gi.value_bytes) // 8
    res = {"config": cfg + "-sym", "workload": wl, "edge": edge if wl == "syn-nlpkkt" else None, "nrows": n, "nnz": nnz,
           "sym_stream_values": s_values, "general_stream_values": g_values, "values_f32": bool(values_f32),
           "waves": int(si.waves), "sym_tiles": int(si.sym_tiles), "sym_segments": int(si.sym_segments),
           "sym_pipeline": int(si.sym_pipeline), "rowblocks": int(si.n_rowblocks),
           "us": {k: round(1e6 * v[0], 2) for k, v in t.items()}, "spread": {k: round(v[1], 3) for k, v in t.items()},
           "vs_sym_forward": {k: round(v[0] / fwd, 3) for k, v in t.items()},
           "sym_scale_gb_per_s": round(16.0 * s_values / t["sym-scale"][0] / 1e9, 1),
           "scale_gb_per_s": round(16.0 * g_values / t["scale"][0] / 1e9, 1),
           "reps": reps, "gate_norms": ok_norms, "gate_scaled_product": ok_scale, "parity": ok_norms and ok_scale,
           "tune_seconds": round(tune_s, 2),
           "protocol": "warm-up calls, hipEvent time per batch of calls, the variants of both handles alternating inside "
                       "every one of %d rounds, median and (max - min) / median; scale vectors of +-1; gb_per_s = 16 B "
                       "per stream value over the time of the scaling" % bench.BATCHES}
    S.destroy()
    G.destroy()
    del x, y, out, rows, cols, d
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--configs", default="e240,cant,webbase", help="the general configs of tools/matmat_bench.py")
    ap.add_argument("--edge", type=int, default=bench.DEFAULT_EDGE)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--values-f32", action="store_true", help="tune with the float copy: scale rewrites it as well")
    ap.add_argument("--no-set-values", action="store_true", help="no values plan, no set-values variant")
    ap.add_argument("--sym", action="store_true", help="the symmetric tune next to the general one (see above)")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    import torch
    torch.cuda.set_device(0)
    ok = True
    for cfg in args.configs.split(","):
        if args.sym:
            line = json.dumps(run_sym(torch, cfg, args.edge, args.threads, args.values_f32))
        else:
            line = json.dumps(run(torch, cfg, args.edge, args.threads, args.values_f32, not args.no_set_values))
        print(line, flush=True)
        ok &= json.loads(line)["parity"]
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
