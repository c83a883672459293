"""The rank program of test_gpu_dist_step.py: started under torch.distributed.run with gloo, it runs the attached
step (spx_hip_mat_dist_attach / spx_hip_matvec_dist) of every case of dist_cases.py whose world is this launch's,
on every rank against the float64 references of dist_cases.py -- the full product comes from the untuned CSR,
which every rank builds itself, so no rank depends on another's arithmetic.  Every rank's y0 holds NaN outside
its own rows and its own random values inside: a beta term read from the wrong rows, or applied once per
sender, shows.

One flushed JSON line per (case, path, family) goes to --out: {"id", "rank", "checks": {name: bool or max
error / bound}, "errors": [...]}.  Between two collectives nothing raises: a failed check is a record.  An
SpxError (or a HIP error) of a library call ends the worker non-zero; the launcher then ends the others."""
import argparse
import json
import os
import sys
import time
import traceback

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CHUNKS = (1, 4, 3)            # spx.rt.dist_chunks per rank in the second overlapped run: rank 0 cuts nothing
NVEC = 3


def record_ids(world):
    """The records a launch of `world` ranks writes, in order (test_gpu_dist_step.py parametrizes over them)."""
    import dist_cases as dc
    out = []
    for case, v in dc.CASES.items():
        if v[1] != world:
            continue
        out += ["%s/general/%s" % (case, f) for f in v[4]] + ["%s/symmetric/%s" % (case, f) for f in v[5]]
    return out


class Checks:
    def __init__(self):
        self.checks, self.errors = {}, []

    def run(self, name, fn):
        """fn() -> bool, or a max error / bound ratio; whatever it raises is a record, not an exception"""
        try:
            v = fn()
            self.checks[name] = bool(v) if isinstance(v, (bool, np.bool_)) else float(v)
        except Exception:
            self.errors.append("%s: %s" % (name, traceback.format_exc(limit=3)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(0)
    import sparsex_amd as sx
    from sparsex_amd import synth
    from sparsex_amd.dist_torch import torch_transport
    import dist_cases as dc
    sx.lib().spx_log_error_console()
    transport = torch_transport(rank, world)
    st = torch.cuda.current_stream().cuda_stream
    A_, B_ = dc.ALPHA_BETA
    B2 = 0.75
    out = open("%s.%d" % (args.out, rank), "a")            # (a file per rank: no two writers)
    mats = {}

    def gather_bits(y):
        """every rank's vector, as bit patterns, on every rank (collective)"""
        mine = torch.from_numpy(dc.bits(y).view(np.int64).copy())
        got = [torch.empty_like(mine) for _ in range(world)]
        dist.all_gather(got, mine)
        return [g.numpy().view(np.uint64) for g in got]

    def gather_to_rank0(y):
        mine = torch.from_numpy(dc.bits(y).view(np.int64).copy())
        got = [torch.empty_like(mine) for _ in range(world)] if rank == 0 else None
        dist.gather(mine, got, dst=0)
        return [g.numpy().view(np.uint64) for g in got] if rank == 0 else None

    for rid in record_ids(world):
        if args.only and args.only not in rid:
            continue
        t0 = time.perf_counter()
        case, path, family = rid.split("/")
        sym = path == "symmetric"
        if case not in mats:
            mats.clear()
            csr = dc.matrix(case)
            n = csr[3]
            m = dc.to_scipy(csr)
            cuts = dc.bounds(case, csr)
            xs = [synth.random_x(n, seed=5 + j) for j in range(NVEC)]
            y0_all = np.zeros(n)            # every rank's own values, on its rows
            for r in range(world):
                y0_all[cuts[r]:cuts[r + 1]] = dc.nan_outside(n, cuts[r], cuts[r + 1], seed=100 + r)[cuts[r]:cuts[r + 1]]
            mats[case] = (csr, n, m, cuts, xs, y0_all, {})
        csr, n, m, cuts, xs, y0_all, fulls = mats[case]
        lo, hi = cuts[rank], cuts[rank + 1]
        own = slice(lo, hi)
        y0 = dc.nan_outside(n, lo, hi, seed=100 + rank)
        nan = np.full(n, np.nan)
        xd = [torch.from_numpy(x).cuda() for x in xs]

        def full(j, alpha, beta, yy=None):
            """(value, bound) of alpha*A*x_j + beta*yy on all rows (yy: every rank's own y0 by default)"""
            key = (j, alpha, beta, yy is None)
            if key not in fulls:
                fulls[key] = dc.reference(m, 0, n, xs[j], alpha, beta, y0_all if yy is None else yy)
            return fulls[key]

        C = Checks()
        A = dc.tune_rows(csr, lo, hi, dc.family_options(case, family, sym), symmetric=sym)
        A.dist_attach(transport)
        plan, halo = A.dist_plan(), A.dist_halo()
        inf = A.info()
        C.run("rows", lambda: (inf.row_lo, inf.row_hi) == (lo, hi) and list(plan["row_lo"]) == cuts[:-1])
        if sym:
            C.run("conflict rows travel", lambda: (len(plan["send_rows"]) > 0) == (rank > 0))
        else:
            C.run("nothing to add", lambda: len(plan["send_rows"]) == 0 and not plan["any_exchange"])

        def step(j, alpha, beta, start, flags):
            y = torch.from_numpy(start.copy()).cuda()
            A.hip_matvec_dist(alpha, xd[j].data_ptr(), beta, y.data_ptr(), flags, st)
            torch.cuda.synchronize()
            return y.cpu().numpy()

        def own_ratio(y, j, alpha, beta):
            ref, bound = full(j, alpha, beta)
            return dc.max_ratio(y, ref, bound, own)

        def halo_checks(tag, y, theirs, j, alpha, beta):
            C.run(tag + ": own rows", lambda: own_ratio(y, j, alpha, beta))
            rc = halo["recv_cols"]
            owner = np.searchsorted(np.asarray(cuts[1:]), rc, side="right")
            C.run(tag + ": halo entries are their owner's",
                  lambda: all(np.array_equal(dc.bits(y)[rc[owner == q]], theirs[q][rc[owner == q]]) for q in range(world)))
            C.run(tag + ": halo entries", lambda: dc.max_ratio(y, *full(j, alpha, beta), rows=rc))
            if not sym:
                rest = np.ones(n, dtype=bool)
                rest[own] = False
                rest[rc] = False
                C.run(tag + ": the other rows keep their NaN", lambda: np.array_equal(dc.bits(y)[rest], dc.bits(y0)[rest]))

        # 1. the owned rows
        y = step(0, A_, B_, y0, sx.SPX_DIST_OWNED_ROWS)
        C.run("owned rows, beta", lambda: own_ratio(y, 0, A_, B_))
        y = step(0, 0.5, 0.0, nan, sx.SPX_DIST_OWNED_ROWS)
        C.run("owned rows, beta = 0 over NaN", lambda: own_ratio(y, 0, 0.5, 0.0))
        # 2. all of y on every rank, the same bits everywhere
        y = step(0, A_, B_, y0, sx.SPX_DIST_GATHER_Y)
        C.run("gather: every row", lambda: dc.max_ratio(y, *full(0, A_, B_)))
        everybody = gather_to_rank0(y)
        if rank == 0:
            C.run("gather: the ranks hold the same bits", lambda: all(np.array_equal(e, everybody[0]) for e in everybody))
        # 3. the halo of x
        y_halo = step(0, A_, B_, y0, sx.SPX_DIST_HALO_X)
        halo_checks("halo", y_halo, gather_bits(y_halo), 0, A_, B_)
        # 4. ... pipelined over parts of the own product (general path; elsewhere the plain order runs)
        if not sym:
            if case in dc.OVERLAP:
                C.run("overlap: parts", lambda: A.dist_parts() >= 2 and len(A.dist_rounds()) >= 2)
            y = step(0, A_, B_, y0, sx.SPX_DIST_HALO_X | sx.SPX_DIST_OVERLAP)
            halo_checks("overlap", y, gather_bits(y), 0, A_, B_)
            if family == "det":
                C.run("overlap: the bits of the plain order", lambda: np.array_equal(dc.bits(y), dc.bits(y_halo)))
            if case in dc.OVERLAP:
                # ... and with another number of parts on every rank: one without parts serves rounds it has none for
                sx.option_set("spx.rt.dist_chunks", str(CHUNKS[rank]))
                A.dist_attach(transport)
                halo = A.dist_halo()
                C.run("overlap, uneven: parts", lambda: (A.dist_parts() >= 2) == (CHUNKS[rank] > 1) and len(A.dist_rounds()) >= 2)
                y = step(0, A_, B_, y0, sx.SPX_DIST_HALO_X | sx.SPX_DIST_OVERLAP)
                halo_checks("overlap, uneven", y, gather_bits(y), 0, A_, B_)
                if family == "det":
                    C.run("overlap, uneven: the bits of the plain order", lambda: np.array_equal(dc.bits(y), dc.bits(y_halo)))
        # 5. two steps in a row (the send and receive buffers are used again), another x and beta
        flags = sx.SPX_DIST_HALO_X | (0 if sym else sx.SPX_DIST_OVERLAP)
        ya = step(0, A_, B_, y0, flags)
        yb = step(1, 0.5, B2, y0, flags)
        C.run("two steps: first", lambda: own_ratio(ya, 0, A_, B_))
        C.run("two steps: second", lambda: own_ratio(yb, 1, 0.5, B2))
        C.run("two steps: second, halo entries", lambda: dc.max_ratio(yb, *full(1, 0.5, B2), rows=halo["recv_cols"]))
        if sym and family == "det":
            yc = step(1, 0.5, B2, y0, flags)
            C.run("the same step twice: the same bits", lambda: np.array_equal(dc.bits(yb)[own], dc.bits(yc)[own]))
        # 6. the plain entry points of an attached matrix: the rows it owns or adds to, nothing else
        first = int(plan["send_rows"][0]) if len(plan["send_rows"]) else lo
        wrote = np.zeros(n, dtype=bool)
        wrote[own] = True
        wrote[plan["send_rows"]] = True
        part = (dc.symmetric_part if sym else dc.general_part)(m, lo, hi)
        Y = torch.full((NVEC, n + 2), float("nan"), dtype=torch.float64, device="cuda")
        Y[:, :n] = torch.from_numpy(y0)
        X = torch.full((NVEC, n + 1), float("nan"), dtype=torch.float64, device="cuda")
        X[:, :n] = torch.from_numpy(np.stack(xs))
        y1 = torch.from_numpy(y0.copy()).cuda()
        A.hip_matvec_kernel(A_, xd[0].data_ptr(), B_, y1.data_ptr(), st)
        A.hip_matmat_kernel(A_, X.data_ptr(), n + 1, NVEC, B_, Y.data_ptr(), n + 2, st)
        torch.cuda.synchronize()
        y1, Yh = y1.cpu().numpy(), Y.cpu().numpy()
        outside = np.ones(n, dtype=bool)
        outside[first:hi] = False
        for tag, col, j in [("plain matvec", y1, 0)] + [("plain matmat %d" % j, Yh[j, :n], j) for j in range(NVEC)]:
            C.run(tag + ": rows it owns or adds to",
                  lambda: dc.max_ratio(col, *dc.reference(part, lo, hi, xs[j], A_, B_, y0), rows=wrote))
            # (a row of [first conflict row, lo) that it does not add to: cleared, or left as it is)
            between = ~outside & ~wrote
            C.run(tag + ": rows in between are 0 or untouched",
                  lambda: bool(np.all((col[between] == 0.0) | (dc.bits(col)[between] == dc.bits(y0)[between]))))
            C.run(tag + ": the rest is untouched", lambda: np.array_equal(dc.bits(col)[outside], dc.bits(y0)[outside]))
            if tag == "plain matvec":
                hit = np.nonzero(outside & (dc.bits(col) != dc.bits(y0)))[0]
                inside = np.nonzero(~outside & ~wrote & (dc.bits(col) != dc.bits(y0)))[0]
                note = {"first": first, "lo": lo, "hi": hi, "written outside": [int(hit.size)] + [int(v) for v in hit[:3]] + [int(v) for v in hit[-2:]],
                        "written inside, not added to": [int(inside.size)] + [int(v) for v in inside[:3]],
                        "values": [float(v) for v in col[hit[:3]]]}
        C.run("plain matmat: padding", lambda: bool(np.isnan(Yh[:, n:]).all()))
        # 7. host vectors: all of y on every rank (the same y0 everywhere)
        yh0 = synth.random_x(n, seed=77)
        yh = yh0.copy()
        A.matvec_kernel(A_, xs[2], B_, yh)
        C.run("host vectors: every row", lambda: dc.max_ratio(yh, *full(2, A_, B_, yh0)))
        A.destroy()
        sx.options_reset()
        out.write(json.dumps({"id": rid, "rank": rank, "world": world, "checks": C.checks, "errors": C.errors, "note": note,
                              "seconds": round(time.perf_counter() - t0, 3)}) + "\n")
        out.flush()
    out.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
