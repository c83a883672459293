"""The attached step on several ranks that share the one GPU: tests/dist_worker.py under a fresh
`python -m torch.distributed.run` child with gloo and torch_transport, started the way
test_gpu_multirank.run_bench starts bench.py.  One launch per world runs every case of dist_cases.py of that
world; every rank writes a record per (case, path, family), and each test here asserts on the records of one.
World 3 is not started where the launch of world 2 ended in an abort, a segmentation fault, a time limit or a
GPU fault; nothing is tried twice."""
import json
import os
import subprocess
import sys
import time

import pytest

import dist_worker
from test_gpu_multirank import ROOT, free_port

pytestmark = pytest.mark.gpu

WORLDS = (2, 3)
TIMEOUT = 900
FATAL = (134, 139, 124, 137, -6, -11, -9)


def launch(world, out):
    env = dict(os.environ)
    env.update({"SPX_BENCH_BACKEND": "gloo", "MASTER_ADDR": "127.0.0.1", "HSA_ENABLE_IPC_MODE_LEGACY": "0"})
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world),
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()),
           os.path.join(ROOT, "tests", "dist_worker.py"), "--out", out]
    t0 = time.perf_counter()
    try:
        p = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=TIMEOUT)
        code, text = p.returncode, p.stdout[-6000:] + "\n" + p.stderr[-6000:]
    except subprocess.TimeoutExpired as e:
        code = 124
        tail = [t.decode(errors="replace") if isinstance(t, bytes) else (t or "") for t in (e.stdout, e.stderr)]
        text = "timed out after %d s\n%s\n%s" % (TIMEOUT, tail[0][-3000:], tail[1][-3000:])
    records = {}
    for rank in range(world):
        f = "%s.%d" % (out, rank)
        if os.path.exists(f):
            with open(f) as fh:
                for line in fh:
                    rec = json.loads(line)
                    records[(rec["id"], rec["rank"])] = rec
    return {"code": code, "text": text, "records": records, "seconds": time.perf_counter() - t0,
            "fatal": code in FATAL or "illegal memory access" in text or "exitcode: -" in text}


@pytest.fixture(scope="module")
def launches(tmp_path_factory):
    """World 2, then world 3 -- unless world 2 ended in a way after which nothing more belongs on the GPU."""
    out = {}
    d = tmp_path_factory.mktemp("dist_step")
    for world in WORLDS:
        out[world] = launch(world, str(d / ("w%d.jsonl" % world)))
        print("world %d: %.1f s, exit code %d, %d records" % (world, out[world]["seconds"], out[world]["code"],
                                                             len(out[world]["records"])))
        if out[world]["fatal"]:
            break
    return out


@pytest.mark.parametrize("world", WORLDS)
def test_launch_ends_clean(launches, world):
    assert world in launches, "not started: the launch of world %d ended in a fault" % (world - 1)
    L = launches[world]
    print("world %d: %.1f s" % (world, L["seconds"]))
    assert L["code"] == 0, L["text"]
    assert L["seconds"] < 300, "the launch took %.0f s" % L["seconds"]


@pytest.mark.parametrize("world,rid", [(w, r) for w in WORLDS for r in dist_worker.record_ids(w)])
def test_attached_step(launches, world, rid):
    assert world in launches, "not started: the launch of world %d ended in a fault" % (world - 1)
    L = launches[world]
    sym = "/symmetric/" in rid
    for rank in range(world):
        rec = L["records"].get((rid, rank))
        assert rec is not None, "rank %d wrote no record for %s (exit code %d)\n%s" % (rank, rid, L["code"], L["text"][-3000:])
        assert not rec["errors"], "\n".join(rec["errors"])
        checks = rec["checks"]
        print(rank, json.dumps(checks), json.dumps(rec.get("note")))
        for name in ("rows", "owned rows, beta", "owned rows, beta = 0 over NaN", "gather: every row", "halo: own rows",
                     "halo: halo entries are their owner's", "two steps: first", "two steps: second",
                     "plain matvec: rows it owns or adds to", "plain matvec: the rest is untouched",
                     "plain matmat 2: rows it owns or adds to", "host vectors: every row"):
            assert name in checks, "rank %d: no check %r" % (rank, name)
        assert ("conflict rows travel" if sym else "nothing to add") in checks
        if rank == 0:
            assert "gather: the ranks hold the same bits" in checks
        if not sym:
            assert "overlap: own rows" in checks and "halo: the other rows keep their NaN" in checks
        for name, v in checks.items():
            if isinstance(v, bool):
                assert v, "rank %d: %s" % (rank, name)
            else:
                assert v <= 1.0, "rank %d: %s: max error / bound %g" % (rank, name, v)
