"""The streams test_gpu_random_paths.py runs on the GPU, host-only: the values plan of every one of them
(test_values_plan.full_check: the plan against the numpy decoder of the saved stream and against spx_mat_get_entry),
and the census that keeps the GPU file honest -- what the randomised streams and the zoo hold today, as conditions:
where a change of the encoder moves a stream below one of them, this file fails instead of the GPU file quietly
testing less.  The figures behind the conditions were counted on these streams (the per-case table is printed)."""
import pytest

import sparsex_amd as sx
from helpers import tune
import limit_cases as lc
import matmat_cases as mc
import random_cases as rc
from test_values_plan import full_check

_census = {}


def _general(seed):
    csr, m = rc.general_matrix(seed)
    return csr, mc.load_rect(sx, csr, m.shape[1], rc.general_options(seed), host_only=True)


def _zoo(xform):
    csr, _ = rc.zoo_matrix()
    return csr, tune(csr, rc.zoo_options(xform), host_only=True)


def _symmetric(seed, matmat):
    csr, _ = rc.random_matrix(seed, symmetric=True)
    return csr, tune(csr, rc.sym_matmat_options(seed) if matmat else rc.sym_options(seed), sym=True, host_only=True)


def census_of(tmp_path, kind, key):
    """the census of a case, taken once per session (before full_check writes other values into the stream)"""
    if (kind, key) not in _census:
        csr, A = {"general": _general, "zoo": _zoo, "sym-matmat": lambda s: _symmetric(s, True)}[kind](key)
        _census[(kind, key)] = rc.census(A, str(tmp_path / "census.spx"))
        _census[(kind, key)].pop("stream")
        A.destroy()
    return _census[(kind, key)]


# ---- the values plan ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", rc.GENERAL_SEEDS)
def test_values_plan_general(tmp_path, seed):
    csr, A = _general(seed)
    assert (A.ncols < A.nrows) == rc.is_rect(seed)
    full_check(A, csr, False, tmp_path, seed=seed)
    A.destroy()


@pytest.mark.parametrize("xform", rc.ZOO_XFORMS)
def test_values_plan_zoo(tmp_path, xform):
    csr, A = _zoo(xform)
    full_check(A, csr, False, tmp_path)
    A.destroy()


@pytest.mark.parametrize("matmat", [False, True], ids=["default", "sym_matmat"])
@pytest.mark.parametrize("seed", rc.SYM_SEEDS)
def test_values_plan_symmetric(tmp_path, seed, matmat):
    csr, A = _symmetric(seed, matmat)
    full_check(A, csr, True, tmp_path, seed=seed)
    A.destroy()


# ---- the census -----------------------------------------------------------------------------------------------------

def test_zoo_sweep_reaches_every_unit_kind(tmp_path):
    """unit kinds 0 .. 4 (block, horizontal, vertical, diagonal, anti-diagonal); the anti-diagonal at steps 1 and 3
    and the vertical at steps 1 and 2: what the general seeds do not reach (below)"""
    steps = {}
    for xform in rc.ZOO_XFORMS:
        c = census_of(tmp_path, "zoo", xform)
        print(rc.census_line("zoo " + xform, c))
        for k, st in c["unit_steps"].items():
            steps.setdefault(k, set()).add(st)
    assert set(steps) == {0, 1, 2, 3, 4}, steps
    assert {1, 3} <= steps[4], steps
    assert {1, 2} <= steps[2], steps


def test_general_seeds_hold_window_plans(tmp_path):
    """at least 30 of the 40 general streams can stage unit windows of x (33 when this was written), a rectangular
    one among them; which unit kinds the seeds hold is printed: no anti-diagonal unit (kind 4), the vertical kind in
    three seeds"""
    with_plan, kinds, rect_plan = [], {}, []
    for seed in rc.GENERAL_SEEDS:
        c = census_of(tmp_path, "general", seed)
        print(rc.census_line("seed %d%s" % (seed, " rect" if rc.is_rect(seed) else ""), c))
        if c["windows"]:
            with_plan.append(seed)
            if rc.is_rect(seed):
                rect_plan.append(seed)
        for k in c["unit_steps"]:
            kinds.setdefault(k, []).append(seed)
    print("window plan: %d seeds; unit kind -> seeds: %s" % (len(with_plan), {k: len(v) for k, v in sorted(kinds.items())}))
    assert len(with_plan) >= 30
    assert rect_plan


def test_symmetric_seeds_serve_groups(tmp_path):
    """spx.gpu.sym_matmat=true on seeds 40 .. 89: read-once passes with a group of two or more on at least 15
    streams (18), a group of four on at least one, segments without a slot on at least 3 (4), tiles and segments in
    one stream on at least 4 (6)"""
    grouped, four, slotless, both = [], [], [], []
    for seed in rc.SYM_SEEDS:
        c = census_of(tmp_path, "sym-matmat", seed)
        print(rc.census_line("seed %d" % seed, c))
        if rc.has_read_once(c) and c["group"] >= 2:
            grouped.append(seed)
            if c["group"] == 4:
                four.append(seed)
        if c["slotless"] > 0:
            slotless.append(seed)
        if {lc.PASS_SYMTILE, lc.PASS_SYMSEG} <= c["pass_kinds"]:
            both.append(seed)
    print("group >= 2: %s\ngroup 4: %s\nslotless segments: %s\ntiles and segments: %s" % (grouped, four, slotless, both))
    assert len(grouped) >= 15
    assert len(four) >= 1
    assert len(slotless) >= 3
    assert len(both) >= 4
