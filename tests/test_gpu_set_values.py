"""New values for a tuned pattern in HBM: spx_hip_mat_set_values (csx_refresh_values_kernel) in front of every
kind of product, against the CSR arrays with the NEW values (helpers.check_y: relative 1e-6 and the fp64 bound).
test_values_plan.py proves on the CPU that the plan names the right positions; here the kernel applies it."""
import numpy as np
import pytest

import sparsex_amd as sx
from sparsex_amd import synth
from helpers import check_y

import dist_cases as dc
import limit_cases as lc
import values_cases as vc

pytestmark = pytest.mark.gpu

ALPHA, BETA = lc.ALPHA_BETA
W4 = {"spx.gpu.waves": "4"}

# name -> (matrix, symmetric, options): one representative of every kernel family
FAMILIES = {
    "plain": ("cant", False, dict(lc.OFF_FAMILIES["plain"], **W4)),
    "unit-windows": ("cant", False, dict(lc.OFF_FAMILIES["unit-windows"], **W4)),
    "slices-c2": ("cant", False, dict(lc.OFF_FAMILIES["slices-c2"], **W4)),
    "sym-tiles": ("nd24k", True, dict(lc.SYM_FAMILIES["lists"], **W4)),
    "sym-tiles-atomic": ("nd24k", True, dict(lc.SYM_FAMILIES["atomic"], **W4)),
    "sym-segments": ("nlpkkt", True, dict(lc.SYM_FAMILIES["segments"], **W4)),
    "sym-pipeline": ("pipeline", True, dict(lc.SYM_FAMILIES["pipeline"], **W4)),
    "sym-mirrored": ("cant", True, dict({"spx.gpu.sym_once": "false"}, **W4)),
    "sym-matmat": ("nlpkkt", True, dict({"spx.gpu.sym_matmat": "true", "spx.gpu.sym_segments": "true"}, **W4)),
}
MATRICES = {
    "cant": lambda: synth.syn_cant(0.02),
    "nd24k": lambda: synth.syn_nd24k(0.02),
    "nlpkkt": lambda: synth.syn_nlpkkt(8),
    "pipeline": dc.MATRICES["pipeline"],
}


class Data:
    """A matrix, its two new value arrays (general and symmetric), x, y0 -- made once, never written again."""

    def __init__(self, name):
        self.csr = MATRICES[name]()
        self.n = self.csr[3]
        self.x = synth.random_x(self.n, seed=3)
        self.X = np.stack([synth.random_x(self.n, seed=30 + j) for j in range(3)])
        self.y0 = synth.random_x(self.n, seed=4)
        self.v = {(sym, seed): vc.new_values(self.csr, sym, seed) for sym in (False, True) for seed in (1, 2)}
        for a in (self.x, self.X, self.y0) + tuple(self.v.values()):
            a.setflags(write=False)

    def new(self, sym, seed=1):
        return vc.with_values(self.csr, self.v[(sym, seed)])


@pytest.fixture(scope="module")
def data():
    import torch
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Data(name)
        return cache[name]
    yield get
    cache.clear()
    sx.options_reset()
    torch.cuda.empty_cache()


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.float64)).cuda()      # (a copy: the shared arrays are read-only)


def product(A, d, alpha=ALPHA, beta=BETA):
    """y <- alpha A x + beta y0 through spx_hip_matvec_kernel, as a numpy array"""
    import torch
    x, y = dev(d.x), dev(d.y0)
    A.hip_matvec_kernel(alpha, x.data_ptr(), beta, y.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return y.cpu().numpy()


def planned(d, sym, opts):
    A = vc.tune(d.csr, opts, sym=sym)
    assert A.info().on_device
    A.values_plan(d.csr[0], d.csr[1])
    info = A.values_plan_info()
    # one uint32_t per position, each array padded to a multiple of four
    assert info["plan_bytes"] == 4 * sum((info[k] + 3) // 4 * 4 for k in ("n_values", "n_mirror", "n_diag"))
    return A


@pytest.mark.parametrize("family", list(FAMILIES))
def test_products_after_an_update(data, family):
    import torch
    name, sym, opts = FAMILIES[family]
    d = data(name)
    A = planned(d, sym, opts)
    inf = A.info()
    if family == "unit-windows":
        assert inf.unit_windows == 1
    if family == "slices-c2":
        assert inf.col_slices == 2
    if family == "sym-pipeline":
        assert inf.sym_pipeline == 1
    if family.startswith("sym-tiles"):
        assert inf.sym_tiles == (2 if family.endswith("atomic") else 1)
    new = d.new(sym)
    v1 = dev(new[2])
    A.set_values(v1)
    check_y(new, d.x, product(A, d), ALPHA, BETA, d.y0)
    # ... three vectors at once
    X, Y = dev(d.X), dev(np.stack([d.y0] * 3))
    A.matmat(ALPHA, X, BETA, Y)
    torch.cuda.synchronize()
    Yh = Y.cpu().numpy()
    for j in range(3):
        check_y(new, d.X[j], Yh[j], ALPHA, BETA, d.y0)
    # ... and the values of the tune again
    A.set_values(dev(d.csr[2]))
    check_y(d.csr, d.x, product(A, d), ALPHA, BETA, d.y0)
    A.destroy()


@pytest.mark.parametrize("windows", ["true", "false"])
def test_transposed_product_after_an_update(data, windows):
    import torch
    d = data("cant")
    A = planned(d, False, dict(lc.OFF_FAMILIES["unit-windows"], **{"spx.gpu.waves": "4", "spx.gpu.trans_windows": windows}))
    assert A.trans_mode() == (2 if windows == "true" else 1)
    new = d.new(False)
    A.set_values(dev(new[2]))
    x, y = dev(d.x), dev(d.y0)
    A.matvec_trans(ALPHA, x, BETA, y)
    torch.cuda.synchronize()
    t = vc.to_scipy(new).T.tocsr()
    t.sort_indices()
    check_y((t.indptr, t.indices, t.data, d.n), d.x, y.cpu().numpy(), ALPHA, BETA, d.y0)
    A.destroy()


@pytest.mark.parametrize("sym", [False, True])
def test_round_trip_is_bitwise_and_the_host_variant_agrees(data, sym):
    """spx.gpu.deterministic: V0 -> V1 -> V0 gives the bits of the first product; a host array gives the bits of
    the device tensor of the same numbers."""
    d = data("nd24k" if sym else "cant")
    opts = dict({"spx.gpu.deterministic": "true"}, **W4)
    if sym:
        opts["spx.gpu.sym_spill"] = "lists"
    A = planned(d, sym, opts)
    before = product(A, d)
    new = d.new(sym)
    A.set_values(dev(new[2]))
    from_device = product(A, d)
    check_y(new, d.x, from_device, ALPHA, BETA, d.y0)
    assert not np.array_equal(before, from_device)
    A.set_values(dev(d.csr[2]))
    assert np.array_equal(dc.bits(product(A, d)), dc.bits(before))
    A.set_values(np.array(new[2]))                    # numpy: spx_hip_mat_set_values_host
    assert np.array_equal(dc.bits(product(A, d)), dc.bits(from_device))
    A.destroy()


@pytest.mark.parametrize("sym", [False, True])
def test_saved_bytes_and_entries_show_the_new_values(tmp_path, data, sym):
    d = data("nd24k" if sym else "cant")
    A = planned(d, sym, W4)
    new = d.new(sym)
    A.set_values(dev(new[2]))
    m1 = vc.to_scipy(new)
    vc.check_stream(A, m1, tmp_path, sym)
    vc.check_entries(A, m1, limit=200)
    # an edit behind a bulk update (the wait-once rule), and a bulk update behind an edit
    r, c = vc.coords(d.csr)
    k = r.size // 2
    A.set_entry(int(r[k]), int(c[k]), 3.25)
    assert A.get_entry(int(r[k]), int(c[k])) == 3.25 and A.get_entry(int(r[k - 1]), int(c[k - 1])) == new[2][k - 1]
    A.set_values(dev(d.v[(sym, 2)]))
    m2 = vc.to_scipy(d.new(sym, 2))
    vc.check_stream(A, m2, tmp_path, sym)
    with pytest.raises(sx.api.SpxError):
        A.export_csx(0)
    assert len(A.export_units(0)) > 0
    # ... and the file carries no stale partitions: the restored matrix shows the new values and exports nothing
    f = str(tmp_path / "after.spx")
    A.save(f)
    A.destroy()
    sx.options_reset()
    B = sx.mat_restore(f)
    assert B.info().on_device
    vc.check_entries(B, m2, limit=100)
    with pytest.raises(sx.api.SpxError):
        B.export_csx(0)
    B.destroy()


def test_tails_of_the_three_arrays(tmp_path, data):
    """A symmetric slice whose value array, thin mirror list and diagonal are no multiples of four long, and whose
    diagonal starts on an odd row (the kernel's stores of that array are then 8 bytes wide)."""
    import torch
    csr = dc.matrix(dc.THIN_MIRROR)
    n = csr[3]
    cuts = dc.bounds(dc.THIN_MIRROR, csr)
    lo, hi = cuts[-2] | 1, cuts[-1]                   # (the balanced cut of the last rank, on an odd row)
    A = dc.tune_rows(csr, lo, hi, dc.family_options(dc.THIN_MIRROR, "lists", True), True)
    rp, ci, va, _ = csr
    part = ((rp[lo:hi + 1] - rp[lo]).astype(np.int32), ci[rp[lo]:rp[hi]].copy(), va[rp[lo]:rp[hi]].copy(), n)
    A.values_plan(part[0], part[1])
    info = A.values_plan_info()
    assert lo % 2 == 1 and all(info[k] > 0 and info[k] % 4 for k in ("n_values", "n_mirror", "n_diag")), \
        [info[k] for k in ("n_values", "n_mirror", "n_diag")]
    v1 = vc.new_values(part, True, 5, row0=lo)
    A.set_values(dev(v1))
    import scipy.sparse as sp
    low = sp.tril(vc.to_scipy(vc.with_values(part, v1), row0=lo, nrows=n)).tocsr()
    full = (low + sp.tril(low, -1).T).tocsr()
    vc.check_stream(A, full, tmp_path, True)
    x = synth.random_x(n, seed=8)
    xd = dev(x)
    y = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    A.hip_matvec_kernel(ALPHA, xd.data_ptr(), 0.0, y.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    full.sort_indices()
    check_y((full.indptr, full.indices, full.data, n), x, y.cpu().numpy(), ALPHA)
    A.destroy()


@pytest.mark.parametrize("sym", [False, True])
def test_one_nonzero(sym):
    import torch
    one = (np.array([0, 1], np.int32), np.array([0], np.int32), np.array([2.5]), 1)
    A = vc.tune(one, W4, sym=sym)
    A.values_plan(one[0], one[1])
    A.set_values(dev(np.array([-7.0])))
    x = dev(np.array([3.0]))
    y = dev(np.array([10.0]))
    A.hip_matvec_kernel(2.0, x.data_ptr(), 0.5, y.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert y.cpu().numpy()[0] == 2.0 * -7.0 * 3.0 + 5.0 and A.get_entry(0, 0) == -7.0
    A.destroy()


@pytest.mark.parametrize("sym", [False, True])
def test_update_and_product_in_one_captured_graph(data, sym):
    import torch
    d = data("nlpkkt")
    A = planned(d, sym, dict(lc.SYM_FAMILIES["segments"], **W4) if sym else W4)
    src = dev(d.v[(sym, 1)])
    x = dev(d.x)
    y = torch.zeros(d.n, dtype=torch.float64, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    A.hip_set_values(src.data_ptr(), s)                            # warm-up outside the capture
    A.hip_matvec_kernel(ALPHA, x.data_ptr(), 0.0, y.data_ptr(), s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = torch.cuda.current_stream().cuda_stream               # one stream, one chain: update, then product
        A.hip_set_values(src.data_ptr(), cap)
        A.hip_matvec_kernel(ALPHA, x.data_ptr(), 0.0, y.data_ptr(), cap)
    g.replay()
    torch.cuda.synchronize()
    check_y(d.new(sym, 1), d.x, y.cpu().numpy(), ALPHA)
    src.copy_(dev(d.v[(sym, 2)]))                                   # new numbers where the graph reads them
    g.replay()
    torch.cuda.synchronize()
    check_y(d.new(sym, 2), d.x, y.cpu().numpy(), ALPHA)
    A.destroy()


@pytest.mark.parametrize("sym", [False, True])
def test_two_row_slices(data, sym):
    """World 2, one rank after the other in this process: each plans from the whole CSR and takes the whole value
    array; the owned rows (general) or the sum of the partial vectors (symmetric) are the product."""
    import torch
    d = data("nlpkkt")
    new = d.new(sym)
    v1, x = dev(new[2]), dev(d.x)
    total = np.zeros(d.n)
    covered = 0
    for rank in range(2):
        A = dc.tune_rank(d.csr, rank, 2, dict(dc.NOSAMPLE, **W4), sym)
        inf = A.info()
        A.values_plan(d.csr[0], d.csr[1])
        A.set_values(v1)
        y = torch.zeros(d.n, dtype=torch.float64, device="cuda")
        A.hip_matvec_kernel(ALPHA, x.data_ptr(), 0.0, y.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        yh = y.cpu().numpy()
        if sym:
            total += yh
        else:
            total[inf.row_lo:inf.row_hi] = yh[inf.row_lo:inf.row_hi]
        covered += inf.row_hi - inf.row_lo
        A.destroy()
    assert covered == d.n
    check_y(new, d.x, total, ALPHA)


@pytest.mark.parametrize("sym", [False, True])
def test_restored_matrix(tmp_path, data, sym):
    d = data("nlpkkt")
    A = vc.tune(d.csr, W4, sym=sym)
    f = str(tmp_path / "saved.spx")
    A.save(f)
    A.destroy()
    sx.options_reset()
    B = sx.mat_restore(f)
    assert B.info().on_device
    B.values_plan(d.csr[0], d.csr[1])
    new = d.new(sym)
    B.set_values(dev(new[2]))
    check_y(new, d.x, product(B, d), ALPHA, BETA, d.y0)
    B.destroy()


def test_calls_that_must_fail(data, capfd):
    d = data("cant")
    A = vc.tune(d.csr, W4)
    v = dev(d.csr[2])
    with pytest.raises(sx.api.SpxError):
        A.hip_set_values(v.data_ptr())                # no plan yet
    A.values_plan(d.csr[0], d.csr[1])
    assert sx.lib().spx_hip_mat_set_values(A.handle, None, None) != 0
    A.set_values(v)
    A.values_plan_drop()
    with pytest.raises(sx.api.SpxError):
        A.hip_set_values(v.data_ptr())
    check_y(d.csr, d.x, product(A, d), ALPHA, BETA, d.y0)
    capfd.readouterr()
    A.destroy()
