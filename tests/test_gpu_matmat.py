"""The multi-vector product spx_hip_matmat_kernel / Matrix.matmat on the GPU: every column against the CSR
product (helpers.check_y), over full, partial and several groups, on every kind of stream the multi-vector
kernels run (unit, gather and window passes, over-long rows, column phases, column slices in one launch,
symmetric streams without tiles) and on the tile / read-once streams that fall back to one product per
column; padding, beta = 0 over NaN, row slices, argument checks, bit-identity under spx.gpu.deterministic and
a captured graph.  Tuned matrices are shared per module."""
import json
import os

import numpy as np
import pytest
import scipy.sparse as sp

import sparsex_amd as sx
from sparsex_amd import synth
from helpers import GOLDEN, check_y, tune
from matmat_cases import NOSAMPLE, block as _block, long_rows as _long_rows, run, to_scipy

pytestmark = pytest.mark.gpu

NVECS = (1, 2, 3, 5, 8, 13)


def _golden(name):
    with open(os.path.join(GOLDEN, "reference_matrices.json")) as f:
        m = json.load(f)[name]
    return (np.array(m["rowptr"], dtype=np.int32), np.array(m["colind"], dtype=np.int32),
            np.array(m["values"]), m["n"])


# name -> (generator, options, symmetric tune, multi-vector kernels expected)
CASES = {
    "demopatt": (lambda: _golden("demopatt"), {"spx.preproc.xform": "all"}, False, True),
    "golden-symmetric": (lambda: _golden("symmetric"), {"spx.preproc.xform": "all"}, False, True),
    "cant": (lambda: synth.syn_cant(0.05), NOSAMPLE, False, True),
    "webbase": (lambda: synth.syn_webbase(0.02), NOSAMPLE, False, True),
    "nlpkkt": (lambda: synth.syn_nlpkkt(20), NOSAMPLE, False, True),
    "long-rows": (_long_rows, NOSAMPLE, False, True),
    "waves2": (lambda: synth.syn_cant(0.05), dict(NOSAMPLE, **{"spx.gpu.waves": "2"}), False, True),
    "waves8": (lambda: synth.syn_webbase(0.02), dict(NOSAMPLE, **{"spx.gpu.waves": "8"}), False, True),
    "phases-c2": (lambda: synth.syn_nlpkkt(20), dict(NOSAMPLE, **{"spx.gpu.col_phases": "c2"}), False, True),
    "phases-c4": (lambda: synth.syn_webbase(0.02), dict(NOSAMPLE, **{"spx.gpu.col_phases": "c4"}), False, True),
    "phases-2": (lambda: synth.syn_nlpkkt(20), dict(NOSAMPLE, **{"spx.gpu.col_phases": "2"}), False, True),
    "unit-windows": (lambda: synth.syn_nlpkkt(20), dict(NOSAMPLE, **{"spx.gpu.unit_windows": "true"}), False, True),
    "no-x-window": (lambda: synth.syn_webbase(0.02), dict(NOSAMPLE, **{"spx.gpu.x_window": "false"}), False, True),
    "sym-no-once": (lambda: synth.syn_nlpkkt(20), dict(NOSAMPLE, **{"spx.gpu.sym_once": "false",
                                                                   "spx.gpu.sym_segments": "false"}), True, True),
    "sym-tiles": (lambda: synth.syn_nd24k(0.05), NOSAMPLE, True, False),
    "sym-segments": (lambda: synth.syn_nlpkkt(20), dict(NOSAMPLE, **{"spx.gpu.sym_segments": "true"}), True, False),
}


@pytest.fixture(scope="module")
def tuned():
    cache = {}

    def get(name):
        if name not in cache:
            gen, opts, sym, _ = CASES[name]
            csr = gen()
            cache[name] = (csr, tune(csr, opts, sym=sym))
        return cache[name]
    yield get
    cache.clear()
    sx.options_reset()


def _run(torch, A, csr, nvec, alpha, beta, padx=0, pady=0):
    run(torch, A, to_scipy(csr), nvec, alpha, beta, padx, pady)


@pytest.mark.parametrize("name", list(CASES))
def test_columns_match_the_csr_product(tuned, name):
    import torch
    csr, A = tuned(name)
    native = CASES[name][3]
    g = A.matmat_group()
    if native:
        assert g >= 2, "%s: the multi-vector kernels should run (group %d)" % (name, g)
    else:
        assert g == 1, "%s: tiles / read-once segments run one product per column (group %d)" % (name, g)
    for k, nvec in enumerate(NVECS):
        alpha, beta = ((0.5, 0.0), (2.0, -0.5), (0.0, 0.75))[k % 3]
        _run(torch, A, csr, nvec, alpha, beta, padx=3 if k % 2 else 0, pady=5 if k % 2 else 0)


@pytest.mark.parametrize("name", ["cant", "webbase", "long-rows", "sym-no-once"])
def test_padding_and_beta_zero_over_nan(tuned, name):
    import torch
    csr, A = tuned(name)
    _run(torch, A, csr, 5, 0.5, 0.0, padx=7, pady=9)
    _run(torch, A, csr, 8, 1.0, 0.0, padx=1, pady=1)


def test_zero_vectors_is_a_no_op(tuned):
    import torch
    csr, A = tuned("cant")
    n = csr[3]
    X = torch.zeros((0, n), dtype=torch.float64, device="cuda")
    Y = torch.zeros((0, n), dtype=torch.float64, device="cuda")
    A.matmat(1.0, X, 0.0, Y)
    A.hip_matmat_kernel(1.0, 0, n, 0, 0.0, 0, n, torch.cuda.current_stream().cuda_stream)


def test_bad_arguments_fail(tuned):
    import torch
    csr, A = tuned("cant")
    n = csr[3]
    s = torch.cuda.current_stream().cuda_stream
    buf = torch.zeros((4, n), dtype=torch.float64, device="cuda")
    base = buf.data_ptr()
    with pytest.raises(sx.SpxError):                      # X and Y overlap
        A.hip_matmat_kernel(1.0, base, n, 2, 0.0, base + 8 * n, n, s)
    with pytest.raises(sx.SpxError):                      # the same block
        A.hip_matmat_kernel(1.0, base, n, 1, 0.0, base, n, s)
    with pytest.raises(sx.SpxError):                      # ldx < ncols
        A.hip_matmat_kernel(1.0, base, n - 1, 2, 0.0, base + 16 * n, n, s)
    with pytest.raises(sx.SpxError):                      # ldy < nrows
        A.hip_matmat_kernel(1.0, base, n, 2, 0.0, base + 16 * n, n - 1, s)
    with pytest.raises(sx.SpxError):                      # NULL
        A.hip_matmat_kernel(1.0, 0, n, 2, 0.0, base + 16 * n, n, s)
    with pytest.raises(sx.SpxError):                      # three vectors 2^62 doubles apart: past the address space
        A.hip_matmat_kernel(1.0, base, 1 << 62, 3, 0.0, base + 16 * n, n, s)
    with pytest.raises(sx.SpxError):                      # ... of Y
        A.hip_matmat_kernel(1.0, base, n, 3, 0.0, base + 24 * n, 1 << 62, s)
    torch.cuda.synchronize()
    assert not buf.any()
    # (adjacent, not overlapping: fine)
    buf[:2] = torch.from_numpy(np.stack([synth.random_x(n, seed=j) for j in range(2)])).cuda()
    A.hip_matmat_kernel(1.0, base, n, 2, 0.0, base + 16 * n, n, s)
    torch.cuda.synchronize()
    for j in range(2):
        check_y(csr, buf[j].cpu().numpy(), buf[2 + j].cpu().numpy(), 1.0)


@pytest.mark.parametrize("sym", [False, True], ids=["general", "symmetric"])
def test_row_slice_writes_the_rows_of_the_single_product(sym):
    import torch
    N = 12
    n = synth.nlpkkt_nrows(N)
    lo, hi = n // 4, (3 * n) // 4
    rl, cl, vl, _ = synth.syn_nlpkkt_rows(N, lo, hi)
    sx.options_reset()
    opts = dict(NOSAMPLE, **{"spx.rt.row_offset": str(lo), "spx.rt.global_rows": str(n)})
    if sym:
        opts.update({"spx.matrix.symmetric": "true", "spx.gpu.sym_once": "false", "spx.gpu.sym_segments": "false"})
    for k, v in opts.items():
        sx.option_set(k, v)
    inp = sx.input_load_csr(rl, cl, vl, hi - lo, n)
    A = sx.mat_tune(inp)
    assert A.nrows == n
    s = torch.cuda.current_stream().cuda_stream
    for nvec, beta in ((3, 0.0), (5, 0.5)):
        _, X = _block(torch, A.ncols, nvec, 0, 7)
        _, Y = _block(torch, A.nrows, nvec, 0, 0, 123.0)
        Y1 = Y.clone()
        A.matmat(0.5, X, beta, Y)
        for j in range(nvec):
            A.hip_matvec_kernel(0.5, X[j].data_ptr(), beta, Y1[j].data_ptr(), s)
        torch.cuda.synchronize()
        y, y1 = Y.cpu().numpy(), Y1.cpu().numpy()
        assert np.array_equal(y == 123.0, y1 == 123.0), "not the rows the single-vector product writes"
        assert np.allclose(y, y1, rtol=1e-13, atol=1e-13)
    del A
    inp.destroy()
    sx.options_reset()


@pytest.mark.parametrize("gen,sym", [(lambda: synth.syn_cant(0.05), False), (lambda: synth.syn_webbase(0.02), False),
                                     (_long_rows, False), (lambda: synth.syn_nlpkkt(20), True)],
                         ids=["cant", "webbase", "long-rows", "nlpkkt-sym-no-once"])
def test_deterministic_columns_are_bit_identical(gen, sym):
    import torch
    csr = gen()
    opts = dict(NOSAMPLE, **{"spx.gpu.deterministic": "true"})
    if sym:
        opts.update({"spx.gpu.sym_once": "false", "spx.gpu.sym_segments": "false"})
    A = tune(csr, opts, sym=sym)
    assert A.matmat_group() >= 2
    n = csr[3]
    s = torch.cuda.current_stream().cuda_stream
    nvec = 13
    _, X = _block(torch, n, nvec, 0, 31)
    y0 = torch.stack([torch.from_numpy(synth.random_x(n, seed=300 + j)) for j in range(nvec)]).cuda()
    for _ in range(2):
        Y, Y1 = y0.clone(), y0.clone()
        A.matmat(0.5, X, 0.25, Y)
        for j in range(nvec):
            A.hip_matvec_kernel(0.5, X[j].data_ptr(), 0.25, Y1[j].data_ptr(), s)
        torch.cuda.synchronize()
        assert torch.equal(Y, Y1), "column differs from the single-vector product"


def test_captured_matmat_replays(tuned):
    import torch
    csr, A = tuned("nlpkkt")
    rp, ci, va, n = csr
    nvec = 5
    _, X = _block(torch, n, nvec, 2, 51)
    Y = torch.zeros((nvec, n), dtype=torch.float64, device="cuda")
    A.matmat(0.5, X, 0.0, Y)                                        # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(4):                                          # Y <- 0.5 A X + 0.25 Y, four times
            A.matmat(0.5, X, 0.25, Y)
    a = sp.csr_matrix((va, ci, rp), shape=(n, n))
    for rep in range(3):                                            # new inputs, same graph
        for j in range(nvec):
            X[j] = torch.from_numpy(synth.random_x(n, seed=500 + 10 * rep + j))
        Y.fill_(float(rep))
        g.replay()
        torch.cuda.synchronize()
        Xh, Yh = X.cpu().numpy(), Y.cpu().numpy()
        for j in range(nvec):
            ref = np.full(n, float(rep))
            for _ in range(4):
                ref = 0.5 * (a @ Xh[j]) + 0.25 * ref
            assert np.allclose(Yh[j], ref, rtol=1e-12, atol=1e-13)
