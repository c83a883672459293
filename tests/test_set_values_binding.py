"""The Python side of the bulk value update: the symbols and their argument types, Matrix.set_values choosing
the host path for a numpy array, and what it refuses before anything reaches the library."""
import ctypes as C

import numpy as np
import pytest

import sparsex_amd as sx
from sparsex_amd import synth
from sparsex_amd.api import SpxError, ValuesPlan

import values_cases as vc

SYMBOLS = {
    "spx_hip_mat_values_plan": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int],
    "spx_hip_mat_values_plan_drop": [C.c_void_p],
    "spx_hip_mat_set_values": [C.c_void_p, C.c_void_p, C.c_void_p],
    "spx_hip_mat_set_values_host": [C.c_void_p, C.c_void_p],
    "spx_hip_mat_values_plan_get": [C.c_void_p, C.POINTER(ValuesPlan)],
}


def test_argtypes():
    L = sx.lib()
    for name, types in SYMBOLS.items():
        fn = getattr(L, name)
        assert list(fn.argtypes) == types, name
    # the struct of include/sparsex_hip.h: three pointers, three size_t, three uint64_t
    assert C.sizeof(ValuesPlan) == 9 * 8
    for m in ("values_plan", "values_plan_drop", "values_plan_info", "hip_set_values", "set_values"):
        assert callable(getattr(sx.api.Matrix, m))


@pytest.fixture(scope="module")
def planned():
    csr = synth.syn_nlpkkt(5)
    A = vc.tune(csr, {}, host_only=True)
    A.values_plan(csr[0], csr[1])
    yield A, csr
    A.destroy()


def test_numpy_takes_the_host_path(planned):
    A, csr = planned
    assert not A.info().on_device
    v1 = vc.new_values(csr, False, 21)
    A.set_values(v1)                       # (a host-only matrix has no other path: this is the host call)
    r, c = vc.coords(csr)
    for k in (0, v1.size // 3, v1.size - 1):
        assert A.get_entry(int(r[k]), int(c[k])) == v1[k]
    info = A.values_plan_info()
    assert info["n_sources"] == v1.size and info["plan_bytes"] == 0


def test_what_set_values_refuses(planned):
    A, csr = planned
    good = vc.new_values(csr, False, 22)
    A.set_values(good)
    for bad in (good.astype(np.float32), good[:-1].copy(), np.concatenate([good, [1.0]]), good.reshape(1, -1),
                np.concatenate([good, good])[::2], list(good), None):
        with pytest.raises(SpxError):
            A.set_values(bad)
    torch = pytest.importorskip("torch")
    for bad in (torch.from_numpy(good), torch.from_numpy(good).to(torch.float32), torch.from_numpy(good)[:-1]):
        with pytest.raises(SpxError):
            A.set_values(bad)              # (a CPU tensor: the device path wants HBM, the host path numpy)
    r, c = vc.coords(csr)
    assert A.get_entry(int(r[7]), int(c[7])) == good[7]
    A.values_plan_drop()
    with pytest.raises(SpxError):
        A.set_values(good)
    A.values_plan(csr[0], csr[1])
