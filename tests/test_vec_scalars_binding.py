"""The device-scalar calls at the library boundary: exported by libsparsex.so and declared, with their argument
types, in the ctypes binding.  No GPU needed (nothing is called)."""
import ctypes as C
import subprocess

import sparsex_amd as sx

NEW = {"spx_hip_vec_mul_dev": 4, "spx_hip_vec_scale_add_ratio": 7, "spx_hip_vec_cg_update": 8}


def test_device_scalar_symbols_are_exported():
    out = subprocess.check_output(["nm", "-D", "--defined-only", sx.lib_path()]).decode()
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert not [n for n in NEW if n not in exported]


def test_device_scalar_calls_have_argtypes():
    L = sx.lib()
    for name, nargs in NEW.items():
        at = getattr(L, name).argtypes
        assert at is not None and len(at) == nargs, name
    # the coefficient of scale_add_ratio travels as a double, everything else as a pointer
    assert L.spx_hip_vec_scale_add_ratio.argtypes[3] is C.c_double
    assert all(t is C.c_void_p for k, t in enumerate(L.spx_hip_vec_scale_add_ratio.argtypes) if k != 3)
    assert all(t is C.c_void_p for t in L.spx_hip_vec_mul_dev.argtypes + L.spx_hip_vec_cg_update.argtypes)


def test_python_surface():
    for m in ("dot_into", "scale_add_ratio_into", "slot_ptr"):
        assert callable(getattr(sx.DeviceVector, m))
    assert callable(sx.cg_update)
