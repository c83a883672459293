"""spx.gpu.values_f32=all without a GPU: the third value of the option tunes general and symmetric host-only
matrices (no device copy: bytes -1), every other unknown value still fails the tune, the saved file of a symmetric
tune does not depend on the option, and the float entry points refuse the host-only symmetric handle."""
import pytest

import sparsex_amd as sx
from sparsex_amd import synth
from helpers import tune
import matmat_cases as mc

OPT = "spx.gpu.values_f32"
NR, NC = 300, 800


def _sym_csr():
    return synth.syn_nlpkkt(8)


def test_all_tunes_a_general_host_only_matrix():
    csr, m = mc.band(NR, 40, 0.2, ncols=NC)
    try:
        A = mc.load_rect(sx, csr, NC, dict(mc.NOSAMPLE, **{OPT: "all"}), host_only=True)
        assert (A.nrows, A.ncols) == (NR, NC)
        assert A.values_f32_bytes() == -1
        A.destroy()
    finally:
        sx.options_reset()


def test_all_tunes_a_symmetric_host_only_matrix():
    csr = _sym_csr()
    try:
        A = tune(csr, dict(mc.NOSAMPLE, **{OPT: "all"}), sym=True, host_only=True)
        assert A.info().symmetric
        assert A.values_f32_bytes() == -1
        A.destroy()
    finally:
        sx.options_reset()


@pytest.mark.parametrize("value", ["All", "both", "sym", "1"])
def test_other_values_still_fail_the_tune(value):
    csr = _sym_csr()
    try:
        with pytest.raises(sx.SpxError):
            tune(csr, dict(mc.NOSAMPLE, **{OPT: value}), sym=True, host_only=True)
    finally:
        sx.options_reset()


def test_saved_file_of_a_symmetric_tune_does_not_depend_on_the_option(tmp_path):
    csr = _sym_csr()
    blobs = {}
    try:
        for value in ("false", "true", "all"):
            A = tune(csr, dict(mc.NOSAMPLE, **{OPT: value}), sym=True, host_only=True)
            f = str(tmp_path / (value + ".spx"))
            A.save(f)
            A.destroy()
            blobs[value] = open(f, "rb").read()
    finally:
        sx.options_reset()
    assert len(blobs["false"]) > 0
    assert blobs["false"] == blobs["true"] == blobs["all"]


def test_restore_reads_all_without_a_device(tmp_path):
    """a host-only restore with the option set to all succeeds and keeps no copy; a bad value fails the restore"""
    csr = _sym_csr()
    try:
        A = tune(csr, dict(mc.NOSAMPLE), sym=True, host_only=True)
        f = str(tmp_path / "m.spx")
        A.save(f)
        A.destroy()
        sx.options_reset()
        sx.option_set("spx.rt.host_only", "true")
        sx.option_set(OPT, "all")
        B = sx.mat_restore(f)
        assert B.info().symmetric and B.values_f32_bytes() == -1
        B.destroy()
        sx.option_set(OPT, "some")
        with pytest.raises(sx.SpxError):
            sx.mat_restore(f)
    finally:
        sx.options_reset()


def test_float_entry_points_refuse_the_host_only_symmetric_handle():
    csr = _sym_csr()
    n = csr[3]
    L = sx.lib()
    try:
        A = tune(csr, dict(mc.NOSAMPLE, **{OPT: "all"}), sym=True, host_only=True)
        assert L.spx_hip_matvec_kernel_f32(1.0, A.handle, 8, 0.0, 1 << 40, None) == sx.SPX_FAILURE
        assert L.spx_hip_matvec_mult_f32(1.0, A.handle, 8, 1 << 40, None) == sx.SPX_FAILURE
        assert L.spx_hip_matvec_kernel_f32_vec(1.0, A.handle, None, 0.0, None, None) == sx.SPX_FAILURE
        with pytest.raises(sx.SpxError):
            A.hip_matvec_kernel_f32(1.0, 8, 0.0, 1 << 40)
        assert A.values_f32_bytes() == -1
        assert (A.nrows, A.ncols) == (n, n)
        A.destroy()
    finally:
        sx.options_reset()
