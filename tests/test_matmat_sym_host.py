"""spx.gpu.sym_matmat on the host (host-only tunes, no GPU): the option is validated, it makes the hand-over
atomic without a measurement and keeps wide row-blocks out of the stream, so that K copies of a row-block's
slots and y tile fit the LDS; with the option off the streams stay what they are; host-only handles serve no
group either way."""
import numpy as np
import pytest

import sparsex_amd as sx
from helpers import tune
from matmat_sym_cases import MATRICES, MAX_RB_ROWS, case_options, check_stream_fits, slotless_groups
from stream_decode import Stream

HOST_CASES = ("tiles", "segments", "no-slot")


@pytest.fixture(scope="module")
def matrices():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = MATRICES[name][0]()
        return cache[name]
    yield get
    cache.clear()
    sx.options_reset()


def _saved(tmp_path, csr, opts, tag):
    A = tune(csr, opts, sym=True, host_only=True)
    assert A.matmat_group() == -1, "a host-only handle serves no group"
    f = str(tmp_path / ("%s.spx" % tag))
    A.save(f)
    return f


def test_a_bad_value_fails_the_tune(matrices):
    csr, _ = matrices("tiles")
    for bad in ("auto", "1", ""):
        with pytest.raises(sx.SpxError):
            tune(csr, dict(case_options("tiles"), **{"spx.gpu.sym_matmat": bad}), sym=True, host_only=True)
    # ... also where the option would be ignored: a general tune
    with pytest.raises(sx.SpxError):
        tune(csr, dict(case_options("tiles"), **{"spx.gpu.sym_matmat": "yes"}), host_only=True)
    sx.options_reset()


@pytest.mark.parametrize("name", HOST_CASES)
def test_the_option_gives_a_stream_that_k_copies_fit(tmp_path, matrices, name):
    csr, m = matrices(name)
    opts = case_options(name)
    assert "spx.gpu.sym_spill" not in opts                    # (auto: resolved to atomic, not measured)
    s = check_stream_fits(_saved(tmp_path, csr, opts, "on"), m)
    r, c, v, _ = s.triplets()
    s.check_ownership()
    if name == "no-slot":
        assert slotless_groups(s) >= 1
    sx.options_reset()


@pytest.mark.parametrize("name", HOST_CASES)
def test_the_option_off_changes_no_stream(tmp_path, matrices, name):
    csr, m = matrices(name)
    on = case_options(name)
    unset = {k: v for k, v in on.items() if k != "spx.gpu.sym_matmat"}
    off = dict(on, **{"spx.gpu.sym_matmat": "false"})
    with open(_saved(tmp_path, csr, unset, "unset"), "rb") as f:
        a = f.read()
    with open(_saved(tmp_path, csr, off, "off"), "rb") as f:
        b = f.read()
    assert a == b
    sx.options_reset()


def test_the_default_still_emits_wide_row_blocks(tmp_path, matrices):
    """What the option takes away is there without it: the read-once segments of the stencil matrix sit in
    row-blocks of more than 512 rows (spx.gpu.sym_wide_rows = 1024)."""
    csr, m = matrices("segments")
    opts = {k: v for k, v in case_options("segments").items() if k != "spx.gpu.sym_matmat"}
    s = Stream(_saved(tmp_path, csr, opts, "default"))
    assert int(s.rbs["n_rows"].max()) > MAX_RB_ROWS
    sx.options_reset()


def test_lists_and_deterministic_keep_their_meaning(tmp_path, matrices):
    csr, m = matrices("tiles")
    for more in ({"spx.gpu.sym_spill": "lists"}, {"spx.gpu.deterministic": "true"}):
        s = Stream(_saved(tmp_path, csr, dict(case_options("tiles"), **more), "x"))
        assert s.sym_atomic == 0
        x = np.ones(m.shape[0])
        assert np.allclose(s.matvec(x), m @ x, rtol=1e-12, atol=1e-13)
    sx.options_reset()


def test_a_general_tune_ignores_the_option(tmp_path, matrices):
    csr, _ = matrices("tiles")

    def saved(opts, tag):
        A = tune(csr, opts, host_only=True)
        assert A.matmat_group() == -1
        f = str(tmp_path / tag)
        A.save(f)
        with open(f, "rb") as fh:
            return fh.read()
    on = case_options("tiles")
    assert saved(on, "on") == saved(dict(on, **{"spx.gpu.sym_matmat": "false"}), "off")
    sx.options_reset()
