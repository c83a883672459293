"""What test_random_cases.py (CPU, host-only) and test_gpu_random_paths.py (GPU) share: the randomised matrices and
options of test_stream_random.py and the zoo of test_stream_layout.py, with the options the newer entry points need
-- the transposed product, the product with the float copy of the values, the bulk value refresh and the K-vector
product on read-once symmetric streams -- and the census of a saved stream that says what a case exercises.
No pytest code in here."""
import numpy as np
import scipy.sparse as sp

import limit_cases as lc
import matmat_cases as mc
import matmat_sym_cases as msc
from test_stream_layout import zoo
from test_stream_random import random_matrix, random_options, random_sym_options

GENERAL_SEEDS = range(40)
SYM_SEEDS = range(40, 90)
WAVES = (0, 2, 4, 8)
TRANS_WINDOWS = ("false", "true", "auto")
NVEC_SYM = 13                      # 8 + 4 + 1 in one call where the group is eight
PASS_NAMES = {0: "unit", 2: "gather", 3: "symtile", 4: "gather-lds", 5: "symseg"}


# ---- general streams --------------------------------------------------------------------------------------------

def unit_windows_choice(seed):
    """spx.gpu.unit_windows of a seed: forced on, forced off, or None (left to the tuner) -- by seed % 7, which
    shares no factor with the residues of the other choices (4: waves, 3: trans_windows, 5: deterministic)"""
    r = seed % 7
    return "true" if r < 3 else "false" if r == 3 else None


def general_options(seed):
    """random_options(seed) -- its draws stay what they are -- and what the newer paths need, each by arithmetic of
    its own on the seed."""
    o = random_options(seed)
    o["spx.gpu.values_f32"] = "true"
    o["spx.gpu.waves"] = str(WAVES[seed % 4])
    o["spx.gpu.trans_windows"] = TRANS_WINDOWS[seed % 3]
    uw = unit_windows_choice(seed)
    if uw is not None:
        o["spx.gpu.unit_windows"] = uw
    if seed % 5 == 0:
        o["spx.gpu.deterministic"] = "true"
    return o


def is_rect(seed):
    return seed % 4 == 1


def rect(seed):
    """random_matrix(seed) cut to its first ceil(2 n / 3) columns: (csr tuple, scipy matrix).  Rows that lose all
    their nonzeros stay, as empty rows."""
    _, m = random_matrix(seed, symmetric=False)
    n = m.shape[0]
    ncols = (2 * n + 2) // 3
    a = sp.csr_matrix(m[:, :ncols])
    a.sort_indices()
    return (a.indptr.astype(np.int32), a.indices.astype(np.int32), a.data.copy(), n), a


def general_matrix(seed):
    """(csr tuple, scipy matrix) of a general seed; the matrix of a seed with seed % 4 == 1 is rect(seed)"""
    return rect(seed) if is_rect(seed) else random_matrix(seed, symmetric=False)


# ---- the zoo ----------------------------------------------------------------------------------------------------

ZOO_XFORMS = ("all", "h", "v", "d", "ad", "br", "bc", "v{2},ad{3},d{2},h{4}")


def zoo_options(xform, more=None):
    """One transform at a time; row-blocks of 23 rows cut the multi-row units at their borders."""
    o = {"spx.preproc.xform": xform, "spx.preproc.sampling": "none", "spx.gpu.rowblock_rows": "23",
         "spx.gpu.values_f32": "true"}
    o.update(more or {})
    return o


def zoo_matrix():
    csr = zoo()
    return csr, mc.to_scipy(csr)


# ---- symmetric streams ------------------------------------------------------------------------------------------

def sym_options(seed):
    return random_sym_options(seed, random_options(seed))


def sym_matmat_options(seed):
    o = sym_options(seed)
    o["spx.gpu.sym_matmat"] = "true"
    o["spx.gpu.waves"] = str(WAVES[seed % 4])
    return o


# ---- what a saved stream holds ----------------------------------------------------------------------------------

def has_read_once(c):
    return bool(c["pass_kinds"] & {lc.PASS_SYMTILE, lc.PASS_SYMSEG})


def census(A, path, windows=True):
    """Saves `A` to `path` and returns what its stream holds: "pass_kinds" (set), "unit_steps" ({descriptor kind:
    largest step}, of the unit passes), "windows" (whether the unit windows of x can be planned for at least one
    row-block: A.unit_windows(3072, 16); general streams), "group" (matmat_sym_cases.expected_mvsym_group),
    "slotless" (read-once segment groups without a slot), "rows" (largest row-block) and the decoded stream."""
    A.save(path)
    c, s = lc.census(path)
    out = {"pass_kinds": set(c["kinds"]), "unit_steps": dict(c["steps"]), "rows": c["rows"], "stream": s,
           "group": msc.expected_mvsym_group(s), "slotless": msc.slotless_groups(s) if s.symmetric else 0,
           "windows": False}
    if windows and not s.symmetric:
        out["windows"] = A.unit_windows(3072, 16)["rowblocks_with_windows"] > 0
    return out


def expected_group(c, inf):
    """The group the device copy of a symmetric stream with the census `c` and the settings `inf` (Matrix.info())
    serves under spx.gpu.sym_matmat=true: matmat_sym_cases.expected_mvsym_group where it holds read-once passes; a
    stream without any (the mirror image is stored) goes through the K-vector kernels of the general path, whose
    rule is matmat_cases.expected_group: one copy of the y tiles, or one per wavefront."""
    if has_read_once(c):
        return c["group"]
    return mc.expected_group(c["rows"], inf.waves if inf.wave_tiles else 1)


def census_line(name, c):
    kinds = ",".join(PASS_NAMES.get(k, str(k)) for k in sorted(c["pass_kinds"]))
    steps = " ".join("%d:%d" % (k, st) for k, st in sorted(c["unit_steps"].items()))
    return "%-26s passes %-28s units(kind:step) %-24s windows %-3s group %d slotless %d" % (
        name, kinds, steps or "-", "yes" if c["windows"] else "no", c["group"], c["slotless"])
