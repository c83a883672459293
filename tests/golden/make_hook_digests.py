"""Generates tests/golden/reference_hook_digests.json: the sha256 of every hook text the reference's
include/sparsex/internals/CsxJit.hpp yields for oracle/build_ref.py's checks (the ${new_row_hook} and ${next_x}
literals, the unit routines' argument lists, ${body_hook} for the cases tests/test_oracle_golden.py builds).
Digests only: no text of the reference is stored.  Run where the reference tree is present
(SPX_REFERENCE_ROOT, as oracle/build_ref.py)."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import test_oracle_golden as t   # noqa: E402


def main():
    src = t._reference_header()
    if src is None:
        raise SystemExit("the reference tree is not present (SPX_REFERENCE_ROOT)")
    with open(os.path.join(HERE, "reference_hook_digests.json"), "w") as f:
        json.dump(t.hook_digests(src), f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
