#!/usr/bin/env python3
"""Records tests/golden/dense_solve_parent.json: the SHA-256 of the bytes of y
and the fail word that sfm_dense_spd_solve and sfm_dense_spd_solve_panels
(panels of 1 and of 2 tiles) give on tests/chol_child.py's `well(n)` systems
at n = 129 and n = 200, so that a change to how these one-shot entry points
build their device problem can be held to the bits of the commit before it
(tests/test_gpu_regrow.py).  Needs a GPU and a built library.

Run from the repository root against the PARENT commit's library, built with
tools/mkrev.sh:
    bash tools/mkrev.sh parent HEAD~1
    SFM_AMD_LIB=$PWD/abvar/var_parent.so python tests/golden/make_dense_solve_parent.py [output.json]
Every entry is computed twice; the run fails if one does not reproduce.
"""
from __future__ import annotations

import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

SIZES = (129, 200)
PANEL_TILES = (1, 2)


def record():
    """{"<entry>/<n>": {"sha256", "fail"}} of the loaded library."""
    from sfm_amd.ba import dense_spd_solve, dense_spd_solve_panels
    from tests.chol_child import well

    out = {}
    for n in SIZES:
        A, b = well(n)
        y, _, fail = dense_spd_solve(A, b)
        out[f"solve/{n}"] = dict(sha256=hashlib.sha256(y.tobytes()).hexdigest(), fail=int(fail))
        for pt in PANEL_TILES:
            y, fail = dense_spd_solve_panels(A, b, pt)
            out[f"panels{pt}/{n}"] = dict(sha256=hashlib.sha256(y.tobytes()).hexdigest(), fail=int(fail))
    return out


def main():
    a, b = record(), record()
    bad = [k for k in a if a[k] != b[k]]
    print(f"{len(a)} entries, {len(bad)} not reproduced: {bad}")
    assert not bad, bad
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "dense_solve_parent.json")
    with open(path, "w") as f:
        json.dump(a, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
