#!/usr/bin/env python3
"""Records tests/golden/backsolve_parent.json: the SHA-256 of the bytes of y
and the fail word that dense_spd_solve at the checked-out commit gives on
tests/chol_child.py's `well(n)` systems (its "bits" mode), on the default
path and under SFM_CHOL_NO_SMALL=1 (a child process each: the knob is read
once per process), so that a change to the back substitution that must not
change a bit can be held to it (tests/test_gpu_backsolve_rows.py).  Needs a
GPU and the built library.

The sizes are the smallest that reach every shape of a row group of the back
substitution (block rows nb = ceil(n / 64)): both residues of nb mod 2 and
all three of nb mod 3, a partial last block, one full group, many groups.

Everything is recorded twice; an entry whose two recordings differ is kept
with "reproduces": false, and the run fails: every one of these must
reproduce.

Run from the repository root, on the commit BEFORE the change:
    python tests/golden/make_backsolve_parent.py [output.json]
"""
from __future__ import annotations

import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

SIZES = (1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 257, 320, 321, 384, 385, 449, 639, 1279, 3007)
PATHS = {"default": {}, "no_small": {"SFM_CHOL_NO_SMALL": "1"}}


def digest(entry):
    """{"sha256", "fail"} of one [hex of y's bytes, fail] of tests.chol_child."""
    return dict(sha256=hashlib.sha256(bytes.fromhex(entry[0])).hexdigest(), fail=int(entry[1]))


def main():
    from tests import chol_child as CC

    def once():
        out = {}
        for path, env in PATHS.items():
            got = CC.in_child("bits", list(SIZES), **env)
            for n in SIZES:
                out[f"{path}/{n}"] = digest(got[str(n)])
        return out

    a, b = once(), once()
    out, bad = {}, []
    for key in a:
        same = a[key] == b[key]
        out[key] = dict(reproduces=same, record=a[key])
        if not same:
            bad.append(key)
    print(f"{len(a)} entries, {len(bad)} not reproduced: {bad}")
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "backsolve_parent.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    assert not bad, bad


if __name__ == "__main__":
    main()
