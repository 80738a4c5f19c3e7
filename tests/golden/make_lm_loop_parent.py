#!/usr/bin/env python3
"""Records tests/golden/lm_loop_parent.json: what the solver at the checked-out
commit leaves behind on every scene and loop setting of tests/lm_loop_cases.py
(trace records, summary without the times, SHA-256 of the parameters), so that
a change to the LM loop that must not change behaviour can be held to it
(tests/test_gpu_lm_loop_parent.py).  Needs a GPU and the built library.

Everything is recorded twice; an entry whose two recordings differ is kept
with "reproduces": false and is not compared by the test.  At most two such
entries are tolerated, none of them on the scenes that pause and re-arm the
loop or take the invalid-step branch.

Run from the repository root, on the commit BEFORE the change:
    python tests/golden/make_lm_loop_parent.py [output.json]
"""
from __future__ import annotations

import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

MUST_REPRODUCE = ("reject_a", "llt_invalid", "rej_100_irr", "rej_130_irr")


def main():
    import lm_loop_cases as LC

    def once():
        out = {f"{name}/{env}": LC.record(name, env) for name in LC.scene_names() for env in LC.ENVS}
        out[LC.TWO_RANKS] = LC.record_two_ranks()
        return out

    a, b = once(), once()
    out, bad = {}, []
    for key in a:
        same = a[key] == b[key]
        out[key] = dict(reproduces=same, record=a[key])
        if not same:
            bad.append(key)
            out[key]["reason"] = "two recordings on the same commit differ"
    print(f"{len(a)} entries, {len(bad)} not reproduced: {bad}")
    assert len(bad) <= 2 and not any(k.split("/")[0] in MUST_REPRODUCE for k in bad), bad
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "lm_loop_parent.json")
    LC.dump_fixture(out, path)


if __name__ == "__main__":
    main()
