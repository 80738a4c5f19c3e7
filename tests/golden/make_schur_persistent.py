#!/usr/bin/env python3
"""Records tests/golden/schur_persistent.json, the fixture of
tests/test_gpu_schur_persistent.py: scenes of 128 cameras and more, whose
off-diagonal Schur pass is k_schur_pairs_rot_pw (several groups of slots per
wave, slot and camera records), solved by the device LM loop.

Per scene the fixture holds digests, not arrays:
  trace      the solve's iteration trace, floats as hex
  final_cost as hex
  params     SHA-256 of the three parameter arrays after the solve

It was recorded on the commit BEFORE that kernel existed (one group per wave,
k_schur_pairs_rot); the tests assert equality bit for bit, for every grid the
test knob SFM_SCHUR_WGS sets.  The fixture rests on run-to-run bitwise
reproducibility (atomics-free reductions); `--check` records again and
compares with the file instead of writing it.  Re-record only for a change
that is meant to move the bits.

Run on a GPU machine from the repository root:
  python tests/golden/make_schur_persistent.py [--check] [OUT_JSON]
"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FIXTURE = os.path.join(ROOT, "tests", "golden", "schur_persistent.json")
INT_FIELDS = ("iteration", "step_is_valid", "step_is_successful")
FLOAT_FIELDS = ("cost", "cost_change", "gradient_max_norm", "step_norm", "relative_decrease", "trust_region_radius")


def _generate(*a, **kw):
    from sfm_amd import scene
    return scene.generate(*a, **kw)


def _irregular(name):
    import irregular_cases as IC
    return IC.build(name)


def _first_order():
    # cameras 0, 1, 2 at rotations (0, 0, 0), (1e-9, 0, 0), (1e-7, 0, 0): the first two in the first-order branch
    from test_gpu_rotated_form import _small_angle_scene
    return _small_angle_scene()


def _irregular_fixture(name):
    with open(os.path.join(ROOT, "tests", "golden", "irregular.json")) as f:
        return json.load(f)[name]


# name -> (scene maker, lanes per block forced through SFM_SCHUR_PTS_SUB or None, irregular.json entry
# with the solve's mode and options or None)
SCENES = {
    "gen_128": (lambda: _generate(128, 3000, views=6), None, None),
    "gen_129": (lambda: _generate(129, 3000, views=6), None, None),
    "irr_136": (lambda: _irregular("irr_136"), None, None),
    "irr_100_hub": (lambda: _irregular("irr_100_hub"), None, None),  # (100 cameras: the pass of small systems)
    "rej_130_irr": (lambda: _irregular("rej_130_irr"), None, "rej_130_irr"),  # rejected steps: gated-off launches
    "sub_8": (lambda: _generate(136, 3000, views=10, seed=11), None, None),
    "sub_16": (lambda: _generate(136, 3000, views=10, seed=11), 16, None),
    "sub_32": (lambda: _generate(136, 3000, views=10, seed=11), 32, None),
    "sub_64": (lambda: _generate(136, 3000, views=10, seed=11), 64, None),
    "first_order": (_first_order, None, None),
}


def solve_kwargs(name):
    fx = SCENES[name][2]
    if fx is None:
        return {}
    import sfm_amd
    c = _irregular_fixture(fx)
    return dict(mode=c["mode"], options=sfm_amd.make_options(**c["options"]))


def digest(sm, tr, params):
    trace = [[int(it[k]) for k in INT_FIELDS] + [float(it[k]).hex() for k in FLOAT_FIELDS] for it in tr]
    m = hashlib.sha256()
    for a in params:
        m.update(np.ascontiguousarray(a).tobytes())
    return {"trace": trace, "final_cost": float(sm.final_cost).hex(), "params": m.hexdigest()}


def record(name, s=None):
    """One-shot solve of scene `name` (set_problem reads the environment's knobs): its fixture entry."""
    import sfm_amd
    make, sub, _ = SCENES[name]
    s = make() if s is None else s
    old = os.environ.get("SFM_SCHUR_PTS_SUB")
    if sub is not None:
        os.environ["SFM_SCHUR_PTS_SUB"] = str(sub)
    try:
        r, t, X = s.copy_params()
        sm, tr = sfm_amd.solve(s.uv, s.cam_idx, s.pt_idx, s.K, r, t, X, **solve_kwargs(name))
    finally:
        if sub is not None:
            if old is None:
                del os.environ["SFM_SCHUR_PTS_SUB"]
            else:
                os.environ["SFM_SCHUR_PTS_SUB"] = old
    return digest(sm, tr, (r, t, X)), (sm, tr, r, t, X)


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--check"]
    out = args[0] if args else FIXTURE
    got = {name: record(name)[0] for name in SCENES}
    if "--check" in sys.argv[1:]:
        with open(out) as f:
            want = json.load(f)
        bad = [name for name in SCENES if want.get(name) != got[name]]
        print("reproduced" if not bad else f"NOT reproduced: {bad}")
        sys.exit(1 if bad else 0)
    with open(out, "w") as f:
        json.dump(got, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out, {k: len(v["trace"]) for k, v in got.items()})
