#!/usr/bin/env python3
"""Records tests/golden/set_problem_paths.json, the fixture of
tests/test_gpu_set_problem_paths.py: one scene per route that
sfm_ba_set_problem takes (host counts or device validation; small or sorted
layouts; in-line or deferred uv; parameters staged early, staged late, or on
the side stream from one of its three enqueue points).

Per scene the fixture holds digests, not arrays:
  evaluate   SHA-256 of evaluate()'s cost, residual and Jacobian bytes
  trace      the solve's iteration trace, floats as hex
  params     SHA-256 of the three parameter arrays after the solve

It was recorded on the commit BEFORE set_problem was split into a host plan
and staged passes (ba_problem.hip); the tests assert equality bit for bit,
i.e. that the route a problem takes, however the code that picks it is
arranged, leaves every result alone.  The fixture rests on run-to-run bitwise
reproducibility (atomics-free reductions), as the path-against-path tests do;
`--check` records again and compares with the file instead of writing it.
Re-record only for a change that is meant to move the bits.

Run on a GPU machine from the repository root:
  python tests/golden/make_set_problem_paths.py [--check] [OUT_JSON]
"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

FIXTURE = os.path.join(ROOT, "tests", "golden", "set_problem_paths.json")
INT_FIELDS = ("iteration", "step_is_valid", "step_is_successful")
FLOAT_FIELDS = ("cost", "cost_change", "gradient_max_norm", "step_norm", "relative_decrease", "trust_region_radius")


def _dup_shuffled():
    """The "dup-shuffled" scene of test_gpu_scale.py's _small_setup_scenes()."""
    from sfm_amd import scene
    s = scene.generate(12, 400, views=4, seed=23)
    rng = np.random.default_rng(5)
    dup = rng.choice(len(s.pt_idx), 40, replace=False)
    s.uv = np.vstack([s.uv, (s.uv[dup] + rng.normal(0, 0.3, (40, 2))).reshape(-1, 2)])
    s.cam_idx = np.concatenate([s.cam_idx, s.cam_idx[dup].astype(np.int32)])
    s.pt_idx = np.concatenate([s.pt_idx, s.pt_idx[dup].astype(np.int32)])
    perm = rng.permutation(len(s.pt_idx))
    s.uv, s.cam_idx, s.pt_idx = s.uv[perm], s.cam_idx[perm], s.pt_idx[perm]
    return s


def _generate(*a, **kw):
    from sfm_amd import scene
    return scene.generate(*a, **kw)


def _config(name):
    from sfm_amd import scene
    return scene.config(name)


# name -> (observations or None, what it reaches, scene maker); the smallest scenes that reach each route
SCENES = {
    "c1": (20000, "host counts, small path, early parameters, return without synchronisation",
           lambda: _config("C1")),
    "dup_shuffled": (None, "small path with caller-order duplicates", _dup_shuffled),
    "sorted_130": (18000, "host counts, sorted path (8515 blocks), XCD block order, one-pass back substitution, "
                   "early parameters", lambda: _generate(130, 3000, views=6)),
    "above_stage_44k": (44000, "N <= 65536 but input above the stage: device validation, in-line uv, late staged "
                        "parameters", lambda: _generate(12, 11000, views=4)),
    "side_params_66k": (66000, "device validation, side-stream parameters enqueued after the layouts",
                        lambda: _generate(50, 22000, views=3)),
    "deferred_late_300k": (300000, "deferred uv, late parameters", lambda: _generate(50, 20000, views=15, seed=5)),
    "deferred_worker_264k": (264000, "deferred uv, parameters from the worker",
                             lambda: _generate(100, 22000, views=12)),
}


def make_scene(name):
    n_obs, _, make = SCENES[name]
    s = make()
    assert n_obs is None or len(s.pt_idx) == n_obs, (name, len(s.pt_idx))
    return s


def _sha(*arrays):
    m = hashlib.sha256()
    for a in arrays:
        m.update(np.ascontiguousarray(a).tobytes())
    return m.hexdigest()


def record(s):
    """set_problem, evaluate and solve of scene s on a fresh handle: its fixture entry."""
    import sfm_amd
    with sfm_amd.BundleAdjuster() as ba:
        ba.set_problem(s.uv, s.cam_idx, s.pt_idx, s.K, s.rot, s.t, s.X)
        cost, res, jac = ba.evaluate()
        sm, tr = ba.solve()
        params = ba.parameters()
    trace = [[int(it[k]) for k in INT_FIELDS] + [float(it[k]).hex() for k in FLOAT_FIELDS] for it in tr]
    return {"n_obs": int(len(s.pt_idx)), "evaluate": _sha(np.float64(cost), res, jac), "trace": trace,
            "final_cost": float(sm.final_cost).hex(), "params": _sha(*params)}


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--check"]
    out = args[0] if args else FIXTURE
    got = {name: record(make_scene(name)) for name in SCENES}
    if "--check" in sys.argv[1:]:
        with open(out) as f:
            want = json.load(f)
        bad = [name for name in SCENES if want.get(name) != got[name]]
        print("reproduced" if not bad else f"NOT reproduced: {bad}")
        sys.exit(1 if bad else 0)
    with open(out, "w") as f:
        json.dump(got, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out, {k: (v["n_obs"], len(v["trace"])) for k, v in got.items()})
