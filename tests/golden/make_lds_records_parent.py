#!/usr/bin/env python3
"""Records tests/golden/lds_records_parent.json, the fixture of
tests/test_gpu_lds_records.py: small irregular scenes at the camera counts
where the passes that keep camera records in LDS change kernel
(k_point_eval_lds<64>, <512, 2>; k_schur_pairs_rot_pw at 8, 16, 32 and 64
lanes per block; k_backsub_pm up to its 512 records), solved for at most two
LM iterations.

Per case the fixture holds digests, not arrays:
  trace      the solve's iteration trace, floats as hex
  summary    termination type, iteration count, initial and final cost (hex)
  params     SHA-256 of the three parameter arrays after the solve

It was recorded on the commit BEFORE the records' LDS layout changed (a
37-double k_backsub_pm record read by 8-byte pairs, k_schur_pairs_rot_pw's
blocks 512 B apart); the layout moves no bit, and the test asserts equality.  The fixture rests on run-to-run bitwise
reproducibility (atomics-free reductions): everything is recorded twice and
the run fails if the two differ.  `--check` records again and compares with
the file instead of writing it.

Scenes (scene(case)): the generator's scene with point p cut to its first
1 + p % 10 observations, 40 observations doubled, all shuffled
(tests/irregular_cases.py's `irregular`, no camera emptied: every camera is
observed), and camera 0 at rotation exactly 0, so its records carry the
first-order flag.  The pair lists of the camera blocks then have every small
length (few are multiples of 8) and most blocks of the reduced system are
empty.

Run on a GPU machine from the repository root, on the commit BEFORE the change:
  python tests/golden/make_lds_records_parent.py [--check] [OUT_JSON]
"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FIXTURE = os.path.join(ROOT, "tests", "golden", "lds_records_parent.json")
INT_FIELDS = ("iteration", "step_is_valid", "step_is_successful")
FLOAT_FIELDS = ("cost", "cost_change", "gradient_max_norm", "step_norm", "relative_decrease", "trust_region_radius")
MAX_ITERATIONS = 2

# case -> (cameras, points, environment of set_problem / solve)
CASES = {
    "c60": (60, 1000, {}),    # k_point_eval_lds<64>
    "c65": (65, 1500, {}),    # the first k_point_eval_lds<512, 2>
    "c128": (128, 2000, {}),  # the first k_schur_pairs_rot_pw / k_backsub_pm
    "c128_sub8": (128, 2000, {"SFM_SCHUR_PTS_SUB": "8"}),
    "c128_sub16": (128, 2000, {"SFM_SCHUR_PTS_SUB": "16"}),
    "c128_sub32": (128, 2000, {"SFM_SCHUR_PTS_SUB": "32"}),
    "c128_sub64": (128, 2000, {"SFM_SCHUR_PTS_SUB": "64"}),
    "c129": (129, 2000, {}),
    "c129_sorted": (129, 2000, {"SFM_SMALL_SETUP": "0"}),  # the sorted layouts: the wave-major streams
    "c129_host": (129, 2000, {"SFM_HOST_LM": "1"}),
    "c512": (512, 3000, {}),  # k_backsub_pm's LDS full but for 12 records' worth: every record slot of thread < C
    "c513": (513, 3000, {}),  # control: k_point_eval_rc and the three-pass back substitution, unchanged
}

_scenes = {}


def scene(case):
    """The case's scene (cached per camera and point count; never modified by a solve)."""
    import irregular_cases as IC
    from sfm_amd import scene as S
    C, P, _ = CASES[case]
    if (C, P) not in _scenes:
        s = IC.irregular(S.generate(C, P, views=10, seed=11), seed=5, hubs=(), empty=(), dups=40, shuffle=True,
                         maxdeg=10)
        s.rot[0] = 0.0
        _scenes[(C, P)] = s
    return _scenes[(C, P)]


def digest(sm, tr, params):
    trace = [[int(it[k]) for k in INT_FIELDS] + [float(it[k]).hex() for k in FLOAT_FIELDS] for it in tr]
    m = hashlib.sha256()
    for a in params:
        m.update(np.ascontiguousarray(a).tobytes())
    summary = [int(sm.termination_type), int(sm.num_iterations), float(sm.initial_cost).hex(),
               float(sm.final_cost).hex()]
    return {"trace": trace, "summary": summary, "params": m.hexdigest()}


def record(case):
    """One-shot solve of the case (set_problem and solve read the environment's knobs): its fixture entry."""
    import sfm_amd
    s = scene(case)
    env = CASES[case][2]
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        r, t, X = s.copy_params()
        sm, tr = sfm_amd.solve(s.uv, s.cam_idx, s.pt_idx, s.K, r, t, X,
                               options=sfm_amd.make_options(max_num_iterations=MAX_ITERATIONS))
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    return digest(sm, tr, (r, t, X))


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--check"]
    out = args[0] if args else FIXTURE
    got = {case: record(case) for case in CASES}
    again = {case: record(case) for case in CASES}
    bad = [case for case in CASES if got[case] != again[case]]
    assert not bad, f"not reproduced from run to run: {bad}"
    if "--check" in sys.argv[1:]:
        with open(out) as f:
            want = json.load(f)
        bad = [case for case in CASES if want.get(case) != got[case]]
        print("reproduced" if not bad else f"NOT reproduced: {bad}")
        sys.exit(1 if bad else 0)
    with open(out, "w") as f:
        json.dump(got, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out, {k: len(v["trace"]) for k, v in got.items()})
