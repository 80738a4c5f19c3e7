"""Per-row account of k_backsolve<R> from the stamped development build
(tools/chol_stamps.sh -> abvar/var_stamps.so, -DSFM_CHOL_STAMPS; another
build with SFM_AMD_LIB).  Per block row b (s_memrealtime, 100 MHz), by the
first thread of the row's slot of its row group:
  0 the slot's poll saw its block of the last awaited group, 1 after the
  barrier that hands that group to the rows, 5 (rows below a group's first)
  after the barrier that hands over the row above, 2 the FMA terms reduced
  into v, 3 after v's barrier, 4 y_b stored; 6 holds R and 7 the row's slot.
A group's arrival is seen when its last row is: stamp 0 of the awaiting
group's last slot.  The hand-off is that minus stamp 4 of the awaited group's
last row; a first row's own work runs from there to its stamp 4, an in-group
step from the row above's stamp 4 to the row's own.
  python tools/backsolve_phases.py [n] [reps]"""
import ctypes
import json
import os
import sys

import numpy as np

R = os.environ.get('GRAFT_REPO_ROOT', os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, R)
os.environ.setdefault("SFM_AMD_LIB", os.path.join(R, "abvar", "var_stamps.so"))
from sfm_amd.ba import dense_spd_solve  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 3000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
rng = np.random.default_rng(n)
B = rng.uniform(-1, 1, (n, n))
A = B + B.T
A[np.diag_indices(n)] += 2.0 * n
b = rng.standard_normal(n)
y, ms, fail = dense_spd_solve(A, b, reps=reps)
L = ctypes.CDLL(os.environ["SFM_AMD_LIB"])
L.sfm_debug_bstamps.argtypes = [ctypes.c_void_p, ctypes.c_int]
buf = (ctypes.c_ulonglong * (256 * 8))()
assert L.sfm_debug_bstamps(buf, 256 * 8) == 0
raw = np.array(buf[:], dtype=np.uint64).reshape(256, 8)
st = raw.astype(np.float64) / 100.0  # us
nb = (n + 63) // 64
rows_per_group = int(raw[nb - 1, 6])
slot = raw[:nb, 7].astype(int)
ng = (nb + rows_per_group - 1) // rows_per_group


def med(v):
    return round(float(np.median(v)), 3) if len(v) else None


# whole groups with a predecessor, away from the ends of the chain
groups = list(range(1, ng - 2))
first = [nb - 1 - g * rows_per_group for g in groups]           # a group's first (highest) row
last = [f - (rows_per_group - 1) for f in first]                # its last row: the one that sees the arrival last
seen = [st[l, 0] for l in last]
hop = [s - st[f + 1, 4] for s, f in zip(seen, first)]
own = [st[f, 4] - s for s, f in zip(seen, first)]
own_parts = {
    "arrival seen -> barrier passed": [st[f, 1] - s for s, f in zip(seen, first)],
    "barrier -> last term reduced into v": [st[f, 2] - st[f, 1] for f in first],
    "v barrier": [st[f, 3] - st[f, 2] for f in first],
    "W^T v + y store issued": [st[f, 4] - st[f, 3] for f in first],
}
below = [f - i for f in first for i in range(1, rows_per_group)]  # rows finished inside a group
step = [st[r, 4] - st[r + 1, 4] for r in below]
step_parts = {
    "row above stored -> its barrier passed": [st[r, 5] - st[r + 1, 4] for r in below],
    "barrier -> last link reduced into v": [st[r, 2] - st[r, 5] for r in below],
    "v barrier": [st[r, 3] - st[r, 2] for r in below],
    "W^T v + y store issued": [st[r, 4] - st[r, 3] for r in below],
}
per_group = [st[l, 4] - st[l + rows_per_group, 4] for l in last]
assert all(slot[f] == 0 for f in first) and all(slot[l] == rows_per_group - 1 for l in last)
out = {"n": n, "ms_factor_plus_backsolve": round(ms, 4), "fail": fail, "blocks": nb, "rows_per_group": rows_per_group,
       "groups": ng,
       "chain_us (first store -> last store)": round(float(st[0, 4] - st[nb - 1, 4]), 2),
       "hop_us_median_p90": [med(hop), round(float(np.percentile(hop, 90)), 3)],
       "own_us_median (first row of a group)": med(own),
       "own_parts_us_median": {k: med(v) for k, v in own_parts.items()},
       "in_group_step_us_median": med(step),
       "in_group_step_parts_us_median": {k: med(v) for k, v in step_parts.items()},
       "group_us_median (last store to last store)": med(per_group),
       "us_per_row": round(float(np.median(per_group)) / rows_per_group, 3)}
print(json.dumps(out, indent=1))
