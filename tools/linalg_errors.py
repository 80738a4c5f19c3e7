"""The record behind tests/test_gpu_linalg.py (profiles/linalg_reference_errors.txt):
per op x family x variant the yardstick errors, the cap, the device error and
device / cap for every metric, and the outcome of the two bit identities;
then the triangulation scenes.  Needs the GPU.

    python tools/linalg_errors.py [out.txt]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import linalg_cases as C  # noqa: E402
import linalg_ref as R  # noqa: E402
from sfm_amd._ffi import LINALG_OPS, linalg_probe  # noqa: E402
from sfm_amd.mapping import triangulate_points  # noqa: E402

BATCH = {0: 700, 1: 100}


def bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def main(path):
    lines, worst = [], (0.0, "")
    for op in list(C.SVD_OPS) + ["svd12"] + list(C.LSTSQ_OPS) + ["qr6x4"]:
        for family in C.families(op):
            cap, y = C.caps(op, family), C.yardsticks(op, family)
            outs = {}
            for v in ((1,) if op == "svd12" else (0, 1) if LINALG_OPS[op][3] else (0,)):
                which = C.deal(BATCH[v])
                outs[v] = out = linalg_probe(op, v, C.problems(op, family)[which])
                err = C.metrics(op, family, out, which)
                ident = ["oracle " + ("same bits" if bits(out, C.oracle_out(op, family)[which]) else "DIFFERS")]
                if v == 1 and 0 in outs:
                    seq = linalg_probe(op, 0, C.problems(op, family)[which])   # the same batch, one problem per lane
                    ident.append("variant 0 " + ("same bits" if bits(out, seq) else "DIFFERS"))
                cols = []
                for m in cap:
                    ratio = err[m] / cap[m] if cap[m] > 0 else 0.0 if err[m] == 0 else float("inf")
                    if ratio > worst[0]:
                        worst = (ratio, f"{m} of {op} {family} variant {v}")
                    cols.append(f"{m} oracle {y['oracle'][m]:.2e} numpy {y['numpy'][m]:.2e} cap {cap[m]:.2e} "
                                f"device {err[m]:.2e} ratio {ratio:.3f}")
                lines.append(f"{op:10s} {family:14s} v{v} | " + " | ".join(cols) + " | " + ", ".join(ident))
    tri = []
    for scene in C.TRI_SCENES:
        s = C.tri_scene(scene)
        X = triangulate_points(s["cam0"], s["cam1"], s["uv0"], s["uv1"], s["P"])
        same = "same bits" if bits(X, C.tri_oracle(scene)) else "DIFFERS"
        if scene == "same_cam":
            tri.append(f"{scene:10s} (two-dimensional null space: no cap) | oracle {same}")
            continue
        (cap, y), err = C.tri_cap(scene), C.tri_error(scene, X)
        _, h, cond = C.tri_reference(scene)
        if err / cap > worst[0]:
            worst = (err / cap, f"point of scene {scene}")
        tri.append(f"{scene:10s} point/cond oracle {y['oracle']:.2e} numpy {y['numpy']:.2e} cap {cap:.2e} device "
                   f"{err:.2e} ratio {err / cap:.3f} | cond {float(cond.min()):.1e}..{float(cond.max()):.1e} |h| "
                   f"{float(np.abs(h).min()):.1e}..{float(np.abs(h).max()):.1e} worst relative error "
                   f"{float(np.max(R.rel_err(X, C.tri_reference(scene)[0]))):.2e} | oracle {same}")
    head = ["# tests/test_gpu_linalg.py: per op, family and variant (v0 one problem per lane, batch 700; v1 one per wave,",
            "# batch 100) and metric: the two fp64 yardsticks' errors against the longdouble reference, the cap (8 x the",
            "# worse yardstick + eps x condition number), the device's error and device / cap (1 is the limit); then",
            "# the bit identities (device == oracle.pnp_oracle; variant 1 == variant 0).  Metrics: tests/linalg_ref.py.",
            f"# worst ratio: {worst[0]:.3f} ({worst[1]})"]
    text = "\n".join(head + lines + ["# sfm_triangulate_points, 300 points per scene"] + tri) + "\n"
    with open(path, "w") as f:
        f.write(text)
    print("\n".join(head))
    print(f"{len(lines) + len(tri)} rows -> {path}")
    return 0 if "DIFFERS" not in text else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "linalg_reference_errors.txt")))
