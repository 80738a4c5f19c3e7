"""Time of one sfm_two_view_init call (the synchronous C-ABI call: upload,
six launches, download, one synchronisation) on seeded two-view scenes of
n = 500 and n = 2000 matches with 30 % outliers, after warm-up, by
time.perf_counter around the call.

    python tools/two_view_bench.py [--reps 50]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import sfm_amd  # noqa: E402
from sfm_amd.mapping import F_PIX  # noqa: E402


def scene(n, seed=1, noise=0.5, outliers=0.3):
    rng = np.random.default_rng(seed)
    K = np.array([[F_PIX, 0.0, 640.0], [0.0, F_PIX, 360.0], [0.0, 0.0, 1.0]])
    uv = np.stack([rng.uniform(60, 1220, n), rng.uniform(60, 660, n)], 1)
    X = np.concatenate([(uv - K[:2, 2]) / F_PIX, np.ones((n, 1))], 1) * rng.uniform(8.0, 14.0, n)[:, None]
    th = 0.03
    R = np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]])
    Xc = X @ R.T + np.array([-0.6, 0.1, 0.15])
    p0 = uv + rng.normal(0, noise, uv.shape)
    p1 = Xc[:, :2] / Xc[:, 2:3] * F_PIX + K[:2, 2] + rng.normal(0, noise, uv.shape)
    idx = rng.choice(n, int(round(outliers * n)), replace=False)
    p1[idx] = np.stack([rng.uniform(0, 1280, len(idx)), rng.uniform(0, 720, len(idx))], 1)
    return p0.astype(np.float32), p1.astype(np.float32), K


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    out = {}
    for n in (500, 2000):
        p0, p1, K = scene(n)
        for _ in range(a.warmup):
            r = sfm_amd.two_view_init(p0, p1, K)
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            r = sfm_amd.two_view_init(p0, p1, K)
            ts.append(time.perf_counter() - t0)
        ts = np.array(ts) * 1e3
        out[f"n{n}"] = {"model": r.model, "n_kept": r.n_kept, "inliers": int(r.f_mask.sum()),
                        "ms_median": float(np.median(ts)), "ms_min": float(ts.min()), "ms_max": float(ts.max())}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
