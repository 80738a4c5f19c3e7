"""The camera front end, timed per 1280x720 frame (writes
profiles/frame_front_end.txt, or --out PATH):

  (a) the composed path: brisk.detect(grey) + matcher.push_frame (the host
      compacts the detector's download, re-packs and re-uploads it);
  (b) sfm_frame_detect on the same grey frame with the hand-off to the
      matcher on the device (plus the undistortion, which (a) does not do);
  (c) sfm_frame_detect on the 3-channel frame, against (c0): numpy grey
      conversion + (a) + host-side numpy undistortion of the keypoints.

Host wall time per frame, the frames rendered beforehand; every round is a
fresh child process (this file with --child) that runs the four variants one
after the other on the same frames; medians over the rounds."""
import argparse
import json
import os
import subprocess
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
VARIANTS = ["a", "b", "c0", "c"]
LENS = (0.039530469484242, -0.149827721353905, -0.000091102042149, 0.001209830654934)  # main/main.cpp:52


def np_grey(img):
    import numpy as np
    c = img.astype(np.int32)
    return ((c[..., 0] * 4899 + c[..., 1] * 9617 + c[..., 2] * 1868 + 8192) >> 14).astype(np.uint8)


def np_undistort(cam, p):
    import numpy as np
    k = np.zeros(8)
    k[:cam.d.size] = cam.d
    k1, k2, p1, p2, k3, k4, k5, k6 = k
    x0 = (p[:, 0] - cam.K[0, 2]) / cam.K[0, 0]
    y0 = (p[:, 1] - cam.K[1, 2]) / cam.K[1, 1]
    x, y = x0.copy(), y0.copy()
    for _ in range(5):
        r2 = x * x + y * y
        icd = (1 + ((k6 * r2 + k5) * r2 + k4) * r2) / (1 + ((k3 * r2 + k2) * r2 + k1) * r2)
        dx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        dy = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        x, y = (x0 - dx) * icd, (y0 - dy) * icd
    return np.stack([x * cam.Kopt[0, 0] + cam.Kopt[0, 2], y * cam.Kopt[1, 1] + cam.Kopt[1, 2]], axis=1)


def child(n_frames: int, warm: int) -> None:
    import numpy as np
    from sfm_amd import brisk
    from sfm_amd.camera import Camera, FrameFrontEnd
    from sfm_amd.matcher import FeatureMatcher
    from sfm_amd.video import SyntheticVideo
    v = SyntheticVideo(speed=2.0)
    K = np.array([[1072.606693272117800, 0.0, v.c[0]], [0.0, 1067.197515608619600, v.c[1]], [0.0, 0.0, 1.0]])
    cam = Camera(K, LENS, (v.w, v.h))
    greys = [v.frame(k) for k in range(warm + n_frames)]
    rgbs = [np.ascontiguousarray(np.stack([np.clip(g.astype(np.int32) + o, 0, 255).astype(np.uint8)
                                           for o in (0, 9, -7)], axis=-1)) for g in greys]
    out = {}
    for name in VARIANTS:
        m = FeatureMatcher()
        fe = FrameFrontEnd(cam, matcher=m)
        ts, n_kp = [], 0
        for i in range(warm + n_frames):
            t0 = time.perf_counter()
            if name == "a":
                kp, _, desc = brisk.detect(greys[i])
                m.push_frame(kp[:, :2].astype(np.float64), desc)
            elif name == "b":
                kp = fe.detect(greys[i])[0]
            elif name == "c0":
                kp, _, desc = brisk.detect(np_grey(rgbs[i]))
                pd = kp[:, :2].astype(np.float64)
                m.push_frame(np_undistort(cam, pd), desc, pd)
            else:
                kp = fe.detect(rgbs[i])[0]
            # the matcher's upload / install is stream-ordered: wait for it as the next match would
            if i >= 1:
                m.match_frames()
            dt = time.perf_counter() - t0
            if i >= warm:
                ts.append(dt)
                n_kp += len(kp)
        m.close()
        ts.sort()
        out[name] = {"ms": 1e3 * ts[len(ts) // 2], "keypoints": n_kp / n_frames}
    print("RESULT " + json.dumps(out), flush=True)


def run_child(n_frames: int, warm: int) -> dict:
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--frames", str(n_frames), "--warm", str(warm)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=400)
    if out.returncode != 0:
        raise RuntimeError(out.stdout + out.stderr)
    return json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def med(v):
    v = sorted(v)
    return v[len(v) // 2]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(R, "profiles", "frame_front_end.txt"))
    a = ap.parse_args()
    if a.child:
        child(a.frames, a.warm)
        return
    runs = [run_child(a.frames, a.warm) for _ in range(a.rounds)]
    what = {"a": "(a)  brisk.detect(grey) + matcher.push_frame",
            "b": "(b)  sfm_frame_detect, grey, hand-off on the device",
            "c0": "(c0) numpy grey + (a) + numpy undistortion",
            "c": "(c)  sfm_frame_detect, 3 channels, hand-off on the device"}
    lines = [f"camera front end, 1280x720, {a.frames} frames after {a.warm} warm-up, per-frame median of each round "
             f"(detect + hand the frame to the matcher + one match_frames as the synchronising consumer); "
             f"{a.rounds} rounds, the four variants alternating inside each; median of the rounds (every round in brackets)"]
    for name in VARIANTS:
        v = [r[name]["ms"] for r in runs]
        lines.append(f"{what[name]:58s}: {med(v):7.3f} ms/frame [{', '.join('%.3f' % x for x in v)}], "
                     f"{runs[-1][name]['keypoints']:.0f} keypoints/frame")
    lines.append(f"(b) / (a) = {med([r['b']['ms'] for r in runs]) / med([r['a']['ms'] for r in runs]):.3f}, "
                 f"(c) / (c0) = {med([r['c']['ms'] for r in runs]) / med([r['c0']['ms'] for r in runs]):.3f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
