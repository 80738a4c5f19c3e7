"""Scan guidance, timed at 1280x720 with about 6000 live map points and one
coloured box in the frame (writes profiles/guidance_timing.txt, or --out PATH):

  (1) host wall time per sfm_guidance_update on a DeviceMap (points read on
      the device), and its split into upload / kernels / download from the
      call's own HIP events;
  (2) LiveSfM.process_image frames/s with guidance on and off on the colour
      synthetic video, the two alternating inside each round.

Every round is a fresh child process (this file with --child); medians over
the rounds."""
import argparse
import json
import os
import subprocess
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
W, H = 1280, 720
LENS = (0.039530469484242, -0.149827721353905, -0.000091102042149, 0.001209830654934)  # main/main.cpp:52


def med(v):
    v = sorted(v)
    return v[len(v) // 2]


def scene(n_live: int):
    """A noisy frame with one saturated box, and points in front of it."""
    import numpy as np
    rng = np.random.default_rng(1)
    img = rng.integers(40, 140, (H, W, 3), dtype=np.uint8)
    img[200:520, 420:860] = np.clip(np.array([25, 60, 230]) + rng.integers(-12, 13, (320, 440, 3)), 0, 255)
    K = np.array([[1072.6, 0.0, 648.8], [0.0, 1067.2, 364.5], [0.0, 0.0, 1.0]])
    n = n_live + 500
    uv = np.column_stack([rng.uniform(440, 840, n), rng.uniform(220, 500, n)])
    z = rng.uniform(3.0, 5.0, n)
    X = np.column_stack([(uv[:, 0] - K[0, 2]) / K[0, 0] * z, (uv[:, 1] - K[1, 2]) / K[1, 1] * z, z])
    return np.ascontiguousarray(img), X, np.eye(3), np.zeros(3), K, np.sort(rng.choice(n, 500, replace=False))


def child(calls: int, warm: int, frames: int, n_live: int) -> None:
    import numpy as np
    from sfm_amd import DeviceMap, ScanGuidance
    from sfm_amd.camera import Camera
    from sfm_amd.live import BriskVideoStream, LiveSfM
    from sfm_amd.video import SyntheticVideo
    img, X, Rm, t, K, gone = scene(n_live)
    dm, sg = DeviceMap(), ScanGuidance(W, H)
    dm.addNewPoints(X, np.zeros((1, len(X)), np.int32), [0])
    dm.removePoints(gone)
    wall, split = [], []
    for i in range(warm + calls):
        t0 = time.perf_counter()
        res = sg.update(img, Rm, t, K, map=dm)
        dt = time.perf_counter() - t0
        if i >= warm:
            wall.append(1e3 * dt)
            split.append(sg.last_time())
    out = {"wall_ms": med(wall), "upload_ms": med([s[0] for s in split]), "kernels_ms": med([s[1] for s in split]),
           "download_ms": med([s[2] for s in split]), "n_points": res.n_points, "n_projected": res.n_projected,
           "n_accepted": res.n_accepted, "box": [float(v) for v in res.box]}
    sg.close()
    dm.close()
    st = BriskVideoStream(SyntheticVideo(W, H, speed=2.0))
    cam = Camera(st.K, LENS, (W, H))
    rgbs = [np.ascontiguousarray(np.stack([np.clip(st.video.frame(k).astype(np.int32) + o, 0, 255).astype(np.uint8)
                                           for o in (0, 9, -7)], axis=-1)) for k in range(frames)]
    fps = {False: [], True: []}
    for on in (False, True) * 3:
        live = LiveSfM(st, camera=cam, guidance=on)
        t0 = time.perf_counter()
        for k in range(frames):
            live.process_image(k, rgbs[k])
        fps[on].append(frames / (time.perf_counter() - t0))
        if on:
            out["live_guidance_calls"] = len(live.guidance_log)
            out["live_guidance_ms"] = 1e3 * live.times["guidance"] / max(1, len(live.guidance_log))
            out["live_points"] = live.guidance_log[-1].n_points if live.guidance_log else 0
        live.close()
    out["fps_off"], out["fps_on"] = med(fps[False]), med(fps[True])
    print("RESULT " + json.dumps(out), flush=True)


def run_child(a) -> dict:
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--calls", str(a.calls), "--warm", str(a.warm),
           "--frames", str(a.frames), "--points", str(a.points)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=400)
    if out.returncode != 0:
        raise RuntimeError(out.stdout + out.stderr)
    return json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--points", type=int, default=6000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(R, "profiles", "guidance_timing.txt"))
    a = ap.parse_args()
    if a.child:
        child(a.calls, a.warm, a.frames, a.points)
        return
    runs = [run_child(a) for _ in range(a.rounds)]

    def row(key, unit="ms", fmt="%.3f"):
        v = [r[key] for r in runs]
        return f"{fmt % med(v)} {unit} [{', '.join(fmt % x for x in v)}]"
    r0 = runs[-1]
    up, ke, dn = (med([r[k] for r in runs]) for k in ("upload_ms", "kernels_ms", "download_ms"))
    lines = [
        f"scan guidance, {W}x{H}, {r0['n_points']} live map points ({r0['n_projected']} projected into the frame), one box; "
        f"median of {a.calls} calls after {a.warm} warm-up in each round; {a.rounds} rounds (fresh processes), median of "
        f"the rounds (every round in brackets)",
        f"sfm_guidance_update, host wall time per call     : {row('wall_ms')}",
        f"  device time, upload of the frame (2.7 MB)       : {row('upload_ms')}",
        f"  device time, memset + 4 kernels                 : {row('kernels_ms')}",
        f"  device time, download of the result             : {row('download_ms')}",
        f"  (the wall time also holds the pinned staging copy of the frame and the host tail: hull + minAreaRect of "
        f"at most {2 * (H // 4)} points; {r0['n_accepted']} accepted pixels, box {['%.1f' % v for v in r0['box']]})",
        f"LiveSfM.process_image, {a.frames} frames of the colour synthetic video per run, guidance off / on alternating "
        f"(off, on, three times) inside each round, the median run of each:",
        f"  guidance off                                     : {row('fps_off', 'frames/s', '%.1f')}",
        f"  guidance on                                      : {row('fps_on', 'frames/s', '%.1f')}",
        f"  guidance inside the loop, per call               : {row('live_guidance_ms')}  ({r0['live_guidance_calls']} calls "
        f"per run, {r0['live_points']} map points at the end)",
    ]
    if up > ke + dn:
        lines.append(f"The upload of the frame dominates the device time ({up:.3f} of {up + ke + dn:.3f} ms). The front end "
                     f"uploads the same frame a moment earlier (sfm_frame_detect); sharing that upload is the follow-up.")
    else:
        lines.append(f"The upload of the frame is {up:.3f} of {up + ke + dn:.3f} ms of device time; the front end uploads "
                     f"the same frame a moment earlier (sfm_frame_detect), and sharing that upload is the follow-up.")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
