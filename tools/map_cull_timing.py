"""Culling in the live loop, timed (writes profiles/map_cull_timing.txt, or
--out PATH):

* the wall time of DeviceMap.removePointsThreshold and .cullKeyFrames as the
  300-frame live run calls them (every call; the map grows to its largest at
  the last ones);
* the 300-frame live loop (bench.py's live leg: frames generated before the
  timed region, one warm-up of 25 frames) with culling off | on, alternating,
  median of three rounds: frames/s, keyframes, map points, BA share.  With
  --base LIB a library of an earlier revision (tools/mkrev.sh) runs the
  cull-off loop in the same rounds: the off column is compared against it,
  never against this build alone.

Every run is a fresh child process (this file with --child)."""
import argparse
import json
import os
import subprocess
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
N = 300


def child(cull: bool, rate: float) -> None:
    from sfm_amd.live import KeypointStream, LiveSfM
    st = KeypointStream()
    frames = [st.frame(k)[:2] for k in range(N)]
    kw = {"cull": True, "cull_kf_rate": rate} if cull else {}
    warm = LiveSfM(st, **kw)
    for k in range(25):
        warm.process(k, *frames[k])
    warm.close()
    s = LiveSfM(st, **kw)
    calls = {"removePointsThreshold": [], "cullKeyFrames": []}
    if cull:
        for name, log in calls.items():
            def timed(*a, _f=getattr(s.map, name), _log=log, **k):
                t0 = time.perf_counter()
                out = _f(*a, **k)
                _log.append(time.perf_counter() - t0)
                return out
            setattr(s.map, name, timed)
    t0 = time.perf_counter()
    for k in range(N):
        s.process(k, *frames[k])
    wall = time.perf_counter() - t0
    n_pts, n_obs, _ = s.map.size()
    out = {"cull": cull, "frames_per_s": N / wall, "keyframes": len(s.kfs), "map_points": int(n_pts),
           "live_points": int(s.map.getNPoints()) if cull else int(n_pts), "observations": int(n_obs),
           "ba_s": s.times["ba"], "mapping_s": s.times["mapping"], "lost": s.lost, "tracked": s.stats["tracked"],
           "culled_points": s.stats.get("culled_points", 0), "culled_keyframes": s.stats.get("culled_keyframes", 0),
           "calls_ms": {k: [round(x * 1e3, 4) for x in v] for k, v in calls.items()}}
    s.close()
    print("RESULT " + json.dumps(out), flush=True)


def run_child(cull: bool, rate: float, lib=None) -> dict:
    env = dict(os.environ)
    if lib:
        env["SFM_AMD_LIB"] = lib
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--rate", str(rate)] + (["--cull"] if cull else [])
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    if out.returncode != 0:
        raise RuntimeError(out.stdout + out.stderr)
    return json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def med(v):
    v = sorted(v)
    return v[len(v) // 2]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--cull", action="store_true")
    ap.add_argument("--rate", type=float, default=0.9)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--base", default=None, help="library of the parent revision (runs the cull-off loop)")
    ap.add_argument("--out", default=os.path.join(R, "profiles", "map_cull_timing.txt"))
    a = ap.parse_args()
    if a.child:
        child(a.cull, a.rate)
        return
    cols = {"off": [], "on": []}
    if a.base:
        cols["base off"] = []
    for _ in range(a.rounds):
        if a.base:
            cols["base off"].append(run_child(False, a.rate, a.base))
        cols["off"].append(run_child(False, a.rate))
        cols["on"].append(run_child(True, a.rate))
    lines = [f"live loop, {N} frames of synthetic detector output, cullKeyFrames rate {a.rate}; "
             f"{a.rounds} rounds alternating, medians (every round's frames/s in brackets)"]
    for name, runs in cols.items():
        r = runs[-1]
        lines.append(f"cull {name:8s}: {med([x['frames_per_s'] for x in runs]):7.1f} frames/s "
                     f"[{', '.join('%.1f' % x['frames_per_s'] for x in runs)}], {r['keyframes']} keyframes, "
                     f"{r['live_points']} map points ({r['map_points']} created), {r['observations']} observations, "
                     f"BA {med([x['ba_s'] for x in runs]):.4f} s, mapping {med([x['mapping_s'] for x in runs]):.4f} s, "
                     f"tracked {r['tracked']}, lost {r['lost']}, culled {r['culled_points']} points / "
                     f"{r['culled_keyframes']} keyframes")
    on = cols["on"][-1]["calls_ms"]
    for name, v in on.items():
        lines.append(f"{name}: {len(v)} calls, median {med(v):.3f} ms, max {max(v):.3f} ms, last {v[-1]:.3f} ms "
                     "(host wall time, one synchronisation each)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
