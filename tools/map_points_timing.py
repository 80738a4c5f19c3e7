"""Map-point creation in the live loop, host path | device path, timed (writes
profiles/map_points_timing.txt, or --out PATH):

* the 300-frame live loop (bench.py's live leg: frames generated before the
  timed region, one warm-up of 25 frames) with device_mapping off | on,
  alternating, median of three rounds: frames/s, the point-creation loop's
  wall time (times["mapping"] - times["ba"]), keyframes, map points;
* the device calls the point-creation loop makes per keyframe, counted in one
  untimed run per variant (every counted call blocks on one host
  synchronisation; the count is deterministic).

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
MATCHER_CALLS = ("match_keyframes", "match", "pair_points", "refind_points")
MAP_CALLS = ("addNewPoints", "addPointMatches", "addDescriptors", "addKeyframeRows")


def count_calls(s) -> dict:
    """Counts the device calls made inside _mapping, the BA aside."""
    import sfm_amd.live as live
    counts: dict = {}
    state = {"on": False}

    def counted(name, f):
        def g(*a, **k):
            if state["on"]:
                counts[name] = counts.get(name, 0) + 1
            return f(*a, **k)
        return g

    for obj, names in ((s.matcher, MATCHER_CALLS), (s.map, MAP_CALLS)):
        for name in names:
            setattr(obj, name, counted(name, getattr(obj, name)))
    live.triangulate_points = counted("triangulate_points", live.triangulate_points)

    def switched(f, on):
        def g(*a, **k):
            before, state["on"] = state["on"], on
            try:
                return f(*a, **k)
            finally:
                state["on"] = before
        return g

    s._mapping = switched(s._mapping, True)
    s._bundle_adjust = switched(s._bundle_adjust, False)
    return counts


def child(device: bool, count: bool) -> None:
    from sfm_amd.live import KeypointStream, LiveSfM
    st = KeypointStream()
    frames = [st.frame(k)[:2] for k in range(N)]
    warm = LiveSfM(st, device_mapping=device)
    for k in range(25):
        warm.process(k, *frames[k])
    warm.close()
    s = LiveSfM(st, device_mapping=device)
    counts = count_calls(s) if count else {}
    t0 = time.perf_counter()
    for k in range(N):
        s.process(k, *frames[k])
    wall = time.perf_counter() - t0
    n_pts, n_obs, _ = s.map.size()
    out = {"device_mapping": device, "frames_per_s": N / wall, "keyframes": len(s.kfs), "map_points": int(n_pts),
           "observations": int(n_obs), "ba_s": s.times["ba"], "mapping_s": s.times["mapping"],
           "create_s": s.times["mapping"] - s.times["ba"], "lost": s.lost, "tracked": s.stats["tracked"],
           "mappings": len(s.ba_log) - 1, "calls": counts}
    s.close()
    print("RESULT " + json.dumps(out), flush=True)


def run_child(device: bool, count: bool = False) -> dict:
    cmd = [sys.executable, os.path.abspath(__file__), "--child"] + (["--device"] if device else []) + \
        (["--count"] if count else [])
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if out.returncode != 0:
        raise RuntimeError(out.stdout + out.stderr)
    return json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def med(v):
    v = sorted(v)
    return v[len(v) // 2]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--device", action="store_true")
    ap.add_argument("--count", action="store_true")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(R, "profiles", "map_points_timing.txt"))
    a = ap.parse_args()
    if a.child:
        child(a.device, a.count)
        return
    cols = {"host": [], "device": []}
    for _ in range(a.rounds):
        cols["host"].append(run_child(False))
        cols["device"].append(run_child(True))
    lines = [f"live loop, {N} frames of synthetic detector output, map-point creation on the host (default) | on the "
             f"device (device_mapping=True); {a.rounds} rounds alternating, medians (every round's value in brackets)"]
    for name, runs in cols.items():
        r = runs[-1]
        lines.append(f"{name:6s}: {med([x['frames_per_s'] for x in runs]):7.1f} frames/s "
                     f"[{', '.join('%.1f' % x['frames_per_s'] for x in runs)}], point creation (mapping - BA) "
                     f"{med([x['create_s'] for x in runs]):.4f} s [{', '.join('%.4f' % x['create_s'] for x in runs)}], "
                     f"mapping {med([x['mapping_s'] for x in runs]):.4f} s, BA {med([x['ba_s'] for x in runs]):.4f} s, "
                     f"{r['keyframes']} keyframes, {r['map_points']} map points, {r['observations']} observations, "
                     f"tracked {r['tracked']}, lost {r['lost']}")
    for name, device in (("host", False), ("device", True)):
        r = run_child(device, count=True)
        total = sum(r["calls"].values())
        lines.append(f"{name:6s}: {total} device calls in the point-creation loop over {r['mappings']} mappings = "
                     f"{total / max(1, r['mappings']):.1f} per keyframe, one host synchronisation each ("
                     + ", ".join(f"{k} {v}" for k, v in sorted(r["calls"].items())) + ")")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
