"""Map-point creation in the live loop, host path | device path | device path
with all older keyframes in one call, timed (writes
profiles/map_points_timing.txt, or --out PATH):

* the 300-frame live loop (bench.py's live leg: frames generated before the
  timed region, one warm-up of 25 frames) with device_mapping off | on | on
  with batch_pairs, alternating, median of three rounds: frames/s, the
  point-creation loop's wall time (times["mapping"] - times["ba"]),
  keyframes, map points;
* the device calls the point-creation loop makes per keyframe, counted in one
  untimed run per variant (every counted call blocks on one host
  synchronisation; the count is deterministic); for the batched variant also
  every call's pair count B, its device time (the handle's HIP events) and
  the pairs computed behind the first productive one, which are discarded.

With --ab PARENT_LIB the device and the batched variant are run on two
builds of the library instead, PARENT_LIB and the tree's own, alternating
(writes profiles/pair_points_single_ab.txt, or --out PATH): every round's
frames/s and point-creation time, the medians, and per variant whether the
tree's median point-creation time lies inside the min-max range of
PARENT_LIB's rounds (or below it).

Every run is a fresh child process (this file with --child; a library other
than the tree's own is selected with SFM_AMD_LIB in the child's environment)."""
import argparse
import json
import os
import subprocess
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
N = 300
MATCHER_CALLS = ("match_keyframes", "match", "pair_points", "pair_points_first", "refind_points")
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


def batch_stats(s) -> list:
    """One record per pair_points_first call: B, rows, first, device ms."""
    recs = []
    f = s.matcher.pair_points_first

    def g(slots0, idx0_list, slot1, idx1, *a, **k):
        out = f(slots0, idx0_list, slot1, idx1, *a, **k)
        knn_ms, total_ms = s.matcher.last_time_ms()
        recs.append({"B": len(slots0), "rows0": int(sum(len(x) for x in idx0_list)), "rows1": len(idx1),
                     "first": int(out[0]), "knn_ms": knn_ms, "total_ms": total_ms})
        return out
    s.matcher.pair_points_first = g
    return recs


def child(device: bool, batch: bool, count: bool) -> None:
    from sfm_amd.live import KeypointStream, LiveSfM
    st = KeypointStream()
    frames = [st.frame(k)[:2] for k in range(N)]
    warm = LiveSfM(st, device_mapping=device, batch_pairs=batch)
    for k in range(25):
        warm.process(k, *frames[k])
    warm.close()
    s = LiveSfM(st, device_mapping=device, batch_pairs=batch)
    batches = batch_stats(s) if count and batch else []
    counts = count_calls(s) if count else {}
    t0 = time.perf_counter()
    for k in range(N):
        s.process(k, *frames[k])
    wall = time.perf_counter() - t0
    n_pts, n_obs, _ = s.map.size()
    out = {"device_mapping": device, "batch_pairs": batch, "batches": batches, "frames_per_s": N / wall, "keyframes": len(s.kfs), "map_points": int(n_pts),
           "observations": int(n_obs), "ba_s": s.times["ba"], "mapping_s": s.times["mapping"],
           "create_s": s.times["mapping"] - s.times["ba"], "lost": s.lost, "tracked": s.stats["tracked"],
           "mappings": len(s.ba_log) - 1, "calls": counts}
    s.close()
    print("RESULT " + json.dumps(out), flush=True)


def run_child(device: bool, batch: bool = False, count: bool = False, lib: str | None = None) -> dict:
    cmd = [sys.executable, os.path.abspath(__file__), "--child"] + (["--device"] if device else []) + \
        (["--batch"] if batch else []) + (["--count"] if count else [])
    env = dict(os.environ)
    env.pop("SFM_AMD_LIB", None)
    if lib:
        env["SFM_AMD_LIB"] = os.path.abspath(lib)
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env)
    if out.returncode != 0:
        raise RuntimeError(out.stdout + out.stderr)
    return json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def med(v):
    v = sorted(v)
    return v[len(v) // 2]


def ab(parent_lib: str, rounds: int, out: str) -> None:
    variants = (("device", False), ("batched", True))
    runs = {(name, who): [] for name, _ in variants for who in ("parent", "tree")}
    for _ in range(rounds):
        for name, batch in variants:
            runs[(name, "parent")].append(run_child(True, batch, lib=parent_lib))
            runs[(name, "tree")].append(run_child(True, batch))
    lines = [f"live loop, {N} frames of synthetic detector output, map-point creation on the device pair by pair "
             f"(device: device_mapping=True) and with all older keyframes in one call (batched: batch_pairs=True), on "
             f"two builds of the library: the parent commit's (parent) and this tree's (tree), in which "
             f"sfm_matcher_pair_points is the n_pairs = 1 case of sfm_matcher_pair_points_first; one session, {rounds} "
             f"rounds, parent and tree alternating, a fresh process per run; medians (every round's value in brackets)"]
    ok = True
    for name, _ in variants:
        for who in ("parent", "tree"):
            r = runs[(name, who)]
            lines.append(f"{name:7s} {who:6s}: {med([x['frames_per_s'] for x in r]):7.1f} frames/s "
                         f"[{', '.join('%.1f' % x['frames_per_s'] for x in r)}], point creation (mapping - BA) "
                         f"{med([x['create_s'] for x in r]):.4f} s [{', '.join('%.4f' % x['create_s'] for x in r)}], "
                         f"{r[-1]['keyframes']} keyframes, {r[-1]['map_points']} map points, "
                         f"{r[-1]['observations']} observations, tracked {r[-1]['tracked']}, lost {r[-1]['lost']}")
        p = [x["create_s"] for x in runs[(name, "parent")]]
        m = med([x["create_s"] for x in runs[(name, "tree")]])
        good = m <= max(p)
        ok = ok and good
        lines.append(f"{name:7s} verdict: tree median {m:.4f} s against the parent's rounds {min(p):.4f} .. {max(p):.4f} s: "
                     + ("inside the range" if min(p) <= m <= max(p) else "below the range (faster)" if good
                        else "ABOVE the range (slower)"))
    lines.append("verdict: " + ("not slower than the parent by the criterion above" if ok else "SLOWER than the parent"))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(text)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--device", action="store_true")
    ap.add_argument("--batch", action="store_true")
    ap.add_argument("--count", action="store_true")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--ab", metavar="PARENT_LIB", help="compare the tree's library with this build of an earlier one")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.child:
        child(a.device, a.batch, a.count)
        return
    if a.ab:
        ab(a.ab, a.rounds, a.out or os.path.join(R, "profiles", "pair_points_single_ab.txt"))
        return
    a.out = a.out or os.path.join(R, "profiles", "map_points_timing.txt")
    cols = {"host": [], "device": [], "batched": []}
    for _ in range(a.rounds):
        cols["host"].append(run_child(False))
        cols["device"].append(run_child(True))
        cols["batched"].append(run_child(True, True))
    lines = [f"live loop, {N} frames of synthetic detector output, map-point creation on the host (default) | on the "
             f"device (device_mapping=True) | on the device, all older keyframes in one call (device_mapping=True, "
             f"batch_pairs=True); {a.rounds} rounds alternating, medians (every round's value in brackets)"]
    for name, runs in cols.items():
        r = runs[-1]
        lines.append(f"{name:7s}: {med([x['frames_per_s'] for x in runs]):7.1f} frames/s "
                     f"[{', '.join('%.1f' % x['frames_per_s'] for x in runs)}], point creation (mapping - BA) "
                     f"{med([x['create_s'] for x in runs]):.4f} s [{', '.join('%.4f' % x['create_s'] for x in runs)}], "
                     f"mapping {med([x['mapping_s'] for x in runs]):.4f} s, BA {med([x['ba_s'] for x in runs]):.4f} s, "
                     f"{r['keyframes']} keyframes, {r['map_points']} map points, {r['observations']} observations, "
                     f"tracked {r['tracked']}, lost {r['lost']}")
    for name, device, batch in (("host", False, False), ("device", True, False), ("batched", True, True)):
        r = run_child(device, batch, count=True)
        total = sum(r["calls"].values())
        lines.append(f"{name:7s}: {total} device calls in the point-creation loop over {r['mappings']} mappings = "
                     f"{total / max(1, r['mappings']):.1f} per keyframe, one host synchronisation each ("
                     + ", ".join(f"{k} {v}" for k, v in sorted(r["calls"].items())) + ")")
        if batch:
            bs = r["batches"]
            hit = [x for x in bs if x["first"] >= 0]
            lines.append(f"batched: {len(bs)} pair_points_first calls, {len(hit)} with a productive pair; pairs per call "
                         f"median {med([x['B'] for x in bs])}, max {max(x['B'] for x in bs)}; older-keyframe rows per "
                         f"call median {med([x['rows0'] for x in bs])}; device time per call (first launch to the "
                         f"pick, HIP events) median {med([x['total_ms'] for x in bs]):.3f} ms, max "
                         f"{max(x['total_ms'] for x in bs):.3f} ms, of which the 2-NN search median "
                         f"{med([x['knn_ms'] for x in bs]):.3f} ms; pairs computed in all {sum(x['B'] for x in bs)}, of "
                         f"them behind the first productive pair (discarded, computed again by the next call) "
                         f"{sum(x['B'] - x['first'] - 1 for x in hit)}")
            lines.append("batched: (B, rows0, rows1, first, total ms) per call: "
                         + " ".join(f"({x['B']},{x['rows0']},{x['rows1']},{x['first']},{x['total_ms']:.3f})" for x in bs))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
