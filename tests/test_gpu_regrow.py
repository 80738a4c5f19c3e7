"""GPU: buffers that grow after their first use.  Every handle and every
per-thread context keeps grow-only device and pinned buffers (dev_mem.h);
the rest of the suite mostly calls each once per size.  Here one handle, or
one thread's cached context, goes small -> larger -> small again across a
capacity floor, and every output is compared bit for bit with the same call
made on fresh state: a fresh thread for the per-thread contexts (thread_ctx
builds a new context per thread), a fresh handle otherwise.

Sizes: the smallest that cross each floor -- 1024 points (PnP, two-view),
exact sizes (triangulation, KLT), the matcher's 4096-byte scratch floor and
its frames' capacity, the map vectors' 1024 elements (whose contents must
survive: DVec::grow is the one place that keeps them), the guidance points'
doubling, the detector workspace's exact sizes, and for the bundle adjuster's
problem pool a middle problem whose every array is less than twice the outer
ones' (all reused) and one where each is more (none reused)."""
import json
import os
import threading

import numpy as np
import pytest

import sfm_amd

pytestmark = pytest.mark.gpu


def in_fresh_thread(fn, *args):
    """fn(*args) on a new thread: its per-thread contexts are new ones."""
    out = {}

    def run():
        try:
            out["value"] = fn(*args)
        except BaseException as e:  # noqa: BLE001 (re-raised below)
            out["error"] = e
    t = threading.Thread(target=run)
    t.start()
    t.join()
    if "error" in out:
        raise out["error"]
    return out["value"]


def same(a, b):
    """Bitwise equality of two results (tuples / arrays / scalars)."""
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def sequence_matches_fresh(call, cases):
    """call(case) over `cases` on this thread's context equals call(case) on a fresh thread's, case by case."""
    for k, case in enumerate(cases):
        got = call(case)
        want = in_fresh_thread(call, case)
        assert same(got, want), f"step {k} differs from a fresh context"


# ---- per-thread contexts ----

def _pnp(n):
    from tests.pnp_cases import K, scene
    X, uv, _, _ = scene(n, 77, noise=0.5, outliers=0.2)
    ok, r, t, inl = sfm_amd.solvePnPRansac(X, uv, K)
    assert ok and len(inl) > n // 2
    return bool(ok), r, t, inl


def test_pnp_regrow():
    sequence_matches_fresh(_pnp, [1000, 1100, 1000])


def _two_view_scene(n, seed=5):
    from tests.two_view_cases import F_PIX, H, K, W, _rot
    rng = np.random.default_rng(seed)
    uv = np.stack([rng.uniform(60, W - 60, n), rng.uniform(60, H - 60, n)], 1)
    rays = np.concatenate([(uv - K[:2, 2]) / F_PIX, np.ones((n, 1))], 1)
    X = rays * rng.uniform(8.0, 14.0, n)[:, None]
    R, t = _rot(np.array([0.02, -0.03, 0.015])), np.array([-0.6, 0.1, 0.15])
    Xc = X @ R.T + t
    p0 = X[:, :2] / X[:, 2:3] * F_PIX + K[:2, 2] + rng.normal(0, 0.3, (n, 2))
    p1 = Xc[:, :2] / Xc[:, 2:3] * F_PIX + K[:2, 2] + rng.normal(0, 0.3, (n, 2))
    return p0.astype(np.float32), p1.astype(np.float32), K


def _two_view(n):
    p0, p1, K = _two_view_scene(n)
    r = sfm_amd.two_view_init(p0, p1, K, K)
    assert r.ok
    return tuple(np.asarray(v) for v in vars(r).values() if isinstance(v, (np.ndarray, int, float, np.generic)))


def test_two_view_regrow():
    sequence_matches_fresh(_two_view, [1000, 1100, 1000])


def _triangulate(n):
    from sfm_amd.mapping import triangulate_points
    from tests.map_points_cases import K
    rng = np.random.default_rng(n)
    X = np.column_stack([rng.uniform(-2, 2, n), rng.uniform(-1, 1, n), rng.uniform(6, 12, n)])
    P = np.stack([K @ np.hstack([np.eye(3), np.zeros((3, 1))]), K @ np.hstack([np.eye(3), [[-0.5], [0.0], [0.0]]]),
                  K @ np.hstack([np.eye(3), [[0.4], [0.1], [0.0]]])])
    cam0, cam1 = rng.integers(0, 2, n).astype(np.int32), np.full(n, 2, np.int32)
    proj = lambda c: (lambda h: h[:, :2] / h[:, 2:3])(np.einsum("nij,nj->ni", P[c], np.hstack([X, np.ones((n, 1))])))
    got = triangulate_points(cam0, cam1, proj(cam0), proj(cam1), P)
    assert np.allclose(got, X, atol=1e-6)
    return got


def test_triangulate_regrow():
    sequence_matches_fresh(_triangulate, [64, 256, 64])


def _descs(rng, n, nbytes=64):
    return rng.integers(0, 256, (n, nbytes), dtype=np.uint8)


def _match_features(n):
    rng = np.random.default_rng(100 + n)
    d0 = _descs(rng, n)
    d1 = d0.copy()
    d1[:, 0] ^= 1
    p0 = rng.uniform(0, 1280, (n, 2))
    p1 = p0 + rng.normal(0, 5, (n, 2))
    i0, i1 = sfm_amd.CTracker().matchFeatures(p0, d0, p1, d1)
    assert len(i0) > n // 2
    return i0, i1


def test_fresh_thread_returns_the_main_threads_bits():
    """sfm_pnp_ransac, sfm_triangulate_points and sfm_match_features through a new thread's contexts."""
    for call, arg in ((_pnp, 200), (_triangulate, 100), (_match_features, 300)):
        assert same(call(arg), in_fresh_thread(call, arg)), call.__name__


# ---- handles ----

def _knn2_and_frames(fm, n):
    """knn2 on n x n descriptors, the frame-resident match of two pushed
    frames of n keypoints, and a keyframe pair stored in slots 0 and 1 with n
    rows each and matched."""
    rng = np.random.default_rng(300 + n)
    d0 = _descs(rng, n)
    d1 = d0[rng.permutation(n)].copy()
    d1[:, 3] ^= 4
    p0 = rng.uniform(0, 1280, (n, 2))
    p1 = p0 + rng.normal(0, 4, (n, 2))
    knn = fm.knn2(d0, d1)
    fm.push_frame(p0, d0)
    fm.push_frame(p1, d0 ^ np.uint8(1))
    res = fm.match_frames()
    assert len(res[0]) > n // 2
    fm.store_keyframe(0, p0, d0)
    fm.store_keyframe(1, p1, d0 ^ np.uint8(1))
    idx = np.arange(n, dtype=np.int32)
    kf = fm.match_keyframes(0, idx, 1, idx)
    assert len(kf[0]) > n // 2
    return tuple(knn) + tuple(res) + tuple(kf)


def test_matcher_regrow():
    """32, 1600, 32 rows: the scratch's 4096-byte floor, a frame's first
    capacity (max(n, 1024) * 3 / 2 = 1536 rows) and a keyframe slot's exact
    capacity (stored again with more rows) are all crossed."""
    from sfm_amd.matcher import FeatureMatcher
    with FeatureMatcher() as fm:
        for k, n in enumerate((32, 1600, 32)):
            got = _knn2_and_frames(fm, n)
            with FeatureMatcher() as fresh:
                assert same(got, _knn2_and_frames(fresh, n)), f"step {k} (n = {n})"


def _map_scene(n=1100):
    from tests.map_points_cases import K
    rng = np.random.default_rng(9)
    X = np.column_stack([rng.uniform(-3, 3, n), rng.uniform(-1.5, 1.5, n), rng.uniform(8, 12, n)])
    uv = X[:, :2] / X[:, 2:3] * np.array([K[0, 0], K[1, 1]]) + K[:2, 2]
    return X, uv, _descs(rng, n), K


def _map_fill(m, X, desc, lo, hi):
    ids = m.addNewPoints(X[lo:hi], [np.arange(lo, hi)], [0])
    assert ids.tolist() == list(range(lo, hi))
    m.addDescriptors(ids, desc[lo:hi])


def test_map_growth_keeps_contents():
    """Points, observations and descriptor rows to 1000, then to 1100: the
    same X, live flags and sfm_map_match_frame result as a map given all 1100 at once."""
    from sfm_amd.cmap import DeviceMap
    from sfm_amd.matcher import FeatureMatcher
    X, uv, desc, K = _map_scene()
    n = len(X)

    def read(m, fm):
        ids = np.arange(n)
        pm, km = m.matchFrame(fm, [0], [], np.eye(3), np.zeros(3), K, ids, 0.8, 0.0, 7.0)
        return m.getPointsAtIdx(ids), m.pointState(ids), np.asarray(m.size()), pm, km

    with FeatureMatcher() as fm:
        fm.push_frame(uv, desc ^ np.uint8(2))
        grown, whole = DeviceMap(), DeviceMap()
        try:
            _map_fill(grown, X, desc, 0, 1000)
            assert np.array_equal(grown.getPointsAtIdx(np.arange(1000)), X[:1000])
            _map_fill(grown, X, desc, 1000, n)
            _map_fill(whole, X, desc, 0, n)
            a, b = read(grown, fm), read(whole, fm)
            assert same(a, b)
            assert np.array_equal(a[0], X) and a[1][:, 4].all() and len(a[3]) > 0  # (not vacuous)
        finally:
            grown.close()
            whole.close()


def _klt_frames(seed, w=64, h=64):
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (h // 4 + 2, w // 4 + 3), dtype=np.uint8)
    big = np.repeat(np.repeat(base, 4, axis=0), 4, axis=1)
    return np.ascontiguousarray(big[:h, :w]), np.ascontiguousarray(big[:h, 1:w + 1])


def test_klt_points_regrow():
    from sfm_amd.klt import KLTTracker
    f0, f1 = _klt_frames(1)
    rng = np.random.default_rng(2)
    sets = [rng.uniform(8, 56, (n, 2)).astype(np.float32) for n in (100, 300, 100)]
    curr = rng.uniform(8, 56, (150, 2))

    def run(t, pts):
        return t.calc_flow(pts) + t.compute_optical_flow(pts.astype(np.float64), curr, with_flow=True)

    t = KLTTracker(64, 64)
    t.push_frame(f0)
    t.push_frame(f1)
    try:
        for k, pts in enumerate(sets):
            got = run(t, pts)
            fresh = KLTTracker(64, 64)
            fresh.push_frame(f0)
            fresh.push_frame(f1)
            try:
                assert same(got, run(fresh, pts)), f"step {k}"
            finally:
                fresh.close()
    finally:
        t.close()


def test_klt_colour_stage_regrow():
    """A 3-channel frame with a larger stride after one with a smaller stride."""
    import ctypes
    from sfm_amd._ffi import check, lib, ptr
    from sfm_amd.klt import KLTTracker
    rng = np.random.default_rng(3)
    w = h = 64
    rgb = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(2)]

    def push(t, img, stride):
        rows = np.zeros((h, stride), np.uint8)
        rows[:, :3 * w] = img.reshape(h, 3 * w)
        check(lib().sfm_klt_push_frame_rgb(t._h, ptr(rows), ctypes.c_int32(stride)), "sfm_klt_push_frame_rgb")

    t, fresh, first = KLTTracker(w, h), KLTTracker(w, h), KLTTracker(w, h)
    try:
        push(t, rgb[0], 3 * w)
        push(t, rgb[1], 3 * w + 40)
        fresh.push_frame_rgb(rgb[1])
        for level in range(t.num_levels):
            assert same(t.level(1, level), fresh.level(1, level)), level
        first.push_frame_rgb(rgb[0])
        assert same(t.level(0, 0), first.level(1, 0))
    finally:
        t.close()
        fresh.close()
        first.close()


def test_guidance_points_regrow():
    from sfm_amd.guidance import ScanGuidance
    from tests.guidance_cases import camera_for, point_set, textured_frame
    W, H = 128, 96
    R, t, K = camera_for(W, H)
    img = textured_frame(W, H, 4)

    def read(g, pts):
        f = g.update(img, R, t, K, points=pts)
        p = g.planes()
        return tuple(np.asarray(v) for v in vars(f).values()) + tuple(np.asarray(p[k]) for k in sorted(p))

    g = ScanGuidance(W, H, ema=0)   # no blend with the previous update: each one stands alone
    try:
        for k, n in enumerate((1000, 1100)):
            pts = point_set(n, W, H, 6)
            got = read(g, pts)
            fresh = ScanGuidance(W, H, ema=0)
            try:
                assert same(got, read(fresh, pts)), f"step {k}"
            finally:
                fresh.close()
    finally:
        g.close()


@pytest.mark.parametrize("w,h", [(8, 8), (96, 64)])
def test_brisk_workspace_regrow(w, h):
    """The detector's workspace is one per device for the process: the first
    frame again after one twice as wide gives the first frame's bits, and the
    wide frame's result does not depend on what the workspace held before."""
    from sfm_amd import brisk
    rng = np.random.default_rng(w)
    base = rng.integers(0, 256, (h // 4 + 1, w // 2 + 1), dtype=np.uint8)
    wide = np.ascontiguousarray(np.repeat(np.repeat(base, 4, axis=0), 4, axis=1)[:h, :2 * w])
    small = np.ascontiguousarray(wide[:, :w])
    det = lambda im: tuple(x for x in brisk.detect(im, threshold=20, octaves=2) if x is not None)
    first, big, again, big_again = det(small), det(wide), det(small), det(wide)
    assert same(first, again) and same(big, big_again)
    if w >= 64:
        assert len(big[0]) > 0


# ---- the bundle adjuster's problem pool ----

def _ba_scenes(seq):
    """(a): cameras, points and views of the middle problem about 1.4 times the
    outer ones' -- 12 -> 17 cameras (78 -> 153 camera blocks), 400 -> 470 points,
    4 -> 5 views (1600 -> 2350 observations, 6 -> 10 pairs per point: 2400 ->
    4700) -- so every array of the third problem is smaller than the second's
    and more than half of it: each buffer is a larger one of the pool, with
    the second problem's contents.  (b): every ratio above 2 (and past 64
    cameras), so nothing is reused and the trim frees the lot."""
    from sfm_amd import scene
    small = (12, 400, 4)
    mid = {"a": (17, 470, 5), "b": (70, 1500, 6)}[seq]
    return [scene.generate(c, p, views=v) for c, p, v in (small, mid, small)]


def _summary_and_trace(sm, tr):
    """The summary without its wall times, and the trace, as arrays (compared as bits: NaNs included)."""
    keep = [k for k in sm.as_dict() if not k.endswith("_time_s")]
    return (np.array([float(getattr(sm, k)) for k in keep]),
            np.array([[float(it[k]) for k in sorted(it)] for it in tr]))


def _two_iterations():
    opts = sfm_amd.default_options()
    opts.max_num_iterations = 2
    return opts


def _ba_resident(ba, s):
    """set_problem, then evaluate() (its records come from the pool after the
    set-up), a two-iteration solve, and the parameters."""
    ba.set_problem(s.uv, s.cam_idx, s.pt_idx, s.K, s.rot, s.t, s.X)
    cost, res, jac = ba.evaluate()
    sm, tr = ba.solve(_two_iterations())
    assert sm.num_iterations > 0 and len(tr) > 1 and np.isfinite(res).all() and np.abs(jac).max() > 0
    return (cost, res, jac) + _summary_and_trace(sm, tr) + tuple(ba.parameters())


@pytest.mark.parametrize("seq", ["a", "b"])
def test_ba_problem_pool_regrow(seq):
    with sfm_amd.BundleAdjuster() as ba:
        for k, s in enumerate(_ba_scenes(seq)):
            got = _ba_resident(ba, s)
            with sfm_amd.BundleAdjuster() as fresh:
                assert same(got, _ba_resident(fresh, s)), f"step {k} differs from a fresh handle"


def _ba_one_shot(s):
    r, t, X = s.copy_params()
    sm, tr = sfm_amd.solve(s.uv, s.cam_idx, s.pt_idx, s.K, r, t, X, _two_iterations())
    assert sm.num_iterations > 0 and len(tr) > 1
    return _summary_and_trace(sm, tr) + (r, t, X)


def test_ba_one_shot_regrow():
    """sfm_ba_solve keeps one handle per thread: three problems through one thread's, each against a new thread's."""
    scenes = _ba_scenes("a")
    got = in_fresh_thread(lambda: [_ba_one_shot(s) for s in scenes])
    for k, s in enumerate(scenes):
        assert same(got[k], in_fresh_thread(_ba_one_shot, s)), f"step {k} differs from a fresh thread's handle"


# ---- the dense solve's one-shot problem (built from owners now): the parent commit's bits ----

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dense_solve_parent.json")


def test_dense_solve_bits_of_the_parent_commit():
    from tests.golden.make_dense_solve_parent import record
    with open(GOLDEN) as f:
        want = json.load(f)
    assert record() == want
