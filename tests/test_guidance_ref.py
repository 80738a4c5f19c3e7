"""CPU: the numpy restatement of the scan guidance (tests/guidance_ref.py)
pinned to properties, and the library's host tail (sfm_min_area_rect,
sfm_guidance_default_options) bitwise against it.  Parity with OpenCV itself
is unpinned: it is not available to this project."""
import math

import numpy as np
import pytest

from tests import guidance_cases as C
from tests import guidance_ref as G

CLOUDS = C.clouds()


# ---- resize --------------------------------------------------------------------

@pytest.mark.parametrize("W,H", [(8, 8), (64, 36), (128, 72)])
def test_resize_multiple_of_four_is_the_2x2_block_mean(W, H):
    rng = np.random.default_rng(W)
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    img[0, :2], img[-1, -2:] = 0, 255
    ws, hs = G.small_size((W, H))
    assert (ws, hs) == (W // 4, H // 4)
    i = img.astype(np.int64)
    want = (i[1::4, 1::4] + i[1::4, 2::4] + i[2::4, 1::4] + i[2::4, 2::4] + 2) >> 2
    assert np.array_equal(G.resize_linear(img, ws, hs), want.astype(np.uint8))


@pytest.mark.parametrize("W,H", [(13, 9), (67, 37)])
def test_resize_ragged_is_within_one_level_of_fp64_bilinear(W, H):
    rng = np.random.default_rng(H)
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    ws, hs = G.small_size((W, H))
    assert (ws, hs) == (W // 4, H // 4)
    fx = (np.arange(ws) + 0.5) * (W / ws) - 0.5
    fy = (np.arange(hs) + 0.5) * (H / hs) - 0.5
    x0, y0 = np.floor(fx).astype(int), np.floor(fy).astype(int)
    ax, ay = (fx - x0)[None, :, None], (fy - y0)[:, None, None]
    assert x0.min() >= 0 and x0.max() + 1 < W and y0.min() >= 0 and y0.max() + 1 < H
    f = img.astype(np.float64)
    want = ((f[y0][:, x0] * (1 - ax) + f[y0][:, x0 + 1] * ax) * (1 - ay)
            + (f[y0 + 1][:, x0] * (1 - ax) + f[y0 + 1][:, x0 + 1] * ax) * ay)
    got = G.resize_linear(img, ws, hs).astype(np.float64)
    assert np.abs(got - want).max() <= 1.0
    assert np.abs(got - want).mean() < 0.35          # rounding, not a shifted tap


# ---- HSV -----------------------------------------------------------------------------

def test_hsv_primaries_secondaries_grey_black():
    # memory order B, G, R
    cases = {(0, 0, 1): 0.0, (0, 1, 1): 60.0, (0, 1, 0): 120.0, (1, 1, 0): 180.0, (1, 0, 0): 240.0, (1, 0, 1): 300.0}
    for bgr, hue in cases.items():
        h, s, v = G.bgr_to_hsv(np.array([[bgr]], np.float32))
        assert abs(float(h[0, 0]) - hue) < 1e-4 and abs(float(s[0, 0]) - 1.0) < 1e-6 and v[0, 0] == 1.0, bgr
        assert s[0, 0] < 1.0
    for level in (0.5, 1.0, 0.0):
        h, s, v = G.bgr_to_hsv(np.full((1, 1, 3), level, np.float32))
        assert h[0, 0] == 0.0 and s[0, 0] == 0.0 and v[0, 0] == np.float32(level)


def test_hsv_ranges_on_a_4096_colour_lattice():
    lv = np.arange(0, 256, 17, dtype=np.uint8)
    assert len(lv) == 16
    lattice = np.stack(np.meshgrid(lv, lv, lv, indexing="ij"), axis=-1).reshape(64, 64, 3)
    h, s, v = G.bgr_to_hsv(G.to_float(lattice))
    assert h.dtype == s.dtype == np.float32
    assert (h >= 0).all() and (h < 360).all() and (s >= 0).all() and (s < 1).all()
    bins = G.bins_of(h, s)
    assert (bins >= 0).all() and (bins[..., 0] < 60).all() and (bins[..., 1] < 50).all()


# ---- histogram, back-projection -------------------------------------------------------------

def test_histogram_sum_and_back_projection():
    W, H = 67, 37
    img = C.textured_frame(W, H, 5)
    R, t, K = C.camera_for(W, H)
    ref = G.ScanGuidanceRef()
    o = ref.calculate_mask(img, C.point_set(65, W, H, 1), R, t, K)
    inside = o["bins"][..., 0] >= 0
    assert o["mask"].sum() > 10
    assert o["frame_hist"].sum() == (o["mask"].astype(bool) & inside).sum()
    assert (o["bproj"][o["mask"].astype(bool) & inside] >= 1).all()
    assert (o["bproj"][~inside] == 0).all()
    # a pixel outside either range is dropped (bin_index itself)
    assert G.bin_index(np.array([-0.1, 0.0, 359.9, 360.0, np.nan], np.float32), 60, 0.0, 360.0).tolist() == [-1, 0, 59, -1, -1]
    b = G.bins_of(np.array([[10.0, 400.0]], np.float32), np.array([[0.5, 0.5]], np.float32))
    assert b.tolist() == [[[1, 25], [-1, -1]]]
    m = np.ones((1, 2), np.uint8)
    assert G.calc_hist(b, m).sum() == 1 and G.back_project(b, G.calc_hist(b, m)).tolist() == [[1.0, 0.0]]


def test_ema_state_and_replacement():
    W, H = 64, 36
    R, t, K = C.camera_for(W, H)
    X = C.point_set(65, W, H, 3)
    frames = [C.textured_frame(W, H, s) for s in (1, 2, 3)]
    rep, ema = G.ScanGuidanceRef(), G.ScanGuidanceRef(ema=1)
    prev = None
    for i, f in enumerate(frames):
        a, b = rep.calculate_mask(f, X, R, t, K), ema.calculate_mask(f, X, R, t, K)
        assert np.array_equal(a["hist"], a["frame_hist"])          # _frameCount stays 0: replaced
        if i == 0:
            assert np.array_equal(b["hist"], b["frame_hist"])      # the first update replaces
        else:
            want = b["frame_hist"] * np.float32(0.9) + prev * np.float32(1.0 - 0.9)
            assert np.array_equal(b["hist"], want.astype(np.float32)) and b["hist"].dtype == np.float32
        prev = b["hist"]


# ---- hull, fill, area ---------------------------------------------------------------------------

def _brute_hull_edges(p):
    """Directed hull edges a -> b (interior on the left, y up) of unique points:
    every other point strictly left of a -> b, or on the segment itself."""
    out = []
    for a in range(len(p)):
        d = p - p[a]                                                   # d[b] = p[b] - p[a]
        cross = d[:, None, 0] * d[None, :, 1] - d[:, None, 1] * d[None, :, 0]   # [b][c]
        dot = d[:, None, 0] * d[None, :, 0] + d[:, None, 1] * d[None, :, 1]
        between = (cross == 0) & (dot >= 0) & (dot <= (d ** 2).sum(-1)[:, None])
        ok = ((cross > 0) | between).all(axis=1)
        ok[a] = False
        out += [(a, int(b)) for b in np.flatnonzero(ok)]
    return out


@pytest.mark.parametrize("name", ["one", "two", "collinear3", "n65", "n1000", "duplicates", "horizontal", "diagonal",
                                  "square", "triangle"])
def test_hull_and_fill_equal_brute_force(name):
    pts = CLOUDS[name]
    hull = G.convex_hull(pts)
    p = np.unique(pts, axis=0)
    if len(p) == 1:
        assert np.array_equal(hull, p)
    else:
        edges = _brute_hull_edges(p)
        verts = sorted({a for a, _ in edges})
        assert sorted(map(tuple, hull.tolist())) == [tuple(p[a]) for a in verts]
        # the order: from the smallest point, clockwise (y up) = against the brute-force edges
        assert tuple(hull[0]) == tuple(p[0])
        nxt = {tuple(p[b]): tuple(p[a]) for a, b in edges}
        for a, b in zip(hull.tolist(), np.roll(hull, -1, axis=0).tolist()):
            assert nxt[tuple(a)] == tuple(b)
    # the fill: inside every half-plane of the hull (and its bounding box)
    ws, hs = int(pts[:, 0].max()) + 3, int(pts[:, 1].max()) + 3
    y, x = np.mgrid[0:hs, 0:ws]
    a, b = hull, np.roll(hull, -1, axis=0)
    inside = (x >= hull[:, 0].min()) & (x <= hull[:, 0].max()) & (y >= hull[:, 1].min()) & (y <= hull[:, 1].max())
    for (ax, ay), (bx, by) in zip(a.tolist(), b.tolist()):
        inside &= (bx - ax) * (y - ay) - (by - ay) * (x - ax) <= 0       # clockwise: interior on the right
    assert np.array_equal(G.fill_hull(hull, ws, hs), inside.astype(np.uint8))
    assert G.fill_hull(hull, ws, hs)[pts[:, 1], pts[:, 0]].all()
    # clipped by a smaller image
    assert np.array_equal(G.fill_hull(hull, max(ws - 5, 1), max(hs - 4, 1)), inside[:max(hs - 4, 1), :max(ws - 5, 1)])
    # area: shoelace = Pick's count for a lattice polygon is not needed; a direct fp64 check
    h = hull.astype(np.float64)
    if len(h) >= 3:
        want = 0.5 * abs(np.sum(h[:, 0] * np.roll(h[:, 1], -1) - np.roll(h[:, 0], -1) * h[:, 1]))
        assert G.contour_area(hull) == want and (2 * want) == int(2 * want)
    else:
        assert G.contour_area(hull) == 0.0


def test_small_points_round_half_to_even():
    assert G.small_points(np.array([[2, 6], [1279, 719], [10, 14]])).tolist() == [[0, 2], [320, 180], [2, 4]]


# ---- minAreaRect ---------------------------------------------------------------------------------

def _brute_min_area(hull):
    """fp64: the smallest rectangle with a side along a hull edge -> (area, perimeter)."""
    h = hull.astype(np.float64)
    best = None
    for a, b in zip(h, np.roll(h, -1, axis=0)):
        e = (b - a) / np.linalg.norm(b - a)
        n = np.array([-e[1], e[0]])
        w, ht = np.ptp(h @ e), np.ptp(h @ n)
        if best is None or w * ht < best[0]:
            best = (w * ht, 2 * (w + ht))
    return best


@pytest.mark.parametrize("name", sorted(CLOUDS))
def test_min_area_rect_contains_the_points_and_is_minimal(name):
    pts = CLOUDS[name]
    box = G.min_area_rect(pts)
    assert box.dtype == np.float32 and np.isfinite(box).all()
    slack = 1e-3           # float32 on coordinates below 512: a few hundred ulps of 3e-5 px
    cx, cy, w, h, ang = (float(v) for v in box)
    a = math.radians(ang)
    e, n = np.array([math.cos(a), math.sin(a)]), np.array([-math.sin(a), math.cos(a)])
    rel = pts.astype(np.float64) - [cx, cy]
    assert (np.abs(rel @ e) <= w / 2 + slack).all() and (np.abs(rel @ n) <= h / 2 + slack).all()
    corners = G.rect_corners(box)
    assert np.allclose(corners.mean(axis=0), [cx, cy])
    hull = G.convex_hull(pts)
    if len(hull) >= 3:
        area, perimeter = _brute_min_area(hull)
        assert w * h <= area + slack * perimeter
    elif len(hull) == 2:
        assert h == 0 and abs(w - np.linalg.norm(hull[1] - hull[0])) < 1e-4
    else:
        assert (w, h) == (0.0, 0.0) and (cx, cy) == tuple(pts[0])
    assert np.array_equal(G.min_area_rect(np.zeros((0, 2), np.int64)), np.zeros(5, np.float32))
    # the hull of the rows' extent points is the hull of the set: the same box, bitwise
    acc = np.zeros((int(pts[:, 1].max()) + 1, int(pts[:, 0].max()) + 1), bool)
    acc[pts[:, 1], pts[:, 0]] = True
    assert np.array_equal(G.min_area_rect(G.extent_points(G.row_extents(acc))).view(np.uint32), box.view(np.uint32))


# ---- the flat two-colour frame ---------------------------------------------------------------------

def test_flat_two_colour_frame():
    img, X, R, t, K = C.flat_case()
    o = G.calculate_mask(img, X, R, t, K)
    sm = o["small_pixels"]
    assert sorted(set(map(tuple, sm.tolist()))) == [(x, y) for x in range(12, 23) for y in range(5, 11)]
    assert o["n_projected"] == len(X) and o["n_hull"] == 4 and o["area"] == 10.0 * 5.0
    assert o["mask"].sum() == 11 * 6 and o["mask"][5:11, 12:23].all()
    want = np.zeros((18, 32), bool)
    want[4:12, 10:24] = True                                   # the block's small pixels, 112 of them
    got = np.zeros((18, 32), bool)
    got[o["accepted"][:, 1], o["accepted"][:, 0]] = True
    assert np.array_equal(got, want) and o["n_accepted"] == 112
    assert np.array_equal(o["box"][:2], [66.0, 30.0])
    assert sorted(o["box"][2:4].tolist()) == [28.0, 52.0]
    assert np.allclose(o["centroid"], X.mean(axis=0), rtol=0, atol=1e-13)
    # no points: NaN centroid, empty mask, zero box
    e = G.calculate_mask(img, np.zeros((0, 3)), R, t, K)
    assert np.isnan(e["centroid"]).all() and e["mask"].sum() == 0 and e["n_accepted"] == 0
    assert np.array_equal(e["box"], np.zeros(5, np.float32))


def test_restatement_is_fast_enough_at_full_size():
    import time
    W, H = 1280, 720
    img = C.textured_frame(W, H, 9)
    R, t, K = C.camera_for(W, H)
    X = C.point_set(6000, W, H, 4)
    t0 = time.perf_counter()
    o = G.calculate_mask(img, X, R, t, K)
    assert time.perf_counter() - t0 < 1.0
    assert o["n_projected"] > 5000 and o["n_accepted"] > 100


# ---- the library's host tail --------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(CLOUDS))
def test_library_min_area_rect_equals_the_restatement_bitwise(name):
    import sfm_amd
    pts = CLOUDS[name]
    got = sfm_amd.min_area_rect(pts)
    want = G.min_area_rect(pts)
    assert got.dtype == np.float32
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (got, want)
    # the order of the input does not matter
    rng = np.random.default_rng(1)
    assert np.array_equal(sfm_amd.min_area_rect(rng.permutation(pts)).view(np.uint32), want.view(np.uint32))


def test_library_min_area_rect_empty_and_bad_arguments():
    import sfm_amd
    from sfm_amd._ffi import ptr
    assert np.array_equal(sfm_amd.min_area_rect(np.zeros((0, 2), np.int32)), np.zeros(5, np.float32))
    box = np.zeros(5, np.float32)
    p = np.zeros((2, 2), np.int32)
    assert sfm_amd.lib().sfm_min_area_rect(2, None, ptr(box)) == -22
    assert sfm_amd.lib().sfm_min_area_rect(2, ptr(p), None) == -22
    assert sfm_amd.lib().sfm_min_area_rect(-1, ptr(p), ptr(box)) == -22


def test_library_default_options_are_the_references_constants():
    from sfm_amd._ffi import default_guidance_options
    o = default_guidance_options()
    assert (o.h_bins, o.s_bins, o.threshold, o.alpha, o.ema) == (G.H_BINS, G.S_BINS, G.THRESHOLD, G.ALPHA, 0)
    assert (o.h_bins, o.s_bins, o.threshold, o.alpha) == (60, 50, 0.01, 0.9)
