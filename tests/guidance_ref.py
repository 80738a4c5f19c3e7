"""numpy restatement of the reference's scan guidance
(CScanGuidance::calculateMask, CScanGuidance.cpp:39-105): the object mask
from the projected map points, the masked hue/saturation histogram, its
back-projection, the thresholded pixel set and cv::minAreaRect of it.

OpenCV is not available to this project: every OpenCV call is restated here
from OpenCV 3.0 and the library is held bit for bit against this file; parity
with OpenCV itself is unpinned.  One function per step, each
keeping the operation order and the number formats of the specification.

Conventions fixed by this restatement where the reference leaves them open:
  * GeometryUtils::projectPoints is restated from its call site: fp64,
    c = R X + t summed left to right, u = c0 / c2 * fx + cx, cvRound.
  * convex_hull returns the strict hull (no collinear vertex), starting at
    the lexicographically smallest (x, y) point and running clockwise in a
    frame whose y axis points up (cv::convexHull(.., clockwise = true)).
  * the fill is the set of pixels inside or on the closed hull (OpenCV's
    rasteriser also sets the Bresenham pixels of every edge: not reproduced).
  * HSV: s = diff / float(double(|v|) + double(FLT_EPSILON)),
    d = float(60. / double(float(diff + FLT_EPSILON))).
"""
from __future__ import annotations

import math

import numpy as np

SCALE = 0.25
H_BINS, S_BINS = 60, 50
H_RANGE, S_RANGE = (0.0, 360.0), (0.0, 1.0)
THRESHOLD = 0.01
ALPHA = 0.9
f32 = np.float32
EPS = f32(np.finfo(np.float32).eps)   # FLT_EPSILON


# ---- 1. centroid ---------------------------------------------------------------

def centroid(pts3d):
    """updateCentroid: the fp64 sum in order times 1.0 / n (NaN for n = 0)."""
    X = np.asarray(pts3d, np.float64).reshape(-1, 3)
    s = np.zeros(3)
    for c in range(3):
        s[c] = np.cumsum(X[:, c])[-1] if len(X) else 0.0   # (cumsum adds in order)
    with np.errstate(divide="ignore", invalid="ignore"):
        return s * (np.float64(1.0) / np.float64(len(X)))


# ---- 2. projection to integer pixels ---------------------------------------------

def project_points(pts3d, R, t, K, size):
    """-> the kept (u, v) integer pixels [m][2] (int64), in input order."""
    X = np.asarray(pts3d, np.float64).reshape(-1, 3)
    R = np.asarray(R, np.float64).reshape(3, 3)
    t = np.asarray(t, np.float64).reshape(3)
    K = np.asarray(K, np.float64).reshape(3, 3)
    W, H = size
    x0, x1, x2 = X[:, 0], X[:, 1], X[:, 2]
    with np.errstate(all="ignore"):
        c0 = R[0, 0] * x0 + R[0, 1] * x1 + R[0, 2] * x2 + t[0]
        c1 = R[1, 0] * x0 + R[1, 1] * x1 + R[1, 2] * x2 + t[1]
        c2 = R[2, 0] * x0 + R[2, 1] * x1 + R[2, 2] * x2 + t[2]
        u = np.rint(c0 / c2 * K[0, 0] + K[0, 2])
        v = np.rint(c1 / c2 * K[1, 1] + K[1, 2])
        keep = (c2 > 0) & (u >= 0) & (u < W) & (v >= 0) & (v < H)
    return np.stack([u[keep], v[keep]], axis=1).astype(np.int64).reshape(-1, 2)


# ---- 3. small coordinates ----------------------------------------------------------

def small_points(px):
    """pts2dM *= 0.25 on an int matrix: rint(u * 0.25), half to even."""
    return np.rint(np.asarray(px, np.int64).astype(np.float64) * SCALE).astype(np.int64).reshape(-1, 2)


# ---- 4. hull, fill, area -------------------------------------------------------------

def convex_hull(pts):
    """Strict convex hull of integer points -> [k][2] int64 (see the module
    docstring for the order); k = 0, 1 or 2 for empty / degenerate input."""
    p = np.unique(np.asarray(pts, np.int64).reshape(-1, 2), axis=0)   # sorted by x, then y
    if len(p) <= 1:
        return p.copy()
    # only a column's extreme points can be hull vertices
    first = np.flatnonzero(np.r_[True, p[1:, 0] != p[:-1, 0]])
    last = np.flatnonzero(np.r_[p[1:, 0] != p[:-1, 0], True])
    q = [tuple(r) for r in p[np.unique(np.r_[first, last])].tolist()]

    def chain(seq):
        out = []
        for c in seq:
            while len(out) >= 2:
                a, b = out[-2], out[-1]
                if (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0]) <= 0:
                    out.pop()
                else:
                    break
            out.append(c)
        return out
    lower, upper = chain(q), chain(q[::-1])
    ccw = lower[:-1] + upper[:-1]
    return np.array([ccw[0]] + ccw[:0:-1], np.int64).reshape(-1, 2)


def contour_area(hull):
    """contourArea: the shoelace sum in fp64 (exact here), absolute value."""
    h = np.asarray(hull, np.float64).reshape(-1, 2)
    if len(h) < 3:
        return 0.0
    a = 0.0
    prev = h[-1]
    for cur in h:
        a += prev[0] * cur[1] - prev[1] * cur[0]
        prev = cur
    return abs(a * 0.5)


def fill_hull(hull, ws, hs):
    """The pixels of a ws x hs image inside or on the closed hull -> uint8
    [hs][ws]; exact integer arithmetic (per-row interval of the hull)."""
    mask = np.zeros((hs, ws), np.uint8)
    h = np.asarray(hull, np.int64).reshape(-1, 2)
    if len(h) == 0:
        return mask
    a, b = h, np.roll(h, -1, axis=0)
    y = np.arange(hs, dtype=np.int64)[:, None]
    ax, ay, bx, by = a[:, 0][None], a[:, 1][None], b[:, 0][None], b[:, 1][None]
    span = (np.minimum(ay, by) <= y) & (y <= np.maximum(ay, by))
    dy = by - ay
    flat = dy == 0
    den = np.where(flat, 1, np.abs(dy))
    num = (ax * dy + (bx - ax) * (y - ay)) * np.where(dy < 0, -1, 1)   # x = num / den
    lo = np.where(flat, np.minimum(ax, bx), -((-num) // den))          # ceil
    hi = np.where(flat, np.maximum(ax, bx), num // den)                # floor
    big = np.int64(1) << 40
    lo = np.where(span, lo, big).min(axis=1)
    hi = np.where(span, hi, -big).max(axis=1)
    x = np.arange(ws, dtype=np.int64)[None]
    mask[(x >= lo[:, None]) & (x <= hi[:, None])] = 1
    return mask


# ---- 5. resize ------------------------------------------------------------------------

def _resize_taps(n_src, n_dst):
    """-> (index of tap 0, index of tap 1, coefficient 0, coefficient 1)."""
    scale = np.float64(n_src) / np.float64(n_dst)
    d = np.arange(n_dst, dtype=np.float64)
    f = ((d + 0.5) * scale - 0.5).astype(f32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(f32)).astype(f32)
    low, high = s < 0, s >= n_src - 1
    f = np.where(low | high, f32(0), f).astype(f32)
    s = np.where(low, 0, np.where(high, n_src - 1, s))
    c1 = np.rint(f * f32(2048)).astype(np.int64)
    c0 = np.rint((f32(1) - f) * f32(2048)).astype(np.int64)
    return s, np.minimum(s + 1, n_src - 1), c0, c1


def resize_linear(img, ws, hs):
    """cv::resize(.., INTER_LINEAR) of an 8-bit image, OpenCV 3.0's fixed
    point form: uint8 [H][W][C] -> [hs][ws][C]."""
    im = np.asarray(img, np.uint8).astype(np.int64)
    H, W = im.shape[:2]
    x0, x1, a0, a1 = _resize_taps(W, ws)
    y0, y1, b0, b1 = _resize_taps(H, hs)
    sh = (1, ws) + (1,) * (im.ndim - 2)
    rows = im[:, x0] * a0.reshape(sh) + im[:, x1] * a1.reshape(sh)     # horizontal pass, int
    sv = (hs, 1) + (1,) * (im.ndim - 2)
    S0, S1 = rows[y0], rows[y1]
    out = (((b0.reshape(sv) * (S0 >> 4)) >> 16) + ((b1.reshape(sv) * (S1 >> 4)) >> 16) + 2) >> 2
    return np.clip(out, 0, 255).astype(np.uint8)


def small_size(size):
    W, H = size
    return int(W * SCALE), int(H * SCALE)


# ---- 6 / 7. float conversion and HSV ------------------------------------------------------

def to_float(small):
    return (np.asarray(small, np.uint8).astype(f32) * f32(1.0 / 255.0)).astype(f32)


def bgr_to_hsv(fimg):
    """cvtColor(.., CV_BGR2HSV) on float: memory channel 0 is B.  -> (h, s, v)."""
    fimg = np.asarray(fimg, f32)
    b, g, r = fimg[..., 0], fimg[..., 1], fimg[..., 2]
    v = np.maximum(np.maximum(r, g), b)
    vmin = np.minimum(np.minimum(r, g), b)
    diff = (v - vmin).astype(f32)
    s = (diff / (np.abs(v).astype(np.float64) + np.float64(EPS)).astype(f32)).astype(f32)
    d = (np.float64(60.0) / (diff + EPS).astype(f32).astype(np.float64)).astype(f32)
    h_r = ((g - b).astype(f32) * d).astype(f32)
    h_g = (((b - r).astype(f32) * d).astype(f32) + f32(120)).astype(f32)
    h_b = (((r - g).astype(f32) * d).astype(f32) + f32(240)).astype(f32)
    h = np.where(v == r, h_r, np.where(v == g, h_g, h_b)).astype(f32)
    h = np.where(h < 0, (h + f32(360)).astype(f32), h).astype(f32)
    return h, s, v


# ---- 8. histogram ---------------------------------------------------------------------------

def bin_index(values, bins, lo, hi):
    """calcHist's uniform bin: cvFloor(double(value) * a + b); -1 = outside."""
    a = np.float64(bins) / (np.float64(hi) - np.float64(lo))
    b = -(a * np.float64(lo))
    idx = np.floor(np.asarray(values, f32).astype(np.float64) * a + b)
    return np.where((idx >= 0) & (idx < bins), idx, -1).astype(np.int64)


def bins_of(h, s, h_bins=H_BINS, s_bins=S_BINS):
    """-> int16 [hs][ws][2]; a pixel with either bin outside is (-1, -1)."""
    hb = bin_index(h, h_bins, *H_RANGE)
    sb = bin_index(s, s_bins, *S_RANGE)
    out = (hb < 0) | (sb < 0)
    return np.stack([np.where(out, -1, hb), np.where(out, -1, sb)], axis=-1).astype(np.int16)


def calc_hist(bins, mask, h_bins=H_BINS, s_bins=S_BINS):
    """Counts (int) of the masked, in-range pixels, stored as float32."""
    use = (mask != 0) & (bins[..., 0] >= 0)
    flat = bins[..., 0][use].astype(np.int64) * s_bins + bins[..., 1][use].astype(np.int64)
    return np.bincount(flat, minlength=h_bins * s_bins).astype(f32).reshape(h_bins, s_bins)


# ---- 9. histogram state -----------------------------------------------------------------------

def blend(hist, old, alpha=ALPHA):
    """_hist = alpha * hist + (1 - alpha) * _hist, float work type."""
    a, b = f32(alpha), f32(np.float64(1.0) - np.float64(alpha))
    return ((hist.astype(f32) * a).astype(f32) + (old.astype(f32) * b).astype(f32)).astype(f32)


# ---- 10 / 11. back-projection, threshold ----------------------------------------------------------

def back_project(bins, hist):
    ok = bins[..., 0] >= 0
    hb = np.where(ok, bins[..., 0], 0).astype(np.int64)
    sb = np.where(ok, bins[..., 1], 0).astype(np.int64)
    return np.where(ok, hist[hb, sb], f32(0)).astype(f32)


def accept(bproj, area, threshold=THRESHOLD):
    with np.errstate(divide="ignore", invalid="ignore"):
        return bproj.astype(np.float64) / np.float64(area) > np.float64(threshold)


def row_extents(acc):
    """Per row (min x, max x) of the accepted pixels; (ws, -1) = empty row."""
    hs, ws = acc.shape
    x = np.arange(ws, dtype=np.int64)[None]
    lo = np.where(acc, x, ws).min(axis=1)
    hi = np.where(acc, x, -1).max(axis=1)
    return np.stack([lo, hi], axis=1).astype(np.int32)


# ---- 12. minAreaRect ---------------------------------------------------------------------------------

def _rotating_calipers(pts):
    """rotatingCalipers(.., CALIPERS_MINAREARECT): float32 throughout; pts
    float32 [n][2], n >= 3, a strict hull.  -> out[6]."""
    n = len(pts)
    px = [f32(v) for v in pts[:, 0]]
    py = [f32(v) for v in pts[:, 1]]
    vx, vy, inv = [None] * n, [None] * n, [None] * n
    left = bottom = right = top = 0
    left_x = right_x = px[0]
    top_y = bottom_y = py[0]
    for i in range(n):
        if px[i] < left_x:
            left_x, left = px[i], i
        if px[i] > right_x:
            right_x, right = px[i], i
        if py[i] > top_y:
            top_y, top = py[i], i
        if py[i] < bottom_y:
            bottom_y, bottom = py[i], i
        j = i + 1 if i + 1 < n else 0
        dx = float(px[j]) - float(px[i])
        dy = float(py[j]) - float(py[i])
        vx[i], vy[i] = f32(dx), f32(dy)
        inv[i] = f32(1.0 / math.sqrt(dx * dx + dy * dy))
    orientation = f32(0)
    ax, ay = float(vx[n - 1]), float(vy[n - 1])
    for i in range(n):
        bx, by = float(vx[i]), float(vy[i])
        convexity = ax * by - ay * bx
        if convexity != 0:
            orientation = f32(1) if convexity > 0 else f32(-1)
            break
        ax, ay = bx, by
    assert orientation != 0
    base_a, base_b = orientation, f32(0)
    seq = [bottom, right, top, left]
    minarea = f32(np.finfo(np.float32).max)
    best = None
    for _ in range(n):
        dp = [base_a * vx[seq[0]] + base_b * vy[seq[0]],
              -base_b * vx[seq[1]] + base_a * vy[seq[1]],
              -base_a * vx[seq[2]] - base_b * vy[seq[2]],
              base_b * vx[seq[3]] - base_a * vy[seq[3]]]
        maxcos = dp[0] * inv[seq[0]]
        main = 0
        for e in (1, 2, 3):
            c = dp[e] * inv[seq[e]]
            if c > maxcos:
                maxcos, main = c, e
        p = seq[main]
        lead_x, lead_y = vx[p] * inv[p], vy[p] * inv[p]
        if main == 0:
            base_a, base_b = lead_x, lead_y
        elif main == 1:
            base_a, base_b = lead_y, -lead_x
        elif main == 2:
            base_a, base_b = -lead_x, -lead_y
        else:
            base_a, base_b = -lead_y, lead_x
        seq[main] = 0 if seq[main] + 1 == n else seq[main] + 1
        dx, dy = px[seq[1]] - px[seq[3]], py[seq[1]] - py[seq[3]]
        width = dx * base_a + dy * base_b
        dx, dy = px[seq[2]] - px[seq[0]], py[seq[2]] - py[seq[0]]
        height = -dx * base_b + dy * base_a
        area = width * height
        if area <= minarea:
            minarea = area
            best = (seq[3], base_a, width, base_b, height, seq[0])
    il, A1, width, B1, height, ib = best
    A2, B2 = -B1, A1
    C1 = A1 * px[il] + py[il] * B1
    C2 = A2 * px[ib] + py[ib] * B2
    idet = f32(1) / (A1 * B2 - A2 * B1)
    return [(C1 * B2 - C2 * B1) * idet, (A1 * C2 - A2 * C1) * idet, A1 * width, B1 * width, A2 * height, B2 * height]


def min_area_rect(points):
    """cv::minAreaRect of integer points -> float32 [5]: cx cy w h angle
    (degrees)."""
    with np.errstate(all="ignore"):
        hull = convex_hull(points).astype(f32)
        n = len(hull)
        cx = cy = w = h = angle = f32(0)
        if n > 2:
            o = _rotating_calipers(hull)
            cx = o[0] + (o[2] + o[4]) * f32(0.5)
            cy = o[1] + (o[3] + o[5]) * f32(0.5)
            w = f32(math.sqrt(float(o[2]) * float(o[2]) + float(o[3]) * float(o[3])))
            h = f32(math.sqrt(float(o[4]) * float(o[4]) + float(o[5]) * float(o[5])))
            angle = f32(math.atan2(float(o[3]), float(o[2])))
        elif n == 2:
            cx = (hull[0, 0] + hull[1, 0]) * f32(0.5)
            cy = (hull[0, 1] + hull[1, 1]) * f32(0.5)
            dx = float(hull[1, 0]) - float(hull[0, 0])
            dy = float(hull[1, 1]) - float(hull[0, 1])
            w = f32(math.sqrt(dx * dx + dy * dy))
            angle = f32(math.atan2(dy, dx))
        elif n == 1:
            cx, cy = hull[0, 0], hull[0, 1]
        angle = f32(float(f32(angle * f32(180))) / math.pi)
        return np.array([cx, cy, w, h, angle], f32)


def scale_box(box):
    """size and centre times 1.0 / 0.25 (float * double stored as float)."""
    b = np.asarray(box, f32).copy()
    b[:4] = (b[:4].astype(np.float64) * (1.0 / SCALE)).astype(f32)
    return b


def rect_corners(box):
    """The four corners of (cx, cy, w, h, angle) in fp64 (for the tests)."""
    cx, cy, w, h, ang = (float(v) for v in box)
    a = math.radians(ang)
    ux, uy = math.cos(a), math.sin(a)
    c = np.array([cx, cy])
    e0, e1 = np.array([ux, uy]) * w * 0.5, np.array([-uy, ux]) * h * 0.5
    return np.array([c - e0 - e1, c + e0 - e1, c + e0 + e1, c - e0 + e1])


# ---- the whole call ---------------------------------------------------------------------------------------

class ScanGuidanceRef:
    """CScanGuidance with its histogram state.  ema = 0: the reference as
    written (_frameCount stays 0, the histogram is replaced every frame);
    ema = 1: the blend at CScanGuidance.cpp:81, the first update replacing."""

    def __init__(self, h_bins=H_BINS, s_bins=S_BINS, threshold=THRESHOLD, alpha=ALPHA, ema=0):
        self.h_bins, self.s_bins, self.threshold, self.alpha, self.ema = h_bins, s_bins, threshold, alpha, int(ema)
        self.hist = None

    def calculate_mask(self, img, pts3d, R, t, K) -> dict:
        img = np.asarray(img, np.uint8)
        H, W = img.shape[:2]
        ws, hs = small_size((W, H))
        X = np.asarray(pts3d, np.float64).reshape(-1, 3)
        o = {"centroid": centroid(X), "n_points": len(X)}
        o["pixels"] = project_points(X, R, t, K, (W, H))
        o["small_pixels"] = small_points(o["pixels"])
        o["hull"] = convex_hull(o["small_pixels"])
        o["mask"] = fill_hull(o["hull"], ws, hs)
        o["area"] = contour_area(o["hull"])
        o["small"] = resize_linear(img, ws, hs)
        h, s, _ = bgr_to_hsv(to_float(o["small"]))
        o["bins"] = bins_of(h, s, self.h_bins, self.s_bins)
        o["frame_hist"] = calc_hist(o["bins"], o["mask"], self.h_bins, self.s_bins)
        if self.ema and self.hist is not None:
            self.hist = blend(o["frame_hist"], self.hist, self.alpha)
        else:
            self.hist = o["frame_hist"].copy()
        o["hist"] = self.hist.copy()
        o["bproj"] = back_project(o["bins"], self.hist)
        acc = accept(o["bproj"], o["area"], self.threshold)
        ys, xs = np.nonzero(acc)
        o["accepted"] = np.stack([xs, ys], axis=1).astype(np.int64)
        o["extents"] = row_extents(acc)
        o["box"] = scale_box(min_area_rect(o["accepted"]))
        o["n_projected"], o["n_hull"], o["n_accepted"] = len(o["pixels"]), len(o["hull"]), len(o["accepted"])
        return o


def calculate_mask(img, pts3d, R, t, K, **options) -> dict:
    return ScanGuidanceRef(**options).calculate_mask(img, pts3d, R, t, K)


def extent_points(extents):
    """The (x, y) points the library's host tail gets from the row extents."""
    e = np.asarray(extents).reshape(-1, 2)
    rows = np.flatnonzero(e[:, 1] >= 0)
    return np.concatenate([np.stack([e[rows, 0], rows], 1), np.stack([e[rows, 1], rows], 1)]).astype(np.int64)
