"""The reference's LIVE tracking path (CSfM::tracking + CSfM::mapping,
/root/reference/CSfM.cpp:109-261, 500-692) on the device stages, fed by
synthetic detector output (KeypointStream) or the device BRISK detector on
rendered frames (BriskVideoStream, row T8).

Per frame (CSfM::tracking):
  1. the frame's keypoints + descriptors go up once (sfm_matcher_push_frame);
  2. matchFeatures(prev matched 2D idx, all current) -- the live
     frame-to-frame call of CSfM.cpp:518 (sfm_matcher_match_subset, window
     (1.5, 40) px, ratio 0.8);
  3. the matched previous keypoints' map points + current positions ->
     solvePnPRansac(20, 7 px, 0.99) (sfm_pnp_ransac); inliers become the
     frame's map associations (CSfM.cpp:553-582);
  4. findMapPointsInCurrentFrame (CSfM.cpp:634-692): points of every
     keyframe (CMap::getPointsInFrames on the device map store) minus the
     frame's, projected with the PnP pose, their representative descriptors
     (device) matched against the unmatched keypoints in the (0, 7) window
     (sfm_matcher_match);
  5. addKeyFrame (CSfM.cpp:481-497: >= 10 frames after the last keyframe,
     >= 50 matched, < 90% of the last keyframe's) -> addPointMatches +
     addDescriptors, then mapping.
Per keyframe (CSfM::mapping): against every earlier keyframe, match their
unmatched keypoints (member window), triangulate (sfm_triangulate_points),
filter, addNewPoints / addDescriptors, re-find the new points in the
keyframes in between (0, 7) window, add them to the new keyframe; then
bundle adjustment over all keyframes, gathered frame-major through
CMap::getPointsInFrame as CSfM::bundleAdjustment does (CSfM.cpp:310-348),
one-shot sfm_ba_solve, poses and points written back.

The initial map (CSfM::init, CSfM.cpp:802-1001): init="known" reads the
second keyframe's pose from the stream's ground truth (the synthetic
bootstrap); init="estimate" runs the reference's two-view initialisation on
the matcher's matches (sfm_two_view_init, sfm_amd/init.py: homography and
fundamental matrix, model choice, R, t, triangulation, filter) and retries on
the next frame while it fails, the first keyframe staying (CSfM.cpp:984-1000);
the map's scale is then the unit baseline of the first two keyframes.

Scope notes: GeometryUtils (filterMatches, projectPoints) is not
in the reference tree, so filterMatches is restated from its call site
(CSfM.cpp:164-165) as positive depth in both keyframes and the point-to-
epipolar-line distance <= _maxReprErr both ways.

Point creation on the device (device_mapping=True, off by default): the pair
loop of CSfM::mapping (CSfM.cpp:138-227) as device calls on the matcher's
keyframe store -- per older keyframe one sfm_matcher_pair_points (match,
triangulate, filter; self.map_log keeps every call), per keyframe in between
one sfm_matcher_refind_points, and the descriptor rows go into the map from
the keyframe store (sfm_map_add_keyframe_rows; the keyframe insert of
tracking too).  The same map calls in the same order as the host loop; the
filter and the projection round in the fixed association of
tests/map_points_ref.py, the host loop's as numpy's BLAS does, so borderline
matches may differ between the two.  batch_pairs=True (with device_mapping)
runs all older keyframes of a new one in one call, up to the first pair that
keeps a point (sfm_matcher_pair_points_first): a pair that keeps none changes
nothing, so the map is the pair-by-pair loop's, bit for bit, in fewer calls.

Culling (cull=True; CSfM.cpp:232-252, 692-752, off by default): between the
pair loop and the BA, CSfM::cullMapPoints (CMap::removePointsThreshold on
the device map store, then CFrame::cullPoints on every keyframe, the
previous and the current frame) and CSfM::cullKeyFrames (the whole greedy
loop in one device call, sfm_map_cull_keyframes), the culled keyframes
leaving self.kfs.  The counters behind the rules live in the map store:
CMap::updatePointViews (the PnP inliers, CSfM.cpp:576, then the re-found
points, :685) and the per-frame incrementMapAge(1, 0) (:629, lost frames
included) are accumulated on the host and flushed in one call each at the
start of mapping, before any point is created or removed, which equals the
per-frame calls (points are created only by init and mapping) and adds no
device call to the tracking path; incrementMapAge(0, 2) follows init
(:962) and incrementMapAge(0, 1) every mapping's BA (:304).  Keyframes own a
fixed slot of the matcher's keyframe store, taken from a counter when they
are stored (their list position while nothing is culled); a culled
keyframe's slot is emptied.
"""
from __future__ import annotations

import os
import time

import numpy as np

from . import ba as _ba
from .cmap import DeviceMap
from .init import two_view_init
from .mapping import F_PIX, _rodrigues, _rodrigues_inv, triangulate_points
from .matcher import FeatureMatcher
from .pnp import solvePnPRansac

MAX_REPR_ERR = 7.0     # CSfM.cpp:35
KF_TIME_LAG = 10       # CSfM.cpp:44
MIN_FEATURES = 5       # CTracker::_minFeatures (CTracker.cpp:32)


class KeypointStream:
    """Synthetic detector output: `n_landmarks` 3D points with a fixed
    512-bit descriptor each, seen by a 1280x720 pinhole camera translating
    ~2 px per frame with a slow roll.  A landmark is detectable during its
    lifetime only (`lifetime` frames from a uniform birth over `horizon`),
    as detector features come and go with viewpoint and lighting: the view's
    content turns over at a few percent per frame, so CSfM's keyframe rule
    (< 90% of the last keyframe's matches) fires while consecutive
    keyframes are still inside the member match window (40 px).  Per frame
    every live visible landmark is detected with probability `p_detect`
    (0.3-px noise, `bit_noise` flipped descriptor bits) and `spurious` random
    keypoints are mixed in; the order is shuffled.  Closed-form ground
    truth: pose(k), landmark of each keypoint."""

    def __init__(self, n_landmarks: int = 15000, seed: int = 7, p_detect: float = 0.85, bit_noise: int = 8,
                 spurious: float = 0.15, px_sigma: float = 0.3, step: float = 0.0196, desc_bytes: int = 64,
                 lifetime=(40, 100), horizon: int = 400, dist=None):
        rng = np.random.default_rng(seed)
        self.w, self.h = 1280, 720
        self.K = np.array([[F_PIX, 0.0, 640.0], [0.0, F_PIX, 360.0], [0.0, 0.0, 1.0]])
        # dist (lens coefficients k1 k2 p1 p2 [k3 [k4 k5 k6]]): the camera
        # above gets that lens.  The landmarks are still seen by a pinhole
        # camera, now the camera's Kopt (stream.K), and the keypoints returned
        # are those pixels pushed through the forward lens model into the
        # lens's own image: what a detector on the distorted frames reports.
        self.camera = None
        if dist is not None:
            from .camera import Camera
            self.camera = Camera(self.K, dist, (self.w, self.h))
            self.K = self.camera.Kopt.copy()
        self.L = np.column_stack([rng.uniform(-6.0, 14.0, n_landmarks), rng.uniform(-4.0, 4.0, n_landmarks),
                                  rng.uniform(8.0, 14.0, n_landmarks)])
        self.D = rng.integers(0, 256, size=(n_landmarks, desc_bytes), dtype=np.uint8)
        self.birth = rng.integers(-lifetime[1], horizon, size=n_landmarks)
        self.death = self.birth + rng.integers(lifetime[0], lifetime[1] + 1, size=n_landmarks)
        self.seed, self.p_detect, self.bit_noise = seed, p_detect, bit_noise
        self.spurious, self.px_sigma, self.step, self.desc_bytes = spurious, px_sigma, step, desc_bytes

    def pose(self, k: int):
        """(rvec, t) of frame k: x_cam = R X + t (frame 0 at the origin)."""
        c = np.array([self.step * k, 0.15 * np.sin(0.02 * k), 0.0])
        r = np.array([0.0, 0.0, 0.0008 * k])
        R = _rodrigues(r)
        return r, -R @ c

    def frame(self, k: int):
        rng = np.random.default_rng((self.seed, k))
        r, t = self.pose(k)
        Xc = self.L @ _rodrigues(r).T + t
        if self.camera is None:
            uv = Xc[:, :2] / Xc[:, 2:3] * F_PIX + self.K[:2, 2]
        else:
            uv = Xc[:, :2] / Xc[:, 2:3] * np.array([self.K[0, 0], self.K[1, 1]]) + self.K[:2, 2]
        vis = (Xc[:, 2] > 0.5) & (uv[:, 0] >= 16) & (uv[:, 0] < self.w - 16) & (uv[:, 1] >= 16) & \
              (uv[:, 1] < self.h - 16) & (self.birth <= k) & (k < self.death) & (rng.random(len(uv)) < self.p_detect)
        lid = np.flatnonzero(vis)
        pts = uv[lid] + rng.normal(0.0, self.px_sigma, size=(len(lid), 2))
        desc = self.D[lid].copy()
        nb = self.desc_bytes * 8
        for _ in range(self.bit_noise):
            bit = rng.integers(0, nb, size=len(lid))
            desc[np.arange(len(lid)), bit // 8] ^= (1 << (bit % 8)).astype(np.uint8)
        ns = int(self.spurious * len(lid))
        pts = np.vstack([pts, np.column_stack([rng.uniform(16, self.w - 16, ns), rng.uniform(16, self.h - 16, ns)])])
        desc = np.vstack([desc, rng.integers(0, 256, size=(ns, self.desc_bytes), dtype=np.uint8)])
        lid = np.concatenate([lid, np.full(ns, -1)])
        perm = rng.permutation(len(lid))
        if self.camera is not None:
            pts = self.camera.distort(pts)
        return pts[perm], desc[perm], lid[perm]


class BriskVideoStream:
    """Detector output of the device BRISK (sfm_brisk_detect_describe,
    row T8) on the rendered synthetic video (sfm_amd.video: a textured plane
    at depth 10, ~2.6 px of motion per frame at speed 2), with the video's
    closed-form poses: the live loop on real detections."""

    def __init__(self, video=None, threshold: int = 60, octaves: int = 6, device: int = 0, depth: float = 10.0):
        from .video import SyntheticVideo
        self.video = video if video is not None else SyntheticVideo(speed=2.0)
        self.threshold, self.octaves, self.device, self.depth = int(threshold), int(octaves), device, float(depth)
        c = self.video.c
        self.K = np.array([[F_PIX, 0.0, c[0]], [0.0, F_PIX, c[1]], [0.0, 0.0, 1.0]])
        self.desc_bytes = 64

    def pose(self, k: int):
        from .mapping import video_gt_pose
        return video_gt_pose(self.video, k, self.depth)

    def frame(self, k: int):
        from . import brisk
        kp, _, desc = brisk.detect(self.video.frame(k), self.threshold, self.octaves, device=self.device)
        return kp[:, :2].astype(np.float64), desc, np.full(len(kp), -1)


def pair_frame_observations(p3, p2):
    """The 2D index of every entry of one frame's getPointsInFrame result.

    Entry e of p3 (point p, the r-th of p's k entries in the frame, in
    equal-range order) owns the k 2D indices p2[o_e : o_e + k] (o_e = the
    sum of the earlier entries' k; CMap.cpp:225-240 emits p's whole 2D list
    for the frame per entry), and its own observation is the r-th of them:
    both lists follow emplace order.  Without duplicates this is p2 itself.
    """
    p3 = np.asarray(p3)
    p2 = np.asarray(p2)
    n = len(p3)
    if n == len(p2):  # no point twice in the frame (k = 1 everywhere)
        return p2
    _, inv, cnt = np.unique(p3, return_inverse=True, return_counts=True)
    k = cnt[inv]
    o = np.concatenate([[0], np.cumsum(k)[:-1]])
    order = np.argsort(inv, kind="stable")
    start = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    r = np.empty(n, np.int64)
    r[order] = np.arange(n) - start[inv[order]]
    if int(k.sum()) != len(p2):
        raise ValueError(f"2D list of {len(p2)} entries, expected {int(k.sum())}")
    return p2[o + r]


class _Frame:
    """CFrame: keypoints (undistorted), descriptors, 3D index per keypoint
    (-1: unmatched), pose."""

    def __init__(self, no, pts, desc, ptsd=None):
        self.no, self.pts, self.desc = no, pts, desc
        self.ptsd = ptsd    # distorted positions (CFrame::_pts_dist) when the loop has a camera
        self.slot = -1  # keyframes: the matcher's keyframe-store slot
        self.pt3d = np.full(len(pts), -1, np.int64)
        self.rot, self.t = np.zeros(3), np.zeros(3)

    def n_matched(self) -> int:
        return int((self.pt3d >= 0).sum())

    def copy(self):
        f = _Frame(self.no, self.pts, self.desc, self.ptsd)
        f.pt3d, f.rot, f.t, f.slot = self.pt3d.copy(), self.rot.copy(), self.t.copy(), self.slot
        return f

    def P(self, K):
        return K @ np.hstack([_R(self.rot), self.t.reshape(3, 1)])


_RCACHE: dict = {}


def _R(rot):
    """_rodrigues(rot), memoised on rot's bytes (a keyframe's pose is asked
    for by every mapping pass and re-finding; the values are the function's
    own, the arrays are not to be modified)."""
    key = np.asarray(rot, np.float64).tobytes()
    R = _RCACHE.get(key)
    if R is None:
        if len(_RCACHE) > 4096:
            _RCACHE.clear()
        R = _RCACHE[key] = _rodrigues(rot)
    return R


def _project(K, rot, t, X):
    Xc = X @ _R(rot).T + t
    return Xc[:, :2] / Xc[:, 2:3] * np.array([K[0, 0], K[1, 1]]) + K[:2, 2], Xc[:, 2]


def _filter_matches(K, f0, f1, uv0, uv1, X, max_err):
    """filterMatches restated from its call site (CSfM.cpp:164-165): positive
    depth in both keyframes, point-to-epipolar-line distance <= max_err both
    ways (F of the two poses)."""
    R0, R1 = _R(f0.rot), _R(f1.rot)
    R = R1 @ R0.T
    tt = f1.t - R @ f0.t
    tx = np.array([[0, -tt[2], tt[1]], [tt[2], 0, -tt[0]], [-tt[1], tt[0], 0]])
    Ki = np.linalg.inv(K)
    F = Ki.T @ tx @ R @ Ki
    h0 = np.column_stack([uv0, np.ones(len(uv0))])
    h1 = np.column_stack([uv1, np.ones(len(uv1))])
    l1 = h0 @ F.T          # lines in image 1
    l0 = h1 @ F            # lines in image 0
    d1 = np.abs((l1 * h1).sum(1)) / np.hypot(l1[:, 0], l1[:, 1])
    d0 = np.abs((l0 * h0).sum(1)) / np.hypot(l0[:, 0], l0[:, 1])
    z0 = (X @ R0.T + f0.t)[:, 2]
    z1 = (X @ R1.T + f1.t)[:, 2]
    return (z0 > 0) & (z1 > 0) & (d0 <= max_err) & (d1 <= max_err) & np.isfinite(X).all(1)


class LiveSfM:
    def __init__(self, stream: KeypointStream | None = None, device: int = 0, init_gap: int = 5,
                 init: str = "known", init_options: dict | None = None, cull: bool = False,
                 cull_kf_rate: float = 0.9, min_visibility: int = 3, camera=None, guidance: bool = False,
                 guidance_options: dict | None = None, device_mapping: bool = False, batch_pairs: bool = False):
        if init not in ("known", "estimate"):
            raise ValueError(f"init must be 'known' or 'estimate', not {init!r}")
        if batch_pairs and not device_mapping:
            raise ValueError("batch_pairs batches the device calls of device_mapping=True")
        if guidance and camera is None:
            raise ValueError("guidance needs a camera (it reads the colour frame: process_image)")
        self.init = init
        self.init_options = dict(init_options or {})
        self.init_log: list[dict] = []   # init="estimate": one entry per attempt
        self.stream = stream if stream is not None else KeypointStream()
        # camera (sfm_amd.camera.Camera, CSfM(K, imSize, d)): process() takes
        # distorted pixels, undistorts them on the device and works in the
        # Kopt image throughout; None: detector output is taken as undistorted
        self.camera = camera
        self.K = camera.Kopt if camera is not None else self.stream.K
        self._installed = False    # process_image: the matcher already holds the current frame
        self._front = None
        self.device = device
        self.init_gap = int(init_gap)
        self.matcher = FeatureMatcher(self.stream.desc_bytes, device=device)
        self.map = DeviceMap(self.stream.desc_bytes, device=device)
        self.kfs: list[_Frame] = []
        self.prev: _Frame | None = None
        self.frame_no = -1
        self.lost = 0
        self.ba_log: list[dict] = []
        self.stats = {"frames": 0, "tracked": 0, "pnp_inliers": 0, "map_matches": 0, "new_points": 0}
        # CSfM::cullMapPoints / cullKeyFrames (thresholdRate, _minVisibilityFrameNo: CSfM.h:70, CSfM.cpp:50)
        self.cull, self.cull_kf_rate, self.min_visibility = bool(cull), float(cull_kf_rate), int(min_visibility)
        self.cull_log: list[dict] = []
        self._views: list[np.ndarray] = []   # updatePointViews since the last mapping
        self._age = 0                        # incrementMapAge(1, 0) since the last mapping
        self._cur: _Frame | None = None
        self._n_slots = 0
        if self.cull:
            self.stats.update({"culled_points": 0, "culled_keyframes": 0})
        self.times = {"stream": 0.0, "track": 0.0, "map_match": 0.0, "mapping": 0.0, "ba": 0.0}
        self._pending: _Frame | None = None
        # CSfM::mapping's point creation as device calls on the resident
        # keyframe rows (sfm_matcher_pair_points / sfm_matcher_refind_points /
        # sfm_map_add_keyframe_rows), off by default: the default path's filter
        # and projection round as numpy's BLAS does, the device's in the fixed
        # association of tests/map_points_ref.py
        self.device_mapping = bool(device_mapping)
        self.map_log: list[dict] = []    # device_mapping: one entry per keyframe-pair call
        # all older keyframes of a new one in one call, up to the first pair
        # that keeps a point (sfm_matcher_pair_points_first): the same map,
        # bit for bit, in fewer calls; map_log then has one entry per batch
        self.batch_pairs = bool(batch_pairs)
        # CScanGuidance (CSfM.cpp:80-81): after every RUNNING frame's tracking
        # and mapping, on the map's live points, read on the device
        self._guidance = None
        self.guidance = None                 # the latest GuidanceFrame
        self.guidance_log: list = []         # one per call
        self._prev_img = None                # _prevFrame.getFrame() (kept by reference, as a cv::Mat would be)
        if guidance:
            from .guidance import ScanGuidance
            self._guidance = ScanGuidance(camera.width, camera.height, device=device, **(guidance_options or {}))
            self.times["guidance"] = 0.0
        # the fused device calls (SFM_LIVE_COMPOSED=1: the composed calls,
        # for A/B timing; the tests compare both forms)
        composed = os.environ.get("SFM_LIVE_COMPOSED") == "1"
        self.fused_find = not composed
        self.fused_track = not composed
        self.resident_kf = not composed  # mapping matches on the matcher's keyframe store

    # ---- driver --------------------------------------------------------------
    def run(self, n_frames: int) -> None:
        for k in range(n_frames):
            t0 = time.perf_counter()
            pts, desc, _ = self.stream.frame(k)
            self.times["stream"] += time.perf_counter() - t0
            self.process(k, pts, desc)

    def process(self, k: int, pts, desc) -> None:
        if self.camera is None:
            self._process(k, pts, desc, None)
            return
        # CFrame::setKeyPoints: undistortPoints(_pts_dist, _pts, _K, _d, _Kopt)
        ptsd = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 2)
        self._process(k, self.camera.undistort(ptsd, device=self.device), desc, ptsd)

    def process_image(self, k: int, img) -> None:
        """process() from the frame itself (8-bit grey or 3-channel): grey
        conversion, BRISK and the undistortion in one device call
        (sfm_frame_detect), whose result is already the matcher's current
        frame when the loop gets to it."""
        if self.camera is None:
            raise ValueError("process_image needs a camera")
        if self._front is None:
            from .camera import FrameFrontEnd
            th = getattr(self.stream, "threshold", 60)
            oc = getattr(self.stream, "octaves", 6)
            self._front = FrameFrontEnd(self.camera, matcher=self.matcher, threshold=th, octaves=oc)
        if self._guidance is not None and np.ndim(img) != 3:
            raise ValueError("guidance needs the colour frame: img must be [h][w][3]")
        running = len(self.kfs) >= 2            # CSfM's RUNNING state at entry
        kps, _, desc, pts = self._front.detect(img)
        self._installed = True
        try:
            self._process(k, pts, desc, kps[:, :2].astype(np.float64))
        finally:
            self._installed = False
        if self._guidance is not None:
            self._guide(k, img, running)

    def _guide(self, k: int, img, running: bool) -> None:
        """_guidance.calculateMask(_prevFrame.getFrame(), mapPts, Kopt, P of
        _prevFrame) (CSfM.cpp:80-81): on a lost frame _prevFrame, and so the
        image, is the earlier frame's."""
        if self.prev is not None and self.prev.no == k:
            self._prev_img = img
        if not running:
            return
        if self._prev_img is None:
            raise ValueError("guidance needs every frame through process_image (the previous frame has no image)")
        t0 = time.perf_counter()
        self.guidance = self._guidance.update(self._prev_img, _R(self.prev.rot), self.prev.t, self.K, map=self.map)
        self.guidance_log.append(self.guidance)
        self.times["guidance"] += time.perf_counter() - t0

    def _push_current(self, pts, desc, ptsd) -> None:
        """sfm_matcher_push_frame of the frame being processed, unless
        process_image has installed it on the device already."""
        if self._installed:
            self._installed = False
            return
        self.matcher.push_frame(pts, desc, ptsd)

    def _process(self, k: int, pts, desc, ptsd) -> None:
        self.frame_no = k
        self.stats["frames"] += 1
        if not self.kfs:
            f = _Frame(k, pts, desc, ptsd)
            self.kfs.append(f)                  # first keyframe at the origin (CFrame.cpp:229-235)
            self._store_keyframe(f)
            self._push_current(pts, desc, ptsd)
            self.prev = f
            return
        if len(self.kfs) == 1:
            if k < self.init_gap:
                return
            self._initialise(k, pts, desc, ptsd)
            return
        self._tracking(k, pts, desc, ptsd)

    # ---- initial map (CSfM::init) ----------------------------------------------
    def _initialise(self, k, pts, desc, ptsd=None) -> None:
        f0 = self.kfs[0]
        f1 = _Frame(k, pts, desc, ptsd)
        if self.init == "estimate":
            # CSfM.cpp:823-946 on the device: no pose is read from the stream
            i0, i1 = self.matcher.match(f0.pts, f0.desc, f1.pts, f1.desc)
            r = two_view_init(f0.pts[i0], f1.pts[i1], self.K, self.K, device=self.device, **self.init_options)
            self.init_log.append({"frame": k, "matches": len(i0), "model": r.model, "n_kept": r.n_kept,
                                  "scores": r.scores.copy(), "avg_err": r.avg_err, "pts0": f0.pts[i0], "pts1": f1.pts[i1]})
            if not r.ok:
                return  # the first keyframe stays; the next frame tries again (CSfM.cpp:984-1000)
            f1.rot, f1.t = _rodrigues_inv(r.R), r.t.copy()
            self._push_current(pts, desc, ptsd)
            ok, X = r.keep.astype(bool), r.X
        else:
            f1.rot, f1.t = self.stream.pose(k)
            self._push_current(pts, desc, ptsd)
            i0, i1 = self.matcher.match(f0.pts, f0.desc, f1.pts, f1.desc)
            X = triangulate_points(np.zeros(len(i0), np.int32), np.ones(len(i0), np.int32), f0.pts[i0], f1.pts[i1],
                                   np.stack([f0.P(self.K), f1.P(self.K)]), device=self.device)
            ok = _filter_matches(self.K, f0, f1, f0.pts[i0], f1.pts[i1], X, MAX_REPR_ERR)
        i0, i1, X = i0[ok], i1[ok], X[ok]
        idx = self.map.addNewPoints(X, np.stack([i0, i1]), [f0.no, f1.no])
        self.map.addDescriptors(idx, f0.desc[i0])
        self.map.addDescriptors(idx, f1.desc[i1])
        f0.pt3d[i0] = idx
        f1.pt3d[i1] = idx
        self.kfs.append(f1.copy())
        self._store_keyframe(self.kfs[-1])
        self.stats["new_points"] += len(idx)
        if self.cull:
            self.map.incrementMapAge(0, 2)      # CSfM.cpp:962
        self._bundle_adjust()
        self.prev = f1
        self.prev.rot, self.prev.t = self.kfs[-1].rot.copy(), self.kfs[-1].t.copy()

    # ---- CSfM::tracking ----------------------------------------------------------
    def _tracking(self, k, pts, desc, ptsd=None) -> None:
        t0 = time.perf_counter()
        cur = _Frame(k, pts, desc, ptsd)
        self._age += 1                          # CSfM.cpp:629, whatever the frame's fate
        self._push_current(pts, desc, ptsd)
        if self.fused_track:
            # matchFeatures + getPointsAtIdx + solvePnPRansac in one device call
            # (sfm_track_pnp); the composed form below is the test's reference
            nm, found, r, t, ikp, ipt = self.matcher.track_pnp(self.map, self.prev.pt3d, self.K, MIN_FEATURES, 20,
                                                               MAX_REPR_ERR, 0.99)
        else:
            prev_idx = np.flatnonzero(self.prev.pt3d >= 0).astype(np.int32)
            pm, cm = self.matcher.match_subset(prev_idx, np.arange(len(pts), dtype=np.int32))
            nm = len(cm)
        if nm < MIN_FEATURES:
            # lost: keep matching against the previous frame (no swap)
            self.lost += 1
            self.matcher.push_frame(self.prev.pts, self.prev.desc, self.prev.ptsd)
            self.times["track"] += time.perf_counter() - t0
            return
        self.lost = 0
        if not self.fused_track:
            m3 = self.prev.pt3d[pm]
            obj = self.map.getPointsAtIdx(m3)
            found, r, t, inl = solvePnPRansac(obj, pts[cm], self.K, 20, MAX_REPR_ERR, 0.99, device=self.device)
            ikp, ipt = cm[inl], m3[inl]
        cur.rot, cur.t = np.asarray(r, float), np.asarray(t, float)
        cur.pt3d[ikp] = ipt
        if self.cull:
            self._views.append(np.asarray(ipt, np.int32).copy())    # CSfM.cpp:576
        self.stats["tracked"] += 1
        self.stats["pnp_inliers"] += len(ikp)
        t1 = time.perf_counter()
        self.times["track"] += t1 - t0
        self._find_map_points(cur)
        self.times["map_match"] += time.perf_counter() - t1
        if self._add_keyframe(cur):
            kf = cur.copy()
            self.kfs.append(kf)
            self._store_keyframe(kf)
            m = np.flatnonzero(kf.pt3d >= 0)
            if self.device_mapping:     # the descriptors are in the keyframe store already
                self.map.addKeyframeRows(self.matcher, kf.slot, kf.no, kf.pt3d[m], m)
            else:
                self.map.addPointMatches(kf.pt3d[m], m, kf.no)
                self.map.addDescriptors(kf.pt3d[m], kf.desc[m])
            t2 = time.perf_counter()
            self._cur = cur
            self._mapping()
            self._cur = None
            self.times["mapping"] += time.perf_counter() - t2
            # CSfM.cpp:261: the previous frame takes the adjusted keyframe pose
            cur.rot, cur.t = self.kfs[-1].rot.copy(), self.kfs[-1].t.copy()
        self.prev = cur

    def _find_map_points(self, cur: _Frame) -> None:
        """CSfM::findMapPointsInCurrentFrame (CSfM.cpp:634-692): one device call
        (sfm_map_match_frame) -- the composed form below (self.fused_find =
        False) is the same query as separate map / matcher calls, kept as the
        test's reference."""
        if self.fused_find:
            un = np.flatnonzero(cur.pt3d < 0).astype(np.int32)
            if len(un) < 2:
                return
            existing = cur.pt3d[cur.pt3d >= 0].astype(np.int32)
            pm, km = self.map.matchFrame(self.matcher, [f.no for f in self.kfs], existing, _R(cur.rot),
                                         cur.t, self.K, un, 0.8, 0.0, MAX_REPR_ERR)
            cur.pt3d[km] = pm
            self.stats["map_matches"] += len(pm)
            if self.cull:
                self._views.append(np.asarray(pm, np.int32).copy())  # CSfM.cpp:685
            return
        cov = self.map.getPointsInFrames([f.no for f in self.kfs])
        existing = np.unique(cur.pt3d[cur.pt3d >= 0])
        new = np.setdiff1d(cov, existing, assume_unique=True).astype(np.int32)
        un = np.flatnonzero(cur.pt3d < 0)
        if not len(new) or len(un) < 2:
            return
        X = self.map.getPointsAtIdx(new)
        desc = self.map.getRepresentativeDescriptors(new)
        uv, _ = _project(self.K, cur.rot, cur.t, X)
        mi, fi = self.matcher.match(uv, desc, cur.pts[un], cur.desc[un], 0.8, 0.0, MAX_REPR_ERR)
        cur.pt3d[un[fi]] = new[mi]
        self.stats["map_matches"] += len(mi)
        if self.cull:
            self._views.append(np.asarray(new[mi], np.int32).copy())

    def _add_keyframe(self, cur: _Frame) -> bool:
        """CSfM::addKeyFrame (CSfM.cpp:481-497)."""
        last = self.kfs[-1]
        a = cur.no >= last.no + KF_TIME_LAG
        b = cur.n_matched() >= 50
        c = cur.n_matched() < 0.9 * last.n_matched()
        return a and b and c

    # ---- CSfM::mapping -------------------------------------------------------------
    def _store_keyframe(self, kf: _Frame) -> None:
        kf.slot = self._n_slots
        self._n_slots += 1
        self.matcher.store_keyframe(kf.slot, kf.pts, kf.desc)

    def _flush_counters(self) -> None:
        """The tracked frames' updatePointViews / incrementMapAge(1, 0) since
        the last mapping, one call each (the live set has not changed since)."""
        if self._views:
            v = np.concatenate(self._views)
            if len(v):
                self.map.updatePointViews(v)
        self._views = []
        if self._age:
            self.map.incrementMapAge(self._age, 0)
        self._age = 0

    def _cull(self) -> None:
        """CSfM::cullMapPoints, then CSfM::cullKeyFrames (CSfM.cpp:237-252)."""
        culled_pts, status = self.map.removePointsThreshold()
        if len(culled_pts):
            frames = list(self.kfs)
            for f in (self.prev, self._cur):
                if f is not None and all(f is not g for g in frames):
                    frames.append(f)
            for f in frames:                    # CFrame::cullPoints
                m = np.flatnonzero(f.pt3d >= 0)
                f.pt3d[m[status[f.pt3d[m]] == -1]] = -1
        lists = [(kf.no, kf.pt3d[kf.pt3d >= 0].astype(np.int32)) for kf in self.kfs]
        culled = self.map.cullKeyFrames(lists, self.min_visibility, self.cull_kf_rate)
        gone = [kf for kf, c in zip(self.kfs, culled) if c]
        for kf in gone:
            self.matcher.store_keyframe(kf.slot, np.zeros((0, 2)), np.zeros((0, self.stream.desc_bytes), np.uint8))
        self.kfs = [kf for kf, c in zip(self.kfs, culled) if not c]
        self.stats["culled_points"] += len(culled_pts)
        self.stats["culled_keyframes"] += len(gone)
        self.cull_log.append({"frame": self.frame_no, "points": np.asarray(culled_pts).copy(),
                              "keyframes": [kf.no for kf in gone], "lists": lists})

    def _mapping(self) -> None:
        if self.cull:
            self._flush_counters()
        new_kf = self.kfs[-1]
        if self.device_mapping:
            self._create_points_device(new_kf)
        for i in range(0 if self.device_mapping else len(self.kfs) - 1):
            kf = self.kfs[i]
            cu = np.flatnonzero(new_kf.pt3d < 0)
            pu = np.flatnonzero(kf.pt3d < 0)
            if len(cu) < 2 or len(pu) < 2:
                continue
            if self.resident_kf:
                pi, ci = self.matcher.match_keyframes(kf.slot, pu, new_kf.slot, cu)
            else:
                pi, ci = self.matcher.match(kf.pts[pu], kf.desc[pu], new_kf.pts[cu], new_kf.desc[cu])
            if not len(pi):
                continue
            uv0, uv1 = kf.pts[pu[pi]], new_kf.pts[cu[ci]]
            X = triangulate_points(np.zeros(len(pi), np.int32), np.ones(len(pi), np.int32), uv0, uv1,
                                   np.stack([kf.P(self.K), new_kf.P(self.K)]), device=self.device)
            ok = _filter_matches(self.K, kf, new_kf, uv0, uv1, X, MAX_REPR_ERR)
            if not ok.any():
                continue
            p2, c2, Xf = pu[pi[ok]], cu[ci[ok]], X[ok]
            idx = self.map.addNewPoints(Xf, p2.reshape(1, -1), [kf.no])
            kf.pt3d[p2] = idx
            pdesc, cdesc = kf.desc[p2], new_kf.desc[c2]
            self.map.addDescriptors(idx, pdesc)
            # re-find the new points in the keyframes in between (CSfM.cpp:189-221)
            for j in range(i + 1, len(self.kfs) - 1):
                kj = self.kfs[j]
                uj = np.flatnonzero(kj.pt3d < 0)
                if len(uj) < 2:
                    continue
                uv, _ = _project(self.K, kj.rot, kj.t, Xf)
                near_kf = abs(kj.no - kf.no) < abs(kj.no - new_kf.no)
                if self.resident_kf:
                    m0, m1 = self.matcher.match_keyframes(kf.slot if near_kf else new_kf.slot, p2 if near_kf else c2,
                                                          kj.slot, uj, uv, 0.8, 0.0, MAX_REPR_ERR)
                else:
                    d = pdesc if near_kf else cdesc
                    m0, m1 = self.matcher.match(uv, d, kj.pts[uj], kj.desc[uj], 0.8, 0.0, MAX_REPR_ERR)
                if len(m0):
                    self.map.addPointMatches(idx[m0], uj[m1], kj.no)
                    kj.pt3d[uj[m1]] = idx[m0]
                    self.map.addDescriptors(idx[m0], kj.desc[uj[m1]])
            self.map.addPointMatches(idx, c2, new_kf.no)
            new_kf.pt3d[c2] = idx
            self.map.addDescriptors(idx, cdesc)
            self.stats["new_points"] += len(idx)
        if self.cull:
            self._cull()
        t0 = time.perf_counter()
        self._bundle_adjust()
        self.times["ba"] += time.perf_counter() - t0
        if self.cull:
            self.map.incrementMapAge(0, 1)      # CSfM.cpp:304

    def _create_points_device(self, new_kf: _Frame) -> None:
        """The pair loop of _mapping (CSfM.cpp:138-227) on the device calls:
        per older keyframe one sfm_matcher_pair_points (match, triangulate,
        filter), the new points' descriptor rows from the keyframe store
        (sfm_map_add_keyframe_rows), per keyframe in between one
        sfm_matcher_refind_points.  The same map calls in the same order as
        the host loop."""
        K, R1 = self.K, _R(new_kf.rot)
        if self.batch_pairs:
            self._create_points_batched(new_kf, K, R1)
            return
        for i in range(len(self.kfs) - 1):
            kf = self.kfs[i]
            cu = np.flatnonzero(new_kf.pt3d < 0).astype(np.int32)
            pu = np.flatnonzero(kf.pt3d < 0).astype(np.int32)
            if len(cu) < 2 or len(pu) < 2:
                continue
            R0 = _R(kf.rot)
            m0, m1, Xf, n_matched = self.matcher.pair_points(kf.slot, pu, new_kf.slot, cu, K, R0, kf.t, K, R1,
                                                             new_kf.t, MAX_REPR_ERR)
            self.map_log.append({"frame": new_kf.no, "slot0": kf.slot, "slot1": new_kf.slot, "idx0": pu, "idx1": cu,
                                 "K": np.array(K, np.float64), "R0": R0.copy(), "t0": kf.t.copy(), "R1": R1.copy(),
                                 "t1": new_kf.t.copy(), "m0": m0, "m1": m1, "X": Xf, "n_matched": n_matched})
            if not len(m0):
                continue
            self._add_pair_points(i, new_kf, pu[m0], cu[m1], Xf)

    def _create_points_batched(self, new_kf: _Frame, K, R1) -> None:
        """_create_points_device's loop with one sfm_matcher_pair_points_first
        per stretch of older keyframes that keep no point: a pair that keeps
        none changes nothing, so every older keyframe from i on is matched
        against the same unmatched rows cu in one call; the first pair that
        keeps a point is applied as the loop applies it, and the next call
        starts behind it with the new cu."""
        n_old = len(self.kfs) - 1
        i = 0
        while i < n_old:
            cu = np.flatnonzero(new_kf.pt3d < 0).astype(np.int32)
            if len(cu) < 2:
                break
            js, pus = [], []
            for j in range(i, n_old):
                pu = np.flatnonzero(self.kfs[j].pt3d < 0).astype(np.int32)
                if len(pu) >= 2:
                    js.append(j)
                    pus.append(pu)
            if not js:
                break
            R0s = np.stack([_R(self.kfs[j].rot) for j in js])
            t0s = np.stack([self.kfs[j].t for j in js])
            slots0 = [self.kfs[j].slot for j in js]
            first, m0, m1, Xf, n_kept, n_matched = self.matcher.pair_points_first(
                slots0, pus, new_kf.slot, cu, K, R0s, t0s, K, R1, new_kf.t, MAX_REPR_ERR)
            self.map_log.append({"frame": new_kf.no, "slots0": slots0, "slot1": new_kf.slot, "idx0": pus, "idx1": cu,
                                 "K": np.array(K, np.float64), "R0s": R0s, "t0s": t0s, "R1": R1.copy(),
                                 "t1": new_kf.t.copy(), "first": first, "m0": m0, "m1": m1, "X": Xf,
                                 "n_kept": n_kept, "n_matched": n_matched})
            if first < 0:
                break
            self._add_pair_points(js[first], new_kf, pus[first][m0], cu[m1], Xf)
            i = js[first] + 1

    def _add_pair_points(self, i: int, new_kf: _Frame, p2, c2, Xf) -> None:
        """The new points Xf of older keyframe i's rows p2 and the new
        keyframe's rows c2 into the map (CSfM.cpp:178-227)."""
        K, kf = self.K, self.kfs[i]
        idx = self.map.addNewPoints(Xf, p2.reshape(1, -1), [kf.no])
        kf.pt3d[p2] = idx
        self.map.addKeyframeRows(self.matcher, kf.slot, kf.no, idx, p2, with_observations=False)
        # re-find the new points in the keyframes in between (CSfM.cpp:189-221)
        for j in range(i + 1, len(self.kfs) - 1):
            kj = self.kfs[j]
            uj = np.flatnonzero(kj.pt3d < 0).astype(np.int32)
            if len(uj) < 2:
                continue
            near_kf = abs(kj.no - kf.no) < abs(kj.no - new_kf.no)
            q0, q1 = self.matcher.refind_points(kf.slot if near_kf else new_kf.slot, p2 if near_kf else c2, Xf, K,
                                                _R(kj.rot), kj.t, kj.slot, uj, 0.8, 0.0, MAX_REPR_ERR)
            if len(q0):
                self.map.addKeyframeRows(self.matcher, kj.slot, kj.no, idx[q0], uj[q1])
                kj.pt3d[uj[q1]] = idx[q0]
        self.map.addKeyframeRows(self.matcher, new_kf.slot, new_kf.no, idx, c2)
        new_kf.pt3d[c2] = idx
        self.stats["new_points"] += len(idx)

    def _bundle_adjust(self) -> None:
        """CSfM::bundleAdjustment over all keyframes (CSfM.cpp:300-348): per
        keyframe, CMap::getPointsInFrame on the device map store, parameter
        blocks deduplicated first-seen, one-shot sfm_ba_solve, write-back."""
        uv, cam, p3 = [], [], []
        per_frame = self.map.getPointsInFrameMulti([kf.no for kf in self.kfs])
        for c, kf in enumerate(self.kfs):
            a3, a2 = per_frame[c]
            # Deliberate departure from the reference: CSfM.cpp:331-340 appends
            # pts3d and pts2d over ALL frames and pairs them globally, so after
            # a point matched twice in one keyframe (getPointsInFrame emits k^2
            # 2D indices, CMap.cpp:225-240) every later observation is paired
            # with a shifted 2D point and CTracker.cpp:676-677 reads camIdx[i]
            # past its end (undefined behaviour).  Here every observation is
            # paired with its own 2D index (pair_frame_observations).
            i2 = pair_frame_observations(a3, a2)
            uv.append(kf.pts[i2])
            cam.append(np.full(len(a3), c, np.int32))
            p3.append(a3)
        uv, cam, p3 = np.vstack(uv), np.concatenate(cam), np.concatenate(p3)
        if not len(p3):
            return
        # first-seen order of the gather (np.minimum.at: each point's first
        # entry; O(n) instead of np.unique's sort)
        n_e = len(p3)
        first = np.full(int(p3.max()) + 1, n_e, np.int64)
        np.minimum.at(first, p3, np.arange(n_e))
        seen = np.flatnonzero(first < n_e)
        order = seen[np.argsort(first[seen], kind="stable")]
        remap = np.empty(int(order.max()) + 1, np.int32)
        remap[order] = np.arange(len(order), dtype=np.int32)
        pt = remap[p3]
        X = self.map.getPointsAtIdx(order)
        C = len(self.kfs)
        rot = np.stack([f.rot for f in self.kfs])
        t = np.stack([f.t for f in self.kfs])
        K9 = np.tile(self.K.reshape(1, 9), (C, 1))
        rec = {"uv": uv.copy(), "cam_idx": cam.copy(), "pt_idx": pt.copy(), "K": K9, "rot": rot.copy(), "t": t.copy(),
               "X": X.copy()}
        t_s = time.perf_counter()
        sm, tr = _ba.solve(uv, cam, pt, K9, rot, t, X)
        self.times["ba_solve"] = self.times.get("ba_solve", 0.0) + time.perf_counter() - t_s
        self.stats["ba_iterations"] = self.stats.get("ba_iterations", 0) + sm.num_iterations
        rec.update({"summary": sm, "trace": tr, "rot_out": rot.copy(), "t_out": t.copy(), "X_out": X.copy()})
        self.ba_log.append(rec)
        for c, f in enumerate(self.kfs):
            f.rot, f.t = rot[c].copy(), t[c].copy()
        self.map.setPointsAtIdx(order, X)

    def close(self) -> None:
        if self._guidance is not None:
            self._guidance.close()
        self.matcher.close()
        self.map.close()
