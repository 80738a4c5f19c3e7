"""GPU: the camera front end (sfm_undistort_points, sfm_rgb_to_grey,
sfm_klt_push_frame_rgb, sfm_frame_detect, LiveSfM(camera=...)) against the
numpy restatement (tests/camera_ref.py) and against the composed calls it
replaces.  Every comparison is bitwise.  (Parity with OpenCV itself is
unpinned: it is not available to this project.)"""
import ctypes

import numpy as np
import pytest

from tests import camera_ref as R

pytestmark = pytest.mark.gpu

SIZE = (1280, 720)
LENS_CASES = ["L1", "L2", "L3", "L4", "none"]


def _camera(name, size=SIZE, K=None):
    from sfm_amd.camera import Camera
    d = () if name == "none" else R.LENSES[name]
    return Camera(R.k_for(size) if K is None else K, d, size), d


# ---- 1. sfm_undistort_points -------------------------------------------------

@pytest.mark.parametrize("name", LENS_CASES)
def test_undistort_points_bitwise(name):
    cam, d = _camera(name)
    rng = np.random.default_rng(11)
    for n in (0, 1, 63, 64, 65, 257, 4099):
        # inside and well outside the image; the principal point itself first
        p = rng.uniform([-200.0, -150.0], [SIZE[0] + 200.0, SIZE[1] + 150.0], (n, 2))
        if n:
            p[0] = cam.K[0, 2], cam.K[1, 2]
        got = cam.undistort(p)
        want = R.undistort_points(p, cam.K, d, cam.Kopt)
        assert got.shape == (n, 2)
        assert np.array_equal(got, want), (name, n, np.abs(got - want).max())
        if n:
            assert np.array_equal(got[0], [cam.Kopt[0, 2], cam.Kopt[1, 2]])  # r2 = 0


# ---- 2. sfm_rgb_to_grey ------------------------------------------------------

@pytest.mark.parametrize("w,h,stride", [(1, 1, 3), (3, 2, 9), (5, 3, 16), (64, 4, 192), (67, 5, 203),
                                        (1280, 2, 3840)])
def test_rgb_to_grey_bitwise(w, h, stride):
    import sfm_amd
    from sfm_amd._ffi import ptr
    rng = np.random.default_rng(w * 131 + h)
    for fill in ("random", 0, 255):
        buf = np.full(h * stride, 0xA5, np.uint8)          # poisoned row padding
        rows = buf.reshape(h, stride)
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8) if fill == "random" else np.full((h, w, 3), fill, np.uint8)
        if fill == "random" and h > 1:
            img[0], img[-1] = 0, 255                        # an all-0 and an all-255 row among them
        rows[:, :3 * w] = img.reshape(h, 3 * w)
        guard = 64
        out = np.full(h * w + guard, 0x5A, np.uint8)
        rc = sfm_amd.lib().sfm_rgb_to_grey(0, ptr(buf), w, h, stride, ptr(out))
        assert rc == 0
        assert np.array_equal(out[:h * w].reshape(h, w), R.rgb_to_grey(img)), (w, h, stride, fill)
        assert (out[h * w:] == 0x5A).all()
    # the Python wrapper (tight rows)
    from sfm_amd.camera import rgb_to_grey
    assert np.array_equal(rgb_to_grey(img), R.rgb_to_grey(img))


# ---- 3. sfm_klt_push_frame_rgb -----------------------------------------------

def _colour(grey):
    """3 channels with a different offset each (so the weights matter)."""
    return np.stack([np.clip(grey.astype(np.int32) + o, 0, 255).astype(np.uint8) for o in (0, 9, -7)], axis=-1)


@pytest.fixture(scope="module")
def video_frames():
    from sfm_amd.video import SyntheticVideo
    v = SyntheticVideo()
    return {k: v.frame(k) for k in (3, 4)}


def test_push_frame_rgb_equals_push_frame_of_the_grey(video_frames):
    from sfm_amd.klt import KLTTracker
    w, h = 160, 120
    a, b = KLTTracker(w, h), KLTTracker(w, h)
    try:
        for k in (3, 4):
            img = _colour(video_frames[k][300:300 + h, 500:500 + w])
            a.push_frame_rgb(img)
            b.push_frame(R.rgb_to_grey(img))
        assert a.num_levels == b.num_levels >= 2
        for which in (0, 1):
            for lv in range(a.num_levels):
                ia, da = a.level(which, lv)
                ib, db = b.level(which, lv)
                assert np.array_equal(ia, ib) and np.array_equal(da, db), (which, lv)
    finally:
        a.close()
        b.close()


# ---- 4 / 5. sfm_frame_detect -------------------------------------------------
# The crop was chosen on the CPU with oracle/brisk_oracle.py: frames 3 and 4 at
# [200:440, 400:720] give 620 / 646 detected, 239 / 252 described keypoints and
# 127 matches through the oracle alone.
CROP = (slice(200, 440), slice(400, 720))
FSIZE = (320, 240)


@pytest.fixture(scope="module")
def crop_frames(video_frames):
    from sfm_amd import brisk
    out = []
    for k in (3, 4):
        img3 = _colour(video_frames[k][CROP])
        grey = R.rgb_to_grey(img3)
        kp, lay, desc = brisk.detect(grey)
        n_detected = len(brisk.detect(grey, describe=False)[0])
        out.append(dict(img3=img3, grey=grey, kp=kp, lay=lay, desc=desc, n_detected=n_detected))
    return out


def _matches(m, n_prev, n_curr):
    sub_p = np.arange(0, n_prev, 2, dtype=np.int32)
    sub_c = np.arange(n_curr, dtype=np.int32)
    return [m.match_frames(distorted=True), m.match_frames(distorted=False), m.match_subset(sub_p, sub_c)]


@pytest.mark.parametrize("with_klt", [True, False])
@pytest.mark.parametrize("channels", [3, 1])
def test_frame_detect_equals_the_composed_calls(crop_frames, with_klt, channels):
    from sfm_amd.camera import FrameFrontEnd
    from sfm_amd.klt import KLTTracker
    from sfm_amd.matcher import FeatureMatcher
    cam, _ = _camera("L1", FSIZE)
    klt = KLTTracker(*FSIZE) if with_klt else None
    ref_klt = KLTTracker(*FSIZE) if with_klt else None
    handed, fed = FeatureMatcher(), FeatureMatcher()
    try:
        fe = FrameFrontEnd(cam, matcher=handed, klt=klt)
        for f in crop_frames:
            kps, lay, desc, pts = fe.detect(f["img3"] if channels == 3 else f["grey"])
            assert len(kps) >= 50 and f["n_detected"] > len(kps)   # the border rule dropped some
            assert np.array_equal(kps, f["kp"]) and np.array_equal(lay, f["lay"]) and np.array_equal(desc, f["desc"])
            und = cam.undistort(kps[:, :2].astype(np.float64))
            assert np.array_equal(pts, und)
            assert np.array_equal(pts, R.undistort_points(kps[:, :2].astype(np.float64), cam.K, cam.d, cam.Kopt))
            fed.push_frame(und, desc, kps[:, :2].astype(np.float64))
            if with_klt:
                ref_klt.push_frame(f["grey"])
        got = _matches(handed, *handed.n)
        want = _matches(fed, *fed.n)
        assert handed.n == fed.n
        assert len(want[0][0]) >= 10
        for (g0, g1), (w0, w1) in zip(got, want):
            assert np.array_equal(g0, w0) and np.array_equal(g1, w1)
        if with_klt:  # the frames became the handle's frames, pyramid and all
            for which in (0, 1):
                for lv in range(klt.num_levels):
                    for x, y in zip(klt.level(which, lv), ref_klt.level(which, lv)):
                        assert np.array_equal(x, y)
    finally:
        handed.close()
        fed.close()
        for k in (klt, ref_klt):
            if k is not None:
                k.close()


def test_frame_detect_without_handles(crop_frames):
    from sfm_amd.camera import FrameFrontEnd
    cam, _ = _camera("L1", FSIZE)
    f = crop_frames[0]
    kps, lay, desc, pts = FrameFrontEnd(cam).detect(f["img3"])
    assert np.array_equal(kps, f["kp"]) and np.array_equal(desc, f["desc"])
    assert np.array_equal(pts, cam.undistort(kps[:, :2].astype(np.float64)))


def test_frame_detect_short_capacity_leaves_the_matcher_alone(crop_frames):
    import sfm_amd
    from sfm_amd._ffi import ptr
    from sfm_amd.camera import FrameFrontEnd
    from sfm_amd.matcher import FeatureMatcher
    cam, _ = _camera("L1", FSIZE)
    m = FeatureMatcher()
    try:
        fe = FrameFrontEnd(cam, matcher=m)
        for f in crop_frames:
            fe.detect(f["img3"])
        before = _matches(m, *m.n)
        img = crop_frames[1]["img3"]
        n = len(crop_frames[1]["kp"])
        cap = n - 1
        kps, lay = np.zeros((cap, 5), np.float32), np.zeros(cap, np.int32)
        desc, pts = np.zeros((cap, 64), np.uint8), np.zeros((cap, 2))
        n_out = ctypes.c_int32()
        rc = sfm_amd.lib().sfm_frame_detect(m._h, None, ptr(img), 3, 3 * FSIZE[0], ctypes.byref(cam._c), 60, 6, cap,
                                            ptr(kps), ptr(lay), ptr(desc), ptr(pts), ctypes.byref(n_out))
        assert rc == -22 and n_out.value == n
        after = _matches(m, *m.n)
        assert len(before[0][0]) >= 10
        for (g0, g1), (w0, w1) in zip(after, before):
            assert np.array_equal(g0, w0) and np.array_equal(g1, w1)
    finally:
        m.close()


def test_frame_detect_rejects_mismatched_handles(crop_frames):
    import sfm_amd
    from sfm_amd._ffi import ptr
    from sfm_amd.klt import KLTTracker
    from sfm_amd.matcher import FeatureMatcher
    cam, _ = _camera("L1", FSIZE)
    img = crop_frames[0]["img3"]
    cap = 1024
    kps, lay = np.zeros((cap, 5), np.float32), np.zeros(cap, np.int32)
    desc, pts = np.zeros((cap, 64), np.uint8), np.zeros((cap, 2))
    n_out = ctypes.c_int32()

    def call(mt, klt, channels=3):
        return sfm_amd.lib().sfm_frame_detect(mt, klt, ptr(img), channels, 3 * FSIZE[0], ctypes.byref(cam._c), 60, 6,
                                              cap, ptr(kps), ptr(lay), ptr(desc), ptr(pts), ctypes.byref(n_out))
    m32, klt = FeatureMatcher(desc_bytes=32), KLTTracker(FSIZE[0] + 16, FSIZE[1])
    try:
        assert call(m32._h, None) == -22      # descriptor width
        assert call(None, klt._h) == -22      # frame size
        assert call(None, None, channels=2) == -22
    finally:
        m32.close()
        klt.close()


# ---- 6. the live loop --------------------------------------------------------

def _log_equal(a, b):
    assert len(a) == len(b)
    for ra, rb in zip(a, b):
        for key in ("uv", "cam_idx", "pt_idx", "K", "rot", "t", "X", "rot_out", "t_out", "X_out"):
            assert np.array_equal(ra[key], rb[key]), key
        assert ra["summary"].final_cost == rb["summary"].final_cost
        assert ra["summary"].num_iterations == rb["summary"].num_iterations


def test_live_loop_with_a_camera_equals_the_undistorted_feed():
    """LiveSfM(camera) on distorted detector output against a loop without a
    camera fed camera.undistort(pts), K = Kopt: the shortest run that reaches
    the second BA (keyframes 0, 5, 15)."""
    from sfm_amd.live import KeypointStream, LiveSfM
    st = KeypointStream(dist=R.LENSES["L1"])
    cam = st.camera
    assert np.array_equal(st.K, cam.Kopt) and not np.array_equal(cam.Kopt, cam.K)
    a, b = LiveSfM(st, camera=cam), LiveSfM(st)
    try:
        for k in range(16):
            pts, desc, _ = st.frame(k)
            a.process(k, pts, desc)
            b.process(k, cam.undistort(pts), desc)
        assert len(a.ba_log) == 2 and a.stats["tracked"] == 10 and a.lost == 0
        assert a.stats == b.stats
        _log_equal(a.ba_log, b.ba_log)
        # the keypoints really were distorted: the feed differs from what the loop used
        assert np.abs(st.frame(15)[0] - a.prev.pts).max() > 1.0
        assert np.array_equal(a.prev.ptsd, st.frame(15)[0])
    finally:
        a.close()
        b.close()


def test_process_image_equals_process_on_the_brisk_video():
    """process_image (one device call per frame, resident hand-off) against
    process fed by the composed detector + undistortion: the shortest run
    that reaches the first BA (keyframes 0 and 5)."""
    from sfm_amd import brisk
    from sfm_amd.camera import Camera
    from sfm_amd.live import BriskVideoStream, LiveSfM
    from sfm_amd.video import SyntheticVideo
    st = BriskVideoStream(SyntheticVideo(640, 360, speed=2.0))
    cam = Camera(st.K, R.LENSES["L1"], (640, 360))
    a, b = LiveSfM(st, camera=cam), LiveSfM(st, camera=cam)
    try:
        for k in range(6):
            img3 = _colour(st.video.frame(k))
            a.process_image(k, img3)
            kp, _, desc = brisk.detect(R.rgb_to_grey(img3), st.threshold, st.octaves)
            b.process(k, kp[:, :2].astype(np.float64), desc)
        assert len(a.ba_log) == 1 and a.stats["new_points"] > 50
        assert a.stats == b.stats
        _log_equal(a.ba_log, b.ba_log)
        assert a.matcher.n[1] == b.matcher.n[1] == len(b.prev.pts)
    finally:
        a.close()
        b.close()
