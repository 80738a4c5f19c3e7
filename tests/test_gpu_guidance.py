"""GPU: the scan guidance (sfm_guidance_*, ScanGuidance, LiveSfM(guidance=True))
against the numpy restatement (tests/guidance_ref.py).  Planes, counts, area
and box are compared bitwise; the centroid within the bound on the difference
of two fp64 summation orders.  (Parity with OpenCV itself is unpinned: it is
not available to this project.)"""
import ctypes

import numpy as np
import pytest

from tests import guidance_cases as C
from tests import guidance_ref as G

pytestmark = pytest.mark.gpu

SIZES = [(8, 8), (13, 9), (64, 36), (67, 37), (260, 132)]
COUNTS = [0, 1, 2, 3, 65, 1000]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _check(sg, res, o, X, what=""):
    """One update's result and planes against the restatement's record."""
    pl = sg.planes()
    for key in ("mask", "bins", "extents"):
        assert np.array_equal(pl[key], o[key]), (what, key)
    assert np.array_equal(_bits(pl["hist"]), _bits(o["hist"])), (what, "hist")
    assert np.array_equal(_bits(pl["bproj"]), _bits(o["bproj"])), (what, "bproj")
    assert res.area == o["area"], (what, res.area, o["area"])
    got = (res.n_points, res.n_projected, res.n_hull, res.n_accepted)
    assert got == (o["n_points"], o["n_projected"], o["n_hull"], o["n_accepted"]), (what, got)
    assert np.array_equal(_bits(res.box), _bits(o["box"])), (what, res.box, o["box"])
    n = len(X)
    if n == 0:
        assert np.isnan(res.centroid).all(), what
    else:
        bound = 2 * (n - 1) * 2.0 ** -53 * np.abs(X).mean(axis=0)
        assert (np.abs(res.centroid - o["centroid"]) <= bound).all(), (what, res.centroid - o["centroid"], bound)


@pytest.mark.parametrize("W,H", SIZES)
def test_planes_and_results_equal_the_restatement(W, H):
    from sfm_amd import ScanGuidance
    img = C.textured_frame(W, H, W + H)
    R, t, K = C.camera_for(W, H)
    sg = ScanGuidance(W, H)
    try:
        assert sg.small == G.small_size((W, H))
        for n in COUNTS:
            X = C.point_set(n, W, H, 100 + n)
            o = G.calculate_mask(img, X, R, t, K)
            _check(sg, sg.update(img, R, t, K, points=X), o, X, (W, H, n))
            if n == 1000:
                assert 0 < o["n_projected"] < n and o["n_hull"] >= 3 and o["mask"].sum() > 0
            if n == 3:
                assert o["n_hull"] == 2 and o["area"] == 0.0
        # padded rows (stride > 3 W), poisoned padding
        wide = np.full((H, 3 * W + 7), 0xA5, np.uint8)
        wide[:, :3 * W] = img.reshape(H, 3 * W)
        view = wide[:, :3 * W].reshape(H, W, 3)
        assert view.strides[0] == 3 * W + 7
        _check(sg, sg.update(view, R, t, K, points=X), o, X, (W, H, "stride"))
    finally:
        sg.close()


def test_full_size_frame_with_6000_points():
    from sfm_amd import ScanGuidance
    W, H = 1280, 720
    img = C.textured_frame(W, H, 9)
    R, t, K = C.camera_for(W, H)
    X = C.point_set(6000, W, H, 4)
    o = G.calculate_mask(img, X, R, t, K)
    assert o["n_projected"] > 5000 and o["n_hull"] >= 6 and o["n_accepted"] > 1000
    a, b = ScanGuidance(W, H), ScanGuidance(W, H)
    try:
        ra = a.update(img, R, t, K, points=X)
        _check(a, ra, o, X, "1280x720")
        # two handles fed the same input, and the same handle fed twice: identical bits
        rb = b.update(img, R, t, K, points=X)
        rc = a.update(img, R, t, K, points=X)
        pa, pb = a.planes(), b.planes()
        for r in (rb, rc):
            assert np.array_equal(r.centroid.view(np.uint64), ra.centroid.view(np.uint64))
            assert np.array_equal(_bits(r.box), _bits(ra.box)) and r.area == ra.area
            assert (r.n_points, r.n_projected, r.n_hull, r.n_accepted) == (ra.n_points, ra.n_projected, ra.n_hull,
                                                                          ra.n_accepted)
        for key in pa:
            assert np.array_equal(pa[key].view(np.uint8), pb[key].view(np.uint8)), key
    finally:
        a.close()
        b.close()


def test_histogram_too_large_for_lds_takes_the_global_path():
    from sfm_amd import ScanGuidance
    W, H = 67, 37
    img = C.textured_frame(W, H, 21)
    R, t, K = C.camera_for(W, H)
    X = C.point_set(65, W, H, 8)
    for hb, sb in ((200, 100), (128, 64), (1, 1), (256, 255)):     # 8192 bins: the last LDS size
        sg = ScanGuidance(W, H, h_bins=hb, s_bins=sb)
        try:
            o = G.calculate_mask(img, X, R, t, K, h_bins=hb, s_bins=sb)
            _check(sg, sg.update(img, R, t, K, points=X), o, X, (hb, sb))
        finally:
            sg.close()


def test_flat_two_colour_frame_gives_the_derived_box():
    from sfm_amd import ScanGuidance
    img, X, R, t, K = C.flat_case()
    sg = ScanGuidance(128, 72)
    try:
        res = sg.update(img, R, t, K, points=X)
        assert np.array_equal(res.box_center, [66.0, 30.0]) and sorted(res.box_size.tolist()) == [28.0, 52.0]
        assert (res.n_projected, res.n_hull, res.n_accepted, res.area) == (len(X), 4, 112, 50.0)
        acc = np.zeros((18, 32), bool)
        acc[4:12, 10:24] = True
        assert np.array_equal(sg.planes()["extents"], G.row_extents(acc))
        _check(sg, res, G.calculate_mask(img, X, R, t, K), X, "flat")
    finally:
        sg.close()


def test_ema_state_and_replacement_over_four_frames():
    from sfm_amd import ScanGuidance
    W, H = 64, 36
    R, t, K = C.camera_for(W, H)
    frames = [C.textured_frame(W, H, 40 + i) for i in range(4)]
    sets = [C.point_set(65, W, H, 50 + i) for i in range(4)]
    ema, rep = ScanGuidance(W, H, ema=1), ScanGuidance(W, H)
    ref_ema, ref_rep = G.ScanGuidanceRef(ema=1), G.ScanGuidanceRef()
    try:
        for i, (img, X) in enumerate(zip(frames, sets)):
            o = ref_ema.calculate_mask(img, X, R, t, K)
            _check(ema, ema.update(img, R, t, K, points=X), o, X, ("ema", i))
            if i:
                assert not np.array_equal(o["hist"], o["frame_hist"])
            o = ref_rep.calculate_mask(img, X, R, t, K)
            assert np.array_equal(o["hist"], G.calculate_mask(img, X, R, t, K)["frame_hist"])   # the single shot
            _check(rep, rep.update(img, R, t, K, points=X), o, X, ("replace", i))
    finally:
        ema.close()
        rep.close()


def test_map_path_equals_the_live_points_in_ascending_index():
    from sfm_amd import DeviceMap, ScanGuidance
    W, H = 260, 132
    img = C.textured_frame(W, H, 3)
    R, t, K = C.camera_for(W, H)
    X = C.point_set(700, W, H, 6)
    dm, a, b = DeviceMap(), ScanGuidance(W, H), ScanGuidance(W, H)
    try:
        # an empty map: NaN centroid, the zero box
        r0 = a.update(img, R, t, K, map=dm)
        assert np.isnan(r0.centroid).all() and r0.n_points == 0 and np.array_equal(r0.box, np.zeros(5, np.float32))
        rng = np.random.default_rng(12)
        idx = np.concatenate([dm.addNewPoints(X[:400], rng.integers(0, 900, (2, 400)), [0, 5]),
                              dm.addNewPoints(X[400:], rng.integers(0, 900, (2, 300)), [5, 9])])
        assert idx.tolist() == list(range(700))
        live = np.ones(700, bool)
        for gone in (np.sort(rng.choice(700, 150, replace=False)), np.array([0, 699])):
            gone = gone[live[gone]]
            dm.removePoints(gone)
            live[gone] = False
            ra = a.update(img, R, t, K, map=dm)
            rb = b.update(img, R, t, K, points=X[live])
            assert ra.n_points == dm.getNPoints() == int(live.sum())
            # (removed points keep their slots, so the two sums associate differently)
            bound = 2 * (ra.n_points - 1) * 2.0 ** -53 * np.abs(X[live]).mean(axis=0)
            assert (np.abs(ra.centroid - rb.centroid) <= bound).all()
            assert np.array_equal(_bits(ra.box), _bits(rb.box)) and ra.area == rb.area
            assert (ra.n_projected, ra.n_hull, ra.n_accepted) == (rb.n_projected, rb.n_hull, rb.n_accepted)
            pa, pb = a.planes(), b.planes()
            for key in pa:
                assert np.array_equal(pa[key].view(np.uint8), pb[key].view(np.uint8)), key
        _check(a, ra, G.calculate_mask(img, X[live], R, t, K), X[live], "map")
    finally:
        a.close()
        b.close()
        dm.close()


def test_every_invalid_argument_is_rejected_on_the_host():
    import sfm_amd
    from sfm_amd import DeviceMap, ScanGuidance
    from sfm_amd._ffi import GuidanceOptions, GuidanceResult, default_guidance_options, ptr
    L = sfm_amd.lib()
    W, H = 64, 36
    img = C.textured_frame(W, H, 1)
    R, t, K = C.camera_for(W, H)
    R9, t3, K9 = np.ascontiguousarray(R.reshape(9)), np.ascontiguousarray(t), np.ascontiguousarray(K.reshape(9))
    X = np.ascontiguousarray(C.point_set(65, W, H, 2))
    # create
    h = ctypes.c_void_p()
    for w_, h_, hb, sb in ((7, 36, 60, 50), (64, 7, 60, 50), (64, 36, 0, 50), (64, 36, 60, 257), (64, 36, 257, 50),
                           (64, 36, 60, 0)):
        o = default_guidance_options()
        o.h_bins, o.s_bins = hb, sb
        assert L.sfm_guidance_create(0, w_, h_, ctypes.byref(o), ctypes.byref(h)) == -22 and not h.value
    assert L.sfm_guidance_create(0, W, H, None, None) == -22
    sg, dm = ScanGuidance(W, H), DeviceMap()
    try:
        dm.addNewPoints(X, np.zeros((1, len(X)), np.int32), [0])
        res = GuidanceResult()
        good = sg.update(img, R, t, K, points=X)

        def still_fine():
            r = sg.update(img, R, t, K, map=dm)
            assert np.array_equal(_bits(r.box), _bits(good.box)) and r.n_accepted == good.n_accepted
            r = sg.update(img, R, t, K, points=X)
            assert np.array_equal(_bits(r.box), _bits(good.box)) and r.n_accepted == good.n_accepted

        def bad(v, i):
            w = v.copy()
            w[i] = np.nan if i % 2 else np.inf
            return w
        args = dict(h=sg._h, map=dm._h, img=ptr(img), stride=3 * W, R=ptr(R9), t=ptr(t3), K=ptr(K9),
                    out=ctypes.byref(res))
        keep = []
        cases = [dict(h=None), dict(img=None), dict(R=None), dict(t=None), dict(K=None), dict(out=None),
                 dict(stride=3 * W - 1), dict(stride=0), dict(stride=-3 * W)]
        for name, v in (("R", R9), ("t", t3), ("K", K9)):
            for i in range(len(v)):
                keep.append(bad(v, i))
                cases.append({name: ptr(keep[-1])})
        for c in cases:
            a = {**args, **c}
            assert L.sfm_guidance_update(a["h"], a["map"], a["img"], a["stride"], a["R"], a["t"], a["K"],
                                         a["out"]) == -22, c
            assert L.sfm_guidance_update_points(a["h"], len(X), ptr(X), a["img"], a["stride"], a["R"], a["t"],
                                                a["K"], a["out"]) == -22, c
            assert L.sfm_last_error()
        still_fine()
        a = args
        assert L.sfm_guidance_update(a["h"], None, a["img"], a["stride"], a["R"], a["t"], a["K"], a["out"]) == -22
        assert L.sfm_guidance_update_points(a["h"], 5, None, a["img"], a["stride"], a["R"], a["t"], a["K"],
                                            a["out"]) == -22
        assert L.sfm_guidance_update_points(a["h"], -1, ptr(X), a["img"], a["stride"], a["R"], a["t"], a["K"],
                                            a["out"]) == -22
        still_fine()
        if sfm_amd.device_count() >= 2:      # the map and the handle on different devices
            other = DeviceMap(device=1)
            try:
                other.addNewPoints(X, np.zeros((1, len(X)), np.int32), [0])
                assert L.sfm_guidance_update(a["h"], other._h, a["img"], a["stride"], a["R"], a["t"], a["K"],
                                             a["out"]) == -22
            finally:
                other.close()
            still_fine()
        # the Python wrapper's own checks
        with pytest.raises(ValueError):
            sg.update(img, R, t, K)
        with pytest.raises(ValueError):
            sg.update(img[:, :, 0], R, t, K, points=X)
        with pytest.raises(TypeError):
            ScanGuidance(W, H, bins=3)
    finally:
        sg.close()
        dm.close()


def _colour(grey):
    return np.stack([np.clip(grey.astype(np.int32) + o, 0, 255).astype(np.uint8) for o in (0, 9, -7)], axis=-1)


def test_live_loop_with_guidance():
    """LiveSfM(guidance=True).process_image against a stand-alone ScanGuidance
    fed the same (image, pose, map state) sequence by a loop without
    guidance, which must also compute exactly what the guided loop computes."""
    from tests import camera_ref
    from sfm_amd import ScanGuidance
    from sfm_amd.camera import Camera
    from sfm_amd.live import BriskVideoStream, LiveSfM, _R
    from sfm_amd.video import SyntheticVideo
    st = BriskVideoStream(SyntheticVideo(640, 360, speed=2.0))
    cam = Camera(st.K, camera_ref.LENSES["L1"], (640, 360))
    with pytest.raises(ValueError):
        LiveSfM(st, guidance=True)                       # no camera
    a, b = LiveSfM(st, camera=cam, guidance=True), LiveSfM(st, camera=cam)
    alone = ScanGuidance(640, 360)
    try:
        with pytest.raises(ValueError):
            a.process_image(0, st.video.frame(0))        # a grey frame
        assert a.stats["frames"] == 0 and "guidance" in a.times and "guidance" not in b.times
        want, prev_img = [], None
        for k in range(15):
            img3 = _colour(st.video.frame(k))
            running = len(b.kfs) >= 2
            a.process_image(k, img3)
            b.process_image(k, img3)
            if b.prev.no == k:
                prev_img = img3
            if running:
                want.append(alone.update(prev_img, _R(b.prev.rot), b.prev.t, b.K, map=b.map))
                assert a.guidance is a.guidance_log[-1]
        assert len(want) == len(a.guidance_log) >= 8 and b.guidance is None and b.guidance_log == []
        for g, w in zip(a.guidance_log, want):
            assert np.array_equal(g.centroid.view(np.uint64), w.centroid.view(np.uint64))
            assert np.array_equal(_bits(g.box), _bits(w.box)) and g.area == w.area
            assert (g.n_points, g.n_projected, g.n_hull, g.n_accepted) == (w.n_points, w.n_projected, w.n_hull,
                                                                          w.n_accepted)
        assert a.guidance_log[-1].n_points == a.map.getNPoints() > 50
        assert a.guidance_log[-1].n_projected > 20 and a.guidance_log[-1].n_accepted > 0
        # guidance changes nothing else
        assert a.stats == b.stats and len(a.ba_log) == len(b.ba_log) >= 1
        for ra, rb in zip(a.ba_log, b.ba_log):
            for key in ("uv", "cam_idx", "pt_idx", "K", "rot", "t", "X", "rot_out", "t_out", "X_out"):
                assert np.array_equal(ra[key], rb[key]), key
            assert ra["summary"].final_cost == rb["summary"].final_cost
        assert [f.no for f in a.kfs] == [f.no for f in b.kfs]
        for fa, fb in zip(a.kfs, b.kfs):
            assert np.array_equal(fa.rot, fb.rot) and np.array_equal(fa.t, fb.t) and np.array_equal(fa.pt3d, fb.pt3d)
        assert np.array_equal(a.prev.rot, b.prev.rot) and np.array_equal(a.prev.t, b.prev.t)
    finally:
        alone.close()
        a.close()
        b.close()
