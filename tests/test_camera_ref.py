"""CPU: properties of the camera front end's restatement (tests/camera_ref.py)
that do not depend on the restatement being right by construction, and
sfm_camera_init (host only) against it, bit for bit.  OpenCV is not available:
parity with it is unpinned."""
import ctypes

import numpy as np
import pytest

from tests import camera_ref as R

L123 = ["L1", "L2", "L3"]


def _uniform_pixels(n=4096, size=(1280, 720), seed=0xCA3E7A):
    rng = np.random.default_rng(seed)
    return rng.uniform([0.0, 0.0], [float(size[0]), float(size[1])], (n, 2))


def _round_trip(name, iters):
    size = (1280, 720)
    d = R.LENSES[name]
    Kopt = R.optimal_new_camera_matrix(R.K_MAIN, d, size)
    p = _uniform_pixels()
    back = R.distort_points(R.undistort_points(p, R.K_MAIN, d, Kopt, iters), Kopt, d, R.K_MAIN)
    return float(np.abs(back - p).max())


@pytest.mark.parametrize("name", ["L1", "L2"])
def test_round_trip_below_a_millipixel(name):
    # measured with this algorithm: 1.8e-4 px (L1) and 8.5e-4 px (L2)
    err = _round_trip(name, 5)
    print(name, "round trip", err)
    assert err < 1e-3


@pytest.mark.parametrize("name", L123)
def test_fifth_iteration_still_improves(name):
    e4, e5 = _round_trip(name, 4), _round_trip(name, 5)
    print(name, "4 iterations", e4, "5 iterations", e5)
    assert e5 < e4


@pytest.mark.parametrize("size", R.SIZES)
@pytest.mark.parametrize("name", L123)
def test_border_of_the_new_image_is_valid_pixels(name, size):
    # alpha = 0: every pixel of the Kopt image comes from inside the source
    # image; the largest excursion measured is 0.031 px (the 9 x 9 grid is
    # coarser than the border's curvature)
    W, H = size
    d, K = R.LENSES[name], R.k_for(size)
    Kopt = R.optimal_new_camera_matrix(K, d, size)
    t = np.linspace(0.0, 1.0, 801)
    z = np.zeros_like(t)
    border = np.concatenate([np.stack([t * (W - 1), z], 1), np.stack([t * (W - 1), z + (H - 1)], 1),
                             np.stack([z, t * (H - 1)], 1), np.stack([z + (W - 1), t * (H - 1)], 1)])
    q = R.distort_points(border, Kopt, d, K)
    exc = max(0.0, float(-q.min()), float((q[:, 0] - W).max()), float((q[:, 1] - H).max()))
    print(name, size, "excursion", exc)
    assert exc < 0.05


@pytest.mark.parametrize("size", R.SIZES)
def test_zero_distortion_is_not_the_identity(size):
    W, H = size
    K = R.k_for(size)
    Kopt = R.optimal_new_camera_matrix(K, (), size)
    want = np.array([(W - 1) / W * K[0, 0], (H - 1) / H * K[1, 1], (W - 1) / W * K[0, 2], (H - 1) / H * K[1, 2]])
    got = np.array([Kopt[0, 0], Kopt[1, 1], Kopt[0, 2], Kopt[1, 2]])
    assert np.all(np.abs(got - want) <= 1e-5 * np.abs(want)), (got, want)
    assert Kopt[0, 1] == 0 and Kopt[1, 0] == 0 and Kopt[2, 2] == 1 and not np.array_equal(Kopt, K)


def test_grey_conversion_weights():
    v = np.arange(256, dtype=np.uint8)
    assert np.array_equal(R.rgb_to_grey(np.stack([v, v, v], axis=-1)), v)
    unit = np.zeros((3, 3), np.uint8)
    unit[np.arange(3), np.arange(3)] = 255
    g = R.rgb_to_grey(unit).astype(int)
    # the first channel in memory takes 4899, the last 1868
    assert g[1] > g[0] > g[2], g
    assert list(g) == [(255 * c + 8192) >> 14 for c in (4899, 9617, 1868)]


# ---- sfm_camera_init (host arithmetic, no GPU) -----------------------------

def _init(K, d, size):
    import sfm_amd
    from sfm_amd._ffi import CameraStruct, ptr
    K9 = np.ascontiguousarray(np.asarray(K, np.float64).reshape(9))
    dd = np.ascontiguousarray(np.asarray(d, np.float64).reshape(-1))
    c = CameraStruct()
    rc = sfm_amd.lib().sfm_camera_init(ctypes.byref(c), ptr(K9), ptr(dd) if dd.size else None, dd.size,
                                       size[0], size[1])
    return rc, c


@pytest.mark.parametrize("size", R.SIZES)
@pytest.mark.parametrize("name", ["L1", "L2", "L3", "L4"])
def test_camera_init_equals_the_restatement(name, size):
    K, d = R.k_for(size), R.LENSES[name]
    rc, c = _init(K, d, size)
    assert rc == 0
    assert np.array_equal(np.array(c.Kopt9).reshape(3, 3), R.optimal_new_camera_matrix(K, d, size))
    assert np.array_equal(np.array(c.K9).reshape(3, 3), K)
    assert list(c.d) == list(R.coeffs(d)) and c.n_d == len(d) and (c.width, c.height) == size


def test_camera_class_matches_and_distorts_back():
    from sfm_amd.camera import Camera
    d = R.LENSES["L1"]
    cam = Camera(R.K_MAIN, d, (1280, 720))
    assert np.array_equal(cam.Kopt, R.optimal_new_camera_matrix(R.K_MAIN, d, (1280, 720)))
    p = _uniform_pixels(64)
    assert np.array_equal(cam.distort(p), R.distort_points(p, cam.Kopt, d, R.K_MAIN))


def test_camera_init_rejects_bad_input():
    K, d = R.K_MAIN, list(R.LENSES["L1"])
    size = (1280, 720)
    assert _init(K, d, size)[0] == 0
    for n_d in (1, 2, 3, 6, 7, 9, 12, -1):
        import sfm_amd
        from sfm_amd._ffi import CameraStruct, ptr
        K9 = np.ascontiguousarray(K.reshape(9))
        dd = np.zeros(16)
        assert sfm_amd.lib().sfm_camera_init(ctypes.byref(CameraStruct()), ptr(K9), ptr(dd), n_d, 1280, 720) == -22
    for bad in (np.nan, np.inf):
        Kb = K.copy()
        Kb[0, 2] = bad
        assert _init(Kb, d, size)[0] == -22
        assert _init(K, [bad] + d[1:], size)[0] == -22
    for i in (0, 1):
        for v in (0.0, -5.0):
            Kb = K.copy()
            Kb[i, i] = v
            assert _init(Kb, d, size)[0] == -22
    assert _init(K, d, (1, 720))[0] == -22 and _init(K, d, (1280, 1))[0] == -22


def test_device_calls_validate_before_touching_the_device():
    import sfm_amd
    from sfm_amd._ffi import ptr
    L = sfm_amd.lib()
    _, c = _init(R.K_MAIN, R.LENSES["L1"], (1280, 720))
    # n = 0 succeeds with no device at all
    assert L.sfm_undistort_points(0, ctypes.byref(c), 0, None, None) == 0
    p = np.zeros((4, 2))
    assert L.sfm_undistort_points(0, ctypes.byref(c), 4, ptr(p), None) == -22
    assert L.sfm_undistort_points(0, None, 4, ptr(p), ptr(p)) == -22
    c.n_d = 3
    assert L.sfm_undistort_points(0, ctypes.byref(c), 4, ptr(p), ptr(p)) == -22
    rgb, g = np.zeros((2, 3, 3), np.uint8), np.zeros((2, 3), np.uint8)
    assert L.sfm_rgb_to_grey(0, ptr(rgb), 3, 2, 8, ptr(g)) == -22   # stride < 3 * w
    assert L.sfm_rgb_to_grey(0, None, 3, 2, 9, ptr(g)) == -22
