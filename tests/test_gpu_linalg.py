"""GPU: the geometry kernels' small linear algebra (cv_linalg.h cv_svd /
cv_svd_at / cv_lstsq / qr_solve, the lane-parallel cv_svd_sweeps_lanes,
pnp_kernels.hip cv_svd12_lanes, tri_point.h) run through the testing hook
sfm_linalg_probe and through sfm_triangulate_points, held to

  * an extended-precision reference (tests/linalg_ref.py: one-sided Jacobi
    in longdouble, itself checked against mpmath), within caps that come from
    correct fp64 code alone (tests/linalg_cases.py, tests/test_linalg_ref.py);
  * the bit identities the code claims: the one-row-per-lane sweeps equal
    the sequential ones (variant 1 == variant 0), and the device equals the
    fp64 oracle written to the same operation order (oracle.pnp_oracle);
  * repeatability, and independence of the batch order.

Batches: 1, one workgroup, one workgroup + 1 and several workgroups (256-lane
workgroups for variant 0, three-wave workgroups for variant 1); adjacent
lanes and waves hold different problems (linalg_cases.deal).
"""
import numpy as np
import pytest

import linalg_cases as C
import linalg_ref as R
import map_points_ref as mref
from sfm_amd._ffi import LINALG_OPS, linalg_probe
from sfm_amd.mapping import triangulate_points
from sfm_amd.matcher import FeatureMatcher

pytestmark = pytest.mark.gpu

ALL_OPS = list(C.SVD_OPS) + ["svd12"] + list(C.LSTSQ_OPS) + ["qr6x4"]
OP_FAMILY = [(op, f) for op in ALL_OPS for f in C.families(op)]
BATCHES = {0: (1, 256, 257, 700), 1: (1, 3, 4, 100)}


def variants(op):
    return (1,) if op == "svd12" else (0, 1) if LINALG_OPS[op][3] else (0,)


def _bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


_RUNS = {}


def run(op, family, variant, n):
    """The device's output for the dealt batch of n problems (once per process)."""
    key = (op, family, variant, n)
    if key not in _RUNS:
        _RUNS[key] = linalg_probe(op, variant, C.problems(op, family)[C.deal(n)])
    return _RUNS[key]


@pytest.mark.parametrize("op,family", OP_FAMILY)
def test_within_caps_of_the_longdouble_reference(op, family):
    cap = C.caps(op, family)
    for v in variants(op):
        for n in BATCHES[v]:
            out, which = run(op, family, v, n), C.deal(n)
            assert np.isfinite(out).all(), (op, family, v, n)
            err = C.metrics(op, family, out, which)
            print(f"{op} {family} variant {v} batch {n}: " +
                  " ".join(f"{m} {err[m]:.2e}/{cap[m]:.2e}" for m in cap))
            for m in cap:
                assert err[m] <= cap[m], (op, family, v, n, m, err[m], cap[m])
            # no cross-talk: a problem's result does not depend on its slot
            first = {int(k): int(np.flatnonzero(which == k)[0]) for k in set(which.tolist())}
            assert _bits(out, out[[first[int(k)] for k in which]]), (op, family, v, n)


@pytest.mark.parametrize("op,family", [(o, f) for o in C.WAVE_OPS for f in C.families(o)])
def test_lane_variant_equals_sequential_variant_bitwise(op, family):
    """cv_svd_sweeps_lanes: "exactly the sequential rotation's values"."""
    for n in (4, 100):
        assert _bits(run(op, family, 1, n), linalg_probe(op, 0, C.problems(op, family)[C.deal(n)])), (op, family, n)


@pytest.mark.parametrize("op,family", OP_FAMILY)
def test_device_equals_the_fp64_oracle_bitwise(op, family):
    """The kernels and oracle.pnp_oracle follow one operation order, unfused."""
    want = C.oracle_out(op, family)
    for v in variants(op):
        n = BATCHES[v][2]
        out, which = run(op, family, v, n), C.deal(n)
        bad = [int(i) for i in range(n) if not _bits(out[i], want[which[i]])]
        if bad:
            i = bad[0]
            d = np.flatnonzero(out[i].view(np.uint64) != want[which[i]].view(np.uint64))
            pytest.fail(f"{op} {family} variant {v}: {len(bad)} of {n} slots differ; slot {i} (problem {which[i]}) "
                        f"entries {d[:6].tolist()} device {out[i][d[:3]].tolist()} oracle {want[which[i]][d[:3]].tolist()}")


# one family per op, and for the ops with such paths the completion of zero
# singular values (the RNG's state), the 12x12 slow path by a tie and by a
# zero, a dropped singular value and the eta == 0 return
ORDER_CASES = [(op, C.families(op)[0]) for op in ALL_OPS] + [(op, "rank2") for op in C.SVD_OPS] + \
    [("svd12", "zero"), ("svd12", "tie"), ("svd12", "epnp_planar"), ("lstsq6x4", "dropped"), ("lstsq6x5", "dropped"),
     ("qr6x4", "eta0")]


@pytest.mark.parametrize("op,family", ORDER_CASES)
def test_repeatable_and_independent_of_batch_order(op, family):
    for v in variants(op):
        n = BATCHES[v][3]
        data = C.problems(op, family)[C.deal(n)]
        a = run(op, family, v, n)
        assert _bits(a, linalg_probe(op, v, data))
        assert _bits(a[::-1], linalg_probe(op, v, data[::-1].copy()))


# ---- triangulation at the geometries where it goes wrong ----------------------
def _tri(scene, idx):
    s = C.tri_scene(scene)
    return triangulate_points(s["cam0"][idx], s["cam1"][idx], s["uv0"][idx], s["uv1"][idx], s["P"])


@pytest.mark.parametrize("scene", [s for s in C.TRI_SCENES if s != "same_cam"])
def test_triangulation_within_caps(scene):
    cap, y = C.tri_cap(scene)
    Xr, _, cond = C.tri_reference(scene)
    full = _tri(scene, np.arange(C.TRI_N))
    err = C.tri_error(scene, full)
    print(f"{scene}: device {err:.2e} cap {cap:.2e} (oracle {y['oracle']:.2e}, numpy {y['numpy']:.2e}); "
          f"worst relative error {float(np.max(R.rel_err(full, Xr))):.2e}, bitwise the oracle: "
          f"{_bits(full, C.tri_oracle(scene))}")
    assert np.isfinite(full).all() and err <= cap
    assert _bits(full, C.tri_oracle(scene))        # tri_point and the oracle: one operation order
    for n in (1, 255, 256, 257):
        assert _bits(_tri(scene, np.arange(n)), full[:n]), (scene, n)
    assert _bits(_tri(scene, np.arange(C.TRI_N)[::-1].copy()), full[::-1])


def test_triangulation_same_camera_equals_oracle_and_leaves_neighbours_alone():
    """cam0 == cam1: a two-dimensional null space, nothing to be right about;
    the device returns the oracle's bits (NaN and inf included), and a good
    point in the next lane is what it is without such neighbours."""
    idx = np.arange(C.TRI_N)
    got, want = _tri("same_cam", idx), C.tri_oracle("same_cam")
    assert _bits(got, want)
    good, bad = C.tri_scene("bd_1e-1"), C.tri_scene("same_cam")
    assert np.array_equal(good["P"], bad["P"])
    mix = lambda key: np.where((idx % 2 == 0).reshape((-1,) + (1,) * (good[key].ndim - 1)), good[key], bad[key])
    X = triangulate_points(mix("cam0"), mix("cam1"), mix("uv0"), mix("uv1"), good["P"])
    alone = _tri("bd_1e-1", idx)
    assert _bits(X[0::2], alone[0::2]) and _bits(X[1::2], got[1::2])


def test_pair_points_inherits_the_low_parallax_result():
    """sfm_matcher_pair_points on a baseline / depth = 1e-3 pair: its points
    are sfm_triangulate_points' bits and lie within the scene's cap."""
    s = C.tri_scene("bd_1e-3")
    n = 200
    p0, p1 = s["uv0"][:n].astype(np.float32), s["uv1"][:n].astype(np.float32)
    desc = np.random.default_rng(11).integers(0, 256, (n, 64), dtype=np.uint8)
    Kc, R1, t1 = s["K"], s["R1"], s["t1"]
    m = FeatureMatcher(64)
    try:
        m.store_keyframe(0, p0, desc)
        m.store_keyframe(1, p1, desc)
        i0, i1, X, nm = m.pair_points(0, np.arange(n), 1, np.arange(n), Kc, np.eye(3), np.zeros(3), Kc, R1, t1,
                                      1e9, min_distance=0.0)
    finally:
        m.close()
    assert nm == n and np.array_equal(i0, i1) and len(i0) > n // 2
    Pm = np.stack([mref.compose_P(Kc, np.eye(3), np.zeros(3)), mref.compose_P(Kc, R1, t1)])
    uv0, uv1 = p0[i0].astype(np.float64), p1[i1].astype(np.float64)
    c0, c1 = np.zeros(len(i0), np.int32), np.ones(len(i0), np.int32)
    assert _bits(X, triangulate_points(c0, c1, uv0, uv1, Pm))
    Xr, _, cond = R.ld_triangulate(Pm[c0], Pm[c1], uv0, uv1)
    assert float(np.max(R.rel_err(X, Xr) / cond)) <= C.tri_cap("bd_1e-3")[0]
