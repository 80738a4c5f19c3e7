"""CPU: the yardsticks of tests/test_gpu_linalg.py are themselves checked.

  * the longdouble reference (linalg_ref.ld_svd and what is built on it)
    against mpmath at 50 digits, on one problem of every op x family and a
    few points of every triangulation scene: at least 1000 x below every cap;
  * the caps come from correct fp64 code alone (the oracle's OpenCV
    restatement and LAPACK) and stay at rounding level;
  * no case sits where a rounding difference could flip a branch: no singular
    value within a factor 100 of cv_lstsq's threshold 2 eps sum(w), no W
    within a factor 100 of DBL_MIN unless it is exactly 0; every 12x12 case
    takes the path of cv_svd12_lanes it is listed for; every triangulation
    scene has the parallax and the homogeneous coordinate it is listed for;
    the beta-sign families put rotations with betas of opposite signs into
    one pass of the lane schedules (svd_schedule.h replayed: 6x4, 6x5, 12x12);
  * planted faults (a rotation skipped, -s for s on one entry, the sort not
    applied to Vt, the threshold 2 eps read as 2e-10, h from the wrong row)
    exceed the caps by a factor 1000 or more.
"""
import mpmath
import numpy as np
import pytest

import linalg_cases as C
import linalg_ref as R

LD = np.longdouble
ALL_OPS = list(C.SVD_OPS) + ["svd12"] + list(C.LSTSQ_OPS) + ["qr6x4"]
OP_FAMILY = [(op, f) for op in ALL_OPS for f in C.families(op)]
TRI_CAPPED = [s for s in C.TRI_SCENES if s != "same_cam"]


def _ld(x):
    return LD(mpmath.nstr(x, 30))


def _mp_svd(A):
    """mpmath.svd_r at 50 digits -> (sigma, U [M][N], V [N][N]) as longdouble."""
    with mpmath.workdps(50):
        M, N = A.shape
        U, S, Vt = mpmath.svd_r(mpmath.matrix([[mpmath.mpf(float(x)) for x in r] for r in A]))
        sig = np.array([_ld(S[i]) for i in range(N)])
        Um = np.array([[_ld(U[i, j]) for j in range(N)] for i in range(M)])
        Vm = np.array([[_ld(Vt[j, i]) for j in range(N)] for i in range(N)])
    return sig, Um, Vm


@pytest.mark.parametrize("op,family", OP_FAMILY)
def test_longdouble_reference_against_mpmath(op, family):
    cap = C.caps(op, family)
    pr = C.problems(op, family)[0]
    ref = C.reference(op, family)
    if op in C.SVD_OPS or op == "svd12":
        M, N = C.SVD_OPS.get(op, (12, 12))
        A = pr.reshape(M, N) if op != "svd12" else pr.reshape(12, 12).T
        mp = _mp_svd(A)
        sig, U, V = ref[0][0], ref[1][0].copy(), ref[2][0]
        # (the metrics never read the reference's left vectors of zero values)
        zero = sig <= R.ZERO_LD * sig[0]
        U[:, zero] = mp[1][:, zero]
        if op == "svd12":
            err = R.svd12_metrics(A, U.T[[11, 10, 9, 8]], mp)
        else:
            err = R.svd_metrics(A, sig, U.T, None if op == "svd_at9x7" else V.T, mp)
        if float(sig[-1]) <= R.ZERO_LD * float(sig[0]):
            err.pop("orthu")      # (the reference leaves the left vectors of zero values unset)
    else:
        N = C.LSTSQ_OPS.get(op, 4)
        A, b = pr[:6 * N].reshape(6, N), pr[6 * N:6 * N + 6]
        sig, U, V = _mp_svd(A)
        kept = ref[1][0] if op in C.LSTSQ_OPS else np.asarray(sig) > 0
        if op == "qr6x4" and not ref[1][0]:
            return                # (no solve: x stays x0)
        x = V[:, kept] @ ((U[:, kept].T @ b.astype(LD)) / sig[kept])
        err = {"x": float(R.rel_err(ref[0][0], x))}
    for m, e in err.items():
        assert e * 1000 <= cap[m], (op, family, m, e, cap[m])


@pytest.mark.parametrize("scene", TRI_CAPPED)
def test_triangulation_reference_against_mpmath(scene):
    s = C.tri_scene(scene)
    Xr, _, cond = C.tri_reference(scene)
    cap, _ = C.tri_cap(scene)
    As = R.tri_system(s["P"][s["cam0"]], s["P"][s["cam1"]], s["uv0"], s["uv1"])
    with mpmath.workdps(50):
        for i in (0, 1, 255, 256, 299):
            # the system itself in 50 digits from the fp64 inputs
            Pa, Pb = s["P"][s["cam0"][i]], s["P"][s["cam1"][i]]
            rows = []
            for (u, v), Pm in ((s["uv0"][i], Pa), (s["uv1"][i], Pb)):
                for c, r in ((u, 0), (v, 1)):
                    rows.append([mpmath.mpf(float(c)) * mpmath.mpf(float(Pm[2, k])) - mpmath.mpf(float(Pm[r, k]))
                                 for k in range(4)])
            _, _, Vt = mpmath.svd_r(mpmath.matrix(rows))
            X = np.array([_ld(Vt[3, k] / Vt[3, 3]) for k in range(3)])
            assert float(np.max(np.abs(As[i] - np.array([[_ld(x) for x in r] for r in rows])))) <= 1e-18 * 1e4
            assert float(R.rel_err(Xr[i], X) / cond[i]) * 1000 <= cap, (scene, i)


@pytest.mark.parametrize("op,family", OP_FAMILY)
def test_caps_come_from_the_yardsticks_and_stay_at_rounding_level(op, family):
    y, cap, fl = C.yardsticks(op, family), C.caps(op, family), C.floors(op, family)
    for m, c in cap.items():
        assert c == 8 * max(y["oracle"][m], y["numpy"][m]) + fl[m]
        assert np.isfinite(c)
        # a yardstick that went wrong would make the check vacuous
        if m in ("flag", "untouched"):
            assert c == 0.0
        elif m == "x":
            assert c <= 100 * fl[m] + 1e-13, (op, family, c, fl[m])
        else:
            assert c < 1e-13, (op, family, m, c)


@pytest.mark.parametrize("scene", TRI_CAPPED)
def test_triangulation_caps_and_scene_geometry(scene):
    cap, y = C.tri_cap(scene)
    assert cap == 8 * max(y.values()) + R.EPS and cap < 1e-13
    s = C.tri_scene(scene)
    Xr, h, cond = C.tri_reference(scene)
    assert s["uv0"].shape == (300, 2)
    # parallax: the angle between the two viewing rays of the true point
    r0, r1 = s["X"], s["X"] - s["C1"]
    cosp = (r0 * r1).sum(1) / np.linalg.norm(r0, axis=1) / np.linalg.norm(r1, axis=1)
    par = np.degrees(np.arccos(np.clip(cosp, -1, 1)))
    if scene.startswith(("bd_", "noise_")):
        assert s["ratio"] == float(scene.split("_")[1])
        assert 40 * s["ratio"] < par.max() < 80 * s["ratio"]          # 57.3 ratio degrees head on
        if scene == "bd_1e-4":
            assert par.min() < 0.006
        assert (s["noise"] == 0.3) == scene.startswith("noise_")
    if scene.startswith("bd_") or scene in ("wide_P", "behind", "h_tiny"):
        sig = R.ld_svd(R.tri_system(s["P"][s["cam0"]], s["P"][s["cam1"]], s["uv0"], s["uv1"]))[0]
        assert float((sig[:, 3] / sig[:, 0]).max()) < 1e-12           # noise-free: sigma_4 = 0 to rounding
    if scene == "wide_P":
        a = np.abs(s["P"][np.abs(s["P"]) > 0])
        assert a.min() <= 1.0 and a.max() >= 1e4
    if scene == "behind":
        z1 = (np.einsum("ij,nj->ni", s["P"][1], np.c_[s["X"], np.ones(300)]))[:, 2]
        assert (z1 < 0).all()
    if scene == "h_tiny":
        assert float(np.abs(h).max()) < 1.01e-6 and float(np.abs(h).min()) > 0.99e-6
    else:
        assert float(np.abs(h).min()) > 5e-5


def test_same_camera_scene_has_a_two_dimensional_null_space():
    s = C.tri_scene("same_cam")
    assert (s["cam0"] == s["cam1"]).all()
    sig = R.ld_svd(R.tri_system(s["P"][s["cam0"]], s["P"][s["cam1"]], s["uv0"], s["uv1"]))[0]
    assert float((sig[:, 2] / sig[:, 0]).max()) < 1e-15


@pytest.mark.parametrize("op,family", [(o, f) for o, f in OP_FAMILY if o != "qr6x4"])
def test_no_case_sits_on_a_branch(op, family):
    for k, row in enumerate(C.problems(op, family)):
        if op == "svd12":
            w = C.oracle_w12(family)[k]
        else:
            M, N = C.SVD_OPS.get(op, (6, C.LSTSQ_OPS.get(op, 0)))
            w = C.P.cv_svd(row[:M * N].reshape(M, N))[0]
        assert all(x == 0.0 or x > 100 * R.DBL_MIN for x in w), (op, family, k, w)
        if op in C.LSTSQ_OPS:
            thr = 2 * R.EPS * w.sum()
            assert all(x < thr / 100 or x > thr * 100 for x in w), (op, family, k, w / thr)
            kept = C.reference(op, family)[1][k]
            assert kept.sum() == (len(w) - 1 if family == "dropped" else len(w))
            if family != "well":
                assert abs(w[-1] / thr / (1e-3 if family == "dropped" else 1e3) - 1) < 1e-6


def test_zero_singular_values_reach_the_completion():
    for op in C.SVD_OPS:
        for family, least in (("rank1", 1), ("rank2", 1)):
            zeros = [int((C.P.cv_svd(r.reshape(C.SVD_OPS[op]))[0] <= R.DBL_MIN).sum())
                     for r in C.problems(op, family)]
            assert max(zeros) >= least and (family == "rank1" or min(zeros) >= 1), (op, family, zeros)


@pytest.mark.parametrize("family", C.SVD12_FAMILIES)
def test_svd12_cases_take_the_listed_path(family):
    paths = [C.svd12_path(w) for w in C.oracle_w12(family)]
    want = C.SVD12_PATH[family]
    assert paths == ([want] * C.K if isinstance(want, str) else want), paths
    if family in ("zero", "epnp_planar"):
        assert all((w <= R.DBL_MIN).any() for w in C.oracle_w12(family))       # the RNG completion
    if family == "tie":
        assert all(len(set(w.tolist())) < 12 and (w > R.DBL_MIN).all() for w in C.oracle_w12(family))
    if family.startswith("epnp"):
        # five points leave M (10 x 12) a null space: the smallest values cluster at 0
        sig = C.reference("svd12", family)[0]
        assert float((sig[:, 10] / sig[:, 0]).max()) < 1e-12
    if family == "dup":
        assert all((w <= R.DBL_MIN).sum() == 1 for w in C.oracle_w12(family))
    if family == "graded":
        a = np.abs(C.problems("svd12", family))
        assert a.max() / a[a > 0].min() > 1e9
    assert set(C.SVD12_PATH) == set(C.SVD12_FAMILIES)


def test_both_signs_of_beta_within_one_pass():
    """beta = W_i - W_j of the disjoint pairs (0, 1) and (2, 3), the first pass
    of the lane schedules, differ in sign (and swap between problems)."""
    for op in ("svd4x4", "svd6x4", "svd6x5", "svd9x9", "svd_at9x7"):
        M, N = C.SVD_OPS[op]
        signs = set()
        for row in C.problems(op, "beta_signs"):
            W = (row.reshape(M, N) ** 2).sum(0)
            assert (W[0] - W[1]) * (W[2] - W[3]) < 0
            signs.add(W[0] < W[1])
        assert signs == {True, False}


@pytest.mark.parametrize("op,prefix", [("svd6x4", "L4"), ("svd6x5", "L5")])
def test_both_signs_of_beta_meet_in_one_lane_pass(op, prefix):
    """In the lane-parallel sweeps a pass rotates two disjoint pairs at once
    and selects the beta < 0 case per lane: every problem of the family has a
    pass of the tail + head schedule (svd_schedule.h, the first one run) whose
    two rotations are both made and have betas of opposite signs.  (The
    schedule makes the sequential order's rotations on the same values, so
    their betas are those of the sequential model.)"""
    from test_pnp_svd_schedule import _tables
    per = _tables(prefix)["Per"]
    M, N = C.SVD_OPS[op]
    for row in C.problems(op, "beta_signs"):
        trace = []
        R.fp64_jacobi(row.reshape(M, N), trace=trace)
        beta = {(s, i, j): b for s, i, j, b in trace}
        assert any(s == 0 for s, _, _ in beta)                                # sweep 0 turns: the schedule runs
        mixed = [slots for n, slots in per if n == 2 and all((t, i, j) in beta for i, j, t in slots)
                 and beta[(slots[0][2],) + slots[0][:2]] * beta[(slots[1][2],) + slots[1][:2]] < 0]
        assert mixed, (op, sorted(beta))


def _replay12(A):
    """cv_svd12_lanes' control flow on the pass tables of svd_schedule.h (as
    tests/test_pnp_svd_schedule.py scheduled) -> per pass the betas W_i - W_j
    of the rotations it makes."""
    from test_pnp_svd_schedule import _rotate, _tables
    tabs = _tables("")
    At = [list(map(float, A[:, i])) for i in range(12)]
    W = [C.P.tree16([x * x for x in r]) for r in At]
    ch, passes = [False, False], []

    def run(name):
        for n, slots in tabs[name]:
            res = [(i, j, t, W[i] - W[j], _rotate(At, W, i, j)) for i, j, t in slots[:n]]
            passes.append([b for _, _, _, b, r in res if r])
            for i, j, t, _, r in res:
                if r:
                    At[i], At[j], W[i], W[j] = r
                    ch[t] = True

    s, head = 0, True
    while True:
        if head:
            run("Pro")
        head = False
        if ch[1] and s + 1 < 30:
            ch[0] = ch[1] = False
            run("Per")
            s += 1
        else:
            turned = ch[1]
            ch[0] = False
            run("Epi")
            if not (turned or ch[0]) or s + 1 >= 30:
                break
            s += 1
            ch[1] = False
            head = True
    return passes, W


@pytest.mark.parametrize("family", ["beta_signs", "gaussian", "epnp_general"])
def test_svd12_passes_mix_both_signs_of_beta(family):
    """svd_pass selects the beta < 0 case per 16-lane row: every problem has
    passes that make two or more rotations with betas of opposite signs (and
    the replay ends at the oracle's singular values, so it is the kernel's
    order)."""
    for k, row in enumerate(C.problems("svd12", family)):
        passes, W = _replay12(row.reshape(12, 12).T)
        mixed = [p for p in passes if len(p) >= 2 and min(p) < 0 < max(p)]
        assert len(mixed) >= (10 if family == "beta_signs" else 1), (family, k, len(mixed))
        assert sorted(np.sqrt(W), reverse=True) == sorted(C.oracle_w12(family)[k], reverse=True)


def test_deal_gives_neighbours_different_problems():
    d = C.deal(600)
    assert (d[1:] != d[:-1]).all() and set(d.tolist()) == set(range(C.K))
    assert d[255] != d[256] and d[2] != d[3]


# ---- planted faults ------------------------------------------------------------
def _model_metrics(op, family, fault):
    M, N = C.SVD_OPS[op]
    out = [C._pack_svd(*(lambda r: (r[0], r[1].T, r[2]))(R.fp64_jacobi(row.reshape(M, N), fault)))
           for row in C.problems(op, family)]
    return C.metrics(op, family, np.array(out))


@pytest.mark.parametrize("op", ["svd4x4", "svd6x4", "svd6x5", "svd9x9"])
def test_planted_svd_faults_exceed_the_caps(op):
    cap = C.caps(op, "gaussian")
    clean = _model_metrics(op, "gaussian", None)
    assert all(clean[m] <= cap[m] for m in cap), (clean, cap)                  # the model itself passes
    for fault, metric in (("skip_rotation", "orthu"), ("neg_s_row", "recon")):
        e = _model_metrics(op, "gaussian", fault)
        assert e[metric] > 1000 * cap[metric], (op, fault, e, cap)
    # (the sweeps leave Gaussian rows in descending order by themselves: the
    # sort matters where nothing turns and the columns come permuted)
    cap, e = C.caps(op, "orthogonal"), _model_metrics(op, "orthogonal", "nosort_vt")
    assert _model_metrics(op, "orthogonal", None)["recon"] <= cap["recon"]
    assert e["recon"] > 1000 * cap["recon"] and e["vecv"] > 1000 * cap["vecv"], (op, e, cap)


@pytest.mark.parametrize("op", list(C.LSTSQ_OPS))
def test_planted_threshold_fault_exceeds_the_cap(op):
    N = C.LSTSQ_OPS[op]
    cap = C.caps(op, "kept")["x"]
    good = np.array([R.fp64_lstsq(r[:6 * N].reshape(6, N), r[6 * N:]) for r in C.problems(op, "kept")])
    bad = np.array([R.fp64_lstsq(r[:6 * N].reshape(6, N), r[6 * N:], 2e-10) for r in C.problems(op, "kept")])
    assert C.metrics(op, "kept", good)["x"] <= cap
    assert C.metrics(op, "kept", bad)["x"] > 1000 * cap


def test_planted_h_fault_exceeds_the_cap():
    for scene in ("bd_1e-1", "bd_1e-3"):
        s = C.tri_scene(scene)
        cap, _ = C.tri_cap(scene)
        args = (s["P"][s["cam0"]], s["P"][s["cam1"]], s["uv0"], s["uv1"])
        assert C.tri_error(scene, R.fp64_triangulate(*args)) <= cap
        assert C.tri_error(scene, R.fp64_triangulate(*args, h_row=2)) > 1000 * cap
