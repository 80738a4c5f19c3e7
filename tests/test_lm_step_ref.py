"""CPU checks of the single-step reference (tests/lm_step_ref.py) and of the
scenes of tests/lm_step_cases.py, which tests/test_gpu_lm_step.py relies on:

* the Schur route agrees with a dense longdouble solve of the full damped
  normal equations, in every mode, and the reduced system's two solvers
  (ref_solve, fp64 LAPACK + compensated refinement) agree at the largest size
  where both run: to ref_self_error(), a factor 1000 below the smallest cap;
* the scale taken at x instead of x0 moves the step by far less than the fp64
  yardsticks' error, and a scaled diagonal entry near a clamp is refused;
* every scene lies on its side of the solve plan's boundaries, and the steps
  chosen on the rejecting scenes are of the kinds they are chosen for;
* the third yardstick: the matrix-form residual is as accurate as the
  functor's, and the twin that takes its point-side sums from it shows the
  lost gauge cancellation lm_step_ref's text describes;
* the caps discriminate: each planted fault in the fp64 twin exceeds the cap
  the GPU test would apply (all three yardsticks) by at least 100x, at step 1
  and at step 2.
"""
import functools

import numpy as np
import pytest

import irregular_cases as IC
import lm_step_cases as LC
import lm_step_ref as S
from oracle import ffi as O
from sfm_amd import scene

LD = np.longdouble
ZERO_TOL, oracle_step = LC.ZERO_TOL, LC.oracle_step


@functools.lru_cache(maxsize=None)
def _step(name, mode, k=1):
    """Reference, twin, split-residual model and oracle of step k from where
    the oracle's first k - 1 iterations lead (shared, left unchanged), and the
    worst yardstick's statistics
    -> (scene, pb, x, radius, ref, twin, x_oracle, (yard_c, yard_p), model)."""
    s = LC.build(name)
    pb = S.problem(s.uv, s.cam_idx, s.pt_idx, s.K, mode)
    x0 = s.copy_params()
    r, t, X = s.copy_params()
    _, tr = O.solve(s.uv, s.cam_idx, s.pt_idx, s.K, r, t, X, mode=mode,
                    options=O.default_options(max_num_iterations=k - 1, **ZERO_TOL))
    x, radius = (r, t, X), tr[-1]["trust_region_radius"]
    ref = S.lm_step(pb, x0, x, radius, LD)
    tw = S.lm_step(pb, x0, x, radius, np.float64)
    md = S.lm_step(pb, x0, x, radius, np.float64, split_residual=True)
    _, xo = oracle_step(s, mode, x, radius)
    e = [S.step_error(*S.delta_of(xo, x), ref), S.step_error(tw.delta_c, tw.delta_p, ref),
         S.step_error(md.delta_c, md.delta_p, ref)]
    return s, pb, x, radius, ref, tw, xo, tuple(max(a) for a in zip(*e)), md


def _small():
    return scene.generate(6, 40, views=4, seed=LC.L.SEED + 1)


@pytest.mark.parametrize("radius", [2.0, 1e4, 2e5])
@pytest.mark.parametrize("mode", [S.STRUCT_AND_POSE, S.POSE_ONLY, S.STRUCT_ONLY])
def test_schur_route_matches_the_dense_longdouble_solve(mode, radius):
    s = _small()
    pb = S.problem(s.uv, s.cam_idx, s.pt_idx, s.K, mode)
    x = s.copy_params()
    ref = S.lm_step(pb, x, x, radius, LD)
    dense = S.lm_step(pb, x, x, radius, LD, dense_full=True)
    e = S.step_error(ref.delta_c, ref.delta_p, dense)
    bound = S.ref_self_error(mode, radius)
    print(f"mode {mode} radius {radius:g}: Schur against dense, cameras {e[0]:.2e} points {e[1]:.2e} (bound {bound:.0e})")
    assert max(e) <= bound
    for f in ("step_norm", "model_cost_change", "new_cost", "relative_decrease", "radius"):
        a, b = getattr(ref, f), getattr(dense, f)
        assert abs(a - b) <= bound * (ref.cost_change_cond + ref.model_cond) * abs(b), f
    assert ref.step_is_valid and dense.step_is_valid and ref.step_is_successful == dense.step_is_successful


def test_the_two_reduced_solvers_agree_at_the_switch():
    C = S.DENSE_LD_MAX // 6
    s = scene.generate(C, 400, views=4, seed=LC.L.SEED + 2)
    pb = S.problem(s.uv, s.cam_idx, s.pt_idx, s.K)
    x = s.copy_params()
    a = S.lm_step(pb, x, x, 1e4, LD, force_solver="ref")
    b = S.lm_step(pb, x, x, 1e4, LD, force_solver="refined")
    e = S.step_error(b.delta_c, b.delta_p, a)
    print(f"{6 * C} rows: refined against ref_solve, cameras {e[0]:.2e} points {e[1]:.2e}")
    assert 6 * C <= S.DENSE_LD_MAX < 6 * (C + 1)
    assert max(e) <= S.ref_self_error(S.STRUCT_AND_POSE, 1e4)


def test_refinement_converges_from_the_fp64_factor():
    rng = np.random.default_rng(3)
    n = 200
    Q, _ = np.linalg.qr(rng.normal(size=(n, n)))
    A = (Q * np.logspace(0, -6, n)) @ Q.T
    A = (A + A.T) / 2
    b = rng.normal(size=n)
    y, steps = S.refined_solve(A, b)
    yr, _ = S.R.ref_solve(A, b)
    assert steps <= 8
    assert float(np.max(np.abs(y - yr)) / np.max(np.abs(yr))) <= 2.0 ** -58


def test_the_step_does_not_depend_on_where_the_scale_is_taken():
    s, pb, _, _, ref, tw, xo, yard, _ = _step("c22", S.STRUCT_AND_POSE)
    x0 = s.copy_params()
    at_x0 = S.lm_step(pb, x0, xo, 3e4, LD)
    at_x = S.lm_step(pb, xo, xo, 3e4, LD)
    assert not np.array_equal(np.asarray(at_x0.scale_c, np.float64), np.asarray(at_x.scale_c, np.float64))
    e = S.step_error(at_x.delta_c, at_x.delta_p, at_x0)
    # the yardsticks of this very step: the twin, and the oracle restarted at x (its scale is taken there)
    tw2 = S.lm_step(pb, x0, xo, 3e4, np.float64)
    _, x2 = oracle_step(s, S.STRUCT_AND_POSE, xo, 3e4)
    y = S.step_error(tw2.delta_c, tw2.delta_p, at_x0) + S.step_error(*S.delta_of(x2, xo), at_x0)
    print(f"scale at x against scale at x0: {e[0]:.2e} {e[1]:.2e}; twin {y[0]:.2e} {y[1]:.2e} oracle {y[2]:.2e} {y[3]:.2e}")
    assert max(e) <= 1e-3 * min(y)


def test_a_diagonal_entry_near_a_clamp_is_refused():
    s = LC.build("c22")
    x = s.copy_params()
    probe = S.lm_step(S.problem(s.uv, s.cam_idx, s.pt_idx, s.K), x, x, 1e4, np.float64)
    assert probe.step_is_valid
    # the scaled diagonal is below 1 (scale = 1 / (1 + norm)): a lower clamp of 0.6 is within a factor 2 of it
    with pytest.raises(AssertionError, match="clamp"):
        S.lm_step(S.problem(s.uv, s.cam_idx, s.pt_idx, s.K, min_lm_diagonal=0.6), x, x, 1e4, np.float64)
    with pytest.raises(AssertionError, match="clamp"):
        S.lm_step(S.problem(s.uv, s.cam_idx, s.pt_idx, s.K, max_lm_diagonal=1.5), x, x, 1e4, np.float64)


@pytest.mark.parametrize("case", list(LC.CASES))
def test_every_scene_is_on_its_side_of_the_plan(case):
    name, mode, env, expect = LC.CASES[case]
    s = LC.build(name)
    p = LC.plan(s, mode, env)
    assert expect, case
    for k, v in expect.items():
        assert p[k] == v, (case, k, p[k], v)
    # inside set_problem's bounds, every camera block of an active camera observed
    assert s.n_obs <= IC.K_HOST_CHECK_MAX_OBS and s.cam_idx.max() < s.n_cams and s.pt_idx.max() < s.n_pts


def test_the_boundaries_are_the_plans():
    side = lambda a, b, key: (LC.plan(LC.build(a), 2, {})[key], LC.plan(LC.build(b), 2, {})[key])
    assert side("c21", "c22", "chol_small") == (True, False)
    assert side("c64", "c65", "point_pass") == ("Lds64", "Lds512x2")
    assert side("c64", "c65", "cam_sums") == ("InPointPass", "SumDiag")
    assert side("c127", "c128", "pair_pass") == ("Pts", "RotPersistent")
    assert side("c127", "c128", "backsub") == ("ThreePass", "OnePass")
    assert side("c256", "c257", "lm") == ("DeviceFusedAcceptFold", "DeviceFused")
    assert side("c512", "c513", "backsub") == ("OnePass", "ThreePass")
    assert side("c512", "c513", "point_pass") == ("Lds512x2", "Rc")
    w = LC.plan(LC.build("wg6"), 2, {})
    assert w["n_blk"] <= 1024 and w["n_pairs"] >= 256 * w["n_blk"] and w["pair_pass"] == "WgBlocks"
    for name in ("irr_100", "irr_130"):
        st = IC.structure(LC.build(name), IC.HUBS)
        assert st["min_degree"] == 0 and st["single_view_points"] > 0 and st["max_degree"] >= st["n_cams"] - 4
        assert st["empty_cameras"] == 2 and st["duplicate_keys"] >= 30
        assert np.bincount(LC.build(name).cam_idx, minlength=st["n_cams"])[-1] == 0   # the last block row of S
        assert not np.all(np.diff(LC.build(name).pt_idx) >= 0)


@pytest.mark.parametrize("name", LC.REJECTING)
def test_the_steps_of_a_rejecting_scene_are_what_they_are_chosen_for(name):
    s = LC.build(name)
    steps = LC.steps_of(name)
    r, t, X = s.copy_params()
    _, tr = O.solve(s.uv, s.cam_idx, s.pt_idx, s.K, r, t, X, options=O.default_options(max_num_iterations=max(steps), **ZERO_TOL))
    seq = IC.seq_of(tr)
    assert seq == LC.recorded_sequence(name)[:len(seq)], (seq, LC.recorded_sequence(name))
    kinds = {k: (seq[k - 2] if k > 1 else "-") + seq[k - 1] for k in steps}
    print(name, seq, kinds)
    assert any(v[1] == "R" for v in kinds.values())                  # a rejected step itself
    assert any(v[0] == "R" for v in kinds.values())                  # the step right after a rejected one
    assert any(v == "RA" for v in kinds.values())                    # ... and an accepted one among them
    assert {1, 2} <= set(steps)


FAULT_SCENES = ("rej_100_irr", "rej_130_irr")


def _faults(s):
    """One fault of each kind, away from the hubs and the empty cameras."""
    deg = np.bincount(s.pt_idx, minlength=s.n_pts)
    p = next(q for q in range(len(IC.HUBS), s.n_pts) if deg[q] >= 3)
    obs = np.flatnonzero(s.pt_idx == p)
    i = int(obs[0])
    j = int(next(o for o in obs if s.cam_idx[o] != s.cam_idx[i]))
    return {"pair": ("pair", i, j), "backsub_obs": ("backsub_obs", i), "stale_point": ("stale_point", p, 2e4),
            "no_damping": ("no_damping", int(s.cam_idx[j]))}


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("kind", ["pair", "backsub_obs", "stale_point", "no_damping"])
@pytest.mark.parametrize("name", FAULT_SCENES)
def test_a_planted_fault_exceeds_the_cap_a_hundredfold(name, kind, k):
    # step 1, and step 2, where the split-residual model makes the cap widest
    s, pb, x, radius, ref, tw, xo, yard, md = _step(name, S.STRUCT_AND_POSE, k)
    x0 = s.copy_params()
    # the unharmed yardsticks, measured as the device is, stay inside
    clean = max(S.delta_ratio(tw.x_new, x, ref, *yard) + S.delta_ratio(xo, x, ref, *yard) + S.delta_ratio(md.x_new, x, ref, *yard))
    assert clean <= 1.0 / 8 + 1e-12, clean
    fault = _faults(s)[kind]
    if kind == "stale_point":
        fault = fault[:2] + (2 * radius,)
    bad = S.lm_step(pb, x0, x, radius, np.float64, fault=fault)
    ratio = max(S.delta_ratio(bad.x_new, x, ref, *yard))
    print(f"{name} step {k} {kind}: error / cap {ratio:.3g} (worst yardstick {yard[0]:.2e} {yard[1]:.2e})")
    assert ratio >= 100.0


def test_the_matrix_form_residual_is_as_good_as_the_functors():
    s, pb, x, _, ref, _, _, _, _ = _step("c65", S.STRUCT_AND_POSE, 2)
    exact, _ = S.residuals_jacobians(pb, x, LD)
    functor, _ = S.residuals_jacobians(pb, x, np.float64)
    matrix = S.residuals_matrix_form(pb, x, np.float64)
    size = np.abs(np.asarray(exact, np.float64) + s.uv) + np.abs(s.uv)
    e_f = np.max(np.abs(np.asarray(functor - exact, np.float64)) / size)
    e_m = np.max(np.abs(np.asarray(matrix - exact, np.float64)) / size)
    print(f"residual error / (|projection| + |uv|): functor {e_f / S.U64:.2f} u, matrix form {e_m / S.U64:.2f} u")
    # (rotation, translation, division, intrinsics: the projection is some eight roundings deep)
    assert e_f <= 8 * S.U64 and e_m <= 8 * S.U64 and e_m <= 2 * e_f
    assert not np.array_equal(functor, matrix)
    # ... and in longdouble the two formulations are one function
    assert np.max(np.abs(np.asarray(S.residuals_matrix_form(pb, x, LD) - exact, np.float64)) / size) <= 2.0 ** -62
    # the small-angle branch (camera 0 of a generated scene has rot = 0)
    s0 = LC.build("c22")
    assert not s0.rot[0].any()
    p0 = S.problem(s0.uv, s0.cam_idx, s0.pt_idx, s0.K)
    a, _ = S.residuals_jacobians(p0, s0.copy_params(), LD)
    b = S.residuals_matrix_form(p0, s0.copy_params(), LD)
    assert np.all(np.isfinite(np.asarray(b, np.float64))) and float(np.max(np.abs(a - b))) <= 1e-15


@pytest.mark.parametrize("name", ["c22", "c65", "c128"])
def test_the_split_residual_model_shows_the_lost_cancellation(name):
    """Two residuals per observation, each right to a few u (|projection| +
    |uv|): near the optimum (step 2) the step's error is far above the twin's
    and lies in the gauge directions, i.e. the cost does not see it."""
    s, pb, x, radius, ref, tw, xo, yard, md = _step(name, S.STRUCT_AND_POSE, 2)
    e_t = S.step_error(tw.delta_c, tw.delta_p, ref)
    e_m = S.step_error(md.delta_c, md.delta_p, ref)
    print(f"{name} step 2: twin {e_t[0]:.2e} {e_t[1]:.2e}, split residuals {e_m[0]:.2e} {e_m[1]:.2e}; "
          f"cost change {float(ref.cost_change):.6g}, model's off by {float(abs(md.cost_change - ref.cost_change) / ref.cost_change):.2e}")
    assert min(e_m) >= 30 * max(e_t)
    # what the trace reports moves no more than the twin's does, up to the 8 of the caps
    refs, tws, mds = S.scalar_refs(ref), S.scalar_refs(tw), S.scalar_refs(md)
    for q in ("cost", "cost_change", "relative_decrease"):
        assert S.scalar_ratio(mds[q][0], refs[q][0], refs[q][1], [tws[q][0]]) <= 8.0, q


def test_the_reference_is_a_thousandfold_below_the_smallest_cap():
    """Mode by mode (the reference's own error follows the system's
    condition), over every scene up to 130 cameras; the GPU test repeats the
    comparison for each of its cases, the larger ones included."""
    small = sorted({(n, m) for n, m, _, _ in LC.CASES.values() if LC.build(n).n_cams <= 130})
    caps = {}
    for name, mode in small:
        yard = _step(name, mode)[7]
        live = [y for y, on in zip(yard, (mode != S.STRUCT_ONLY, mode != S.POSE_ONLY)) if on]
        caps.setdefault(mode, {})[name] = 8 * min(live)
    assert set(caps) == {0, 1, 2}
    for mode, c in caps.items():
        k = min(c, key=c.get)
        print(f"mode {mode}: smallest cap {c[k]:.2e} at {k}; the reference's own error is below {S.ref_self_error(mode, 1e4):.0e}")
        assert 1000 * S.ref_self_error(mode, 1e4) <= c[k]
