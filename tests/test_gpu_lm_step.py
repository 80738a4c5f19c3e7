"""Single Levenberg-Marquardt steps of the device bundle adjuster against the
extended-precision reference of tests/lm_step_ref.py, at the precision fp64
arithmetic delivers, on one scene per side of every boundary of the solve
plan (tests/lm_step_cases.py; tests/test_lm_step_ref.py checks reference,
scenes and caps on the CPU).

Step k of a case, every stopping tolerance 0: the device solves with
max_num_iterations = k and again with k - 1; the shorter trace must be
bitwise the prefix of the longer, and the device's step is x_k - x_(k-1)
formed in longdouble.  The reference starts from the device's own x_(k-1) and
trace[k-1].trust_region_radius, with the Jacobi scale of x0.  Two correct
fp64 solutions of the same step are the yardsticks: the oracle restarted at
x_(k-1) with that radius for one iteration, and the reference's fp64 twin.
A third one is the twin with the one property of the device's formulation
that correct fp64 code of another shape does not share: the camera side's
and the point side's sums take their residuals from separate evaluations
(lm_step_ref's text: the gauge directions lose an exact cancellation, and
near the optimum the step's error is 100 to 1000 times the twin's).

Caps (none comes from a GPU run):
* the step, per parameter block (a camera's 6, a point's 3) in scaled units
  delta / scale: the 2-norm of the error over max(the block's reference norm,
  the RMS block norm of its kind) may be 8 x the worst yardstick's maximum of
  the same statistic, plus the read-back floor u |x_k| / scale of the block.
  8 is the margin tests/test_gpu_chol.py gives another accumulation order;
* trace[k]'s cost, cost_change, step_norm, relative_decrease,
  trust_region_radius and gradient_max_norm, and trace[k-1]'s cost and
  gradient_max_norm (trace[0]'s at k = 1): 8 x the worst yardstick's error plus
  4 u x a condition number the reference computes (the cancellation of the
  two costs, of the model's sum and of the gradient's sum; 1 elsewhere);
* step_is_valid and step_is_successful equal the reference's; after a
  rejected step x_k is bitwise x_(k-1) and only the scalars are compared.

Every run prints device error / cap per quantity; SFM_LM_STEP_RECORD=1
rewrites profiles/lm_step_reference_errors.txt from a full run of this file.
"""
import contextlib
import functools
import os

import numpy as np
import pytest

import lm_step_cases as LC
import lm_step_ref as S
import sfm_amd

pytestmark = pytest.mark.gpu

LD = np.longdouble
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_rows = {}


@pytest.fixture(scope="module", autouse=True)
def _record():
    yield
    if os.environ.get("SFM_LM_STEP_RECORD") != "1" or len(_rows) != len(LC.case_steps()):
        return
    with open(os.path.join(ROOT, "profiles", "lm_step_reference_errors.txt"), "w") as f:
        f.write("# tests/test_gpu_lm_step.py: device error / cap per case, step and quantity (a cap is 8 x the worst of\n"
                "# the three fp64 yardsticks plus the floor; 1 is the limit); A accepted, R rejected step\n")
        worst = max((v, q, k) for k, (_, row) in _rows.items() for q, v in row.items())
        f.write(f"# worst: {worst[0]:.3g} ({worst[1]} of {worst[2][0]} step {worst[2][1]})\n")
        for (case, k), (kind, row) in _rows.items():
            f.write(f"{case:16s} {k:2d} {kind} " + " ".join(f"{q} {v:.3g}" for q, v in row.items()) + "\n")


@contextlib.contextmanager
def _environment(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@functools.lru_cache(maxsize=None)
def _device(case, iterations):
    """The device solve of a case stopped after `iterations` -> (trace, x)."""
    name, mode, env, _ = LC.CASES[case]
    s = LC.build(name)
    r, t, X = s.copy_params()
    with _environment(env):
        _, tr = sfm_amd.solve(s.uv, s.cam_idx, s.pt_idx, s.K, r, t, X, mode=mode,
                              options=sfm_amd.make_options(max_num_iterations=iterations, **LC.ZERO_TOL))
    return tr, (r, t, X)


def _bits(trace):
    return [{k: (float(v).hex() if isinstance(v, float) else v) for k, v in it.items()} for it in trace]


def _same(a, b):
    return all(p.tobytes() == q.tobytes() for p, q in zip(a, b))


@pytest.mark.parametrize("case,k", LC.case_steps())
def test_step_matches_the_reference(case, k):
    name, mode, env, _ = LC.CASES[case]
    s = LC.build(name)
    x0 = s.copy_params()
    tr, x_k = _device(case, k)
    tr_prev, x_prev = _device(case, k - 1)
    assert len(tr) == k + 1 and len(tr_prev) == k
    assert _bits(tr_prev) == _bits(tr[:k]), "the shorter solve's trace is not the prefix of the longer"
    if k == 1:
        assert _same(x_prev, x0)
    it, before = tr[k], tr[k - 1]
    radius = before["trust_region_radius"]
    rejected_before = 0
    while rejected_before < k - 1 and not tr[k - 1 - rejected_before]["step_is_successful"]:
        rejected_before += 1

    pb = S.problem(s.uv, s.cam_idx, s.pt_idx, s.K, mode)
    ref = S.lm_step(pb, x0, x_prev, radius, LD, decrease_factor=2.0 ** (1 + rejected_before))
    twin = S.lm_step(pb, x0, x_prev, radius, np.float64, decrease_factor=2.0 ** (1 + rejected_before))
    model = S.lm_step(pb, x0, x_prev, radius, np.float64, decrease_factor=2.0 ** (1 + rejected_before), split_residual=True)
    tr_o, x_o = LC.oracle_step(s, mode, x_prev, radius, threads=8 if s.n_cams > 200 else 1)
    kind = "A" if ref.step_is_successful else "R" if ref.step_is_valid else "I"
    # the yardsticks solve the step the reference solves
    assert (twin.step_is_valid, twin.step_is_successful) == (ref.step_is_valid, ref.step_is_successful)
    assert (model.step_is_valid, model.step_is_successful) == (ref.step_is_valid, ref.step_is_successful)
    assert (bool(tr_o[1]["step_is_valid"]), bool(tr_o[1]["step_is_successful"])) == (ref.step_is_valid, ref.step_is_successful)
    assert ref.step_is_valid, "the cases hold no invalid step"
    assert (bool(it["step_is_valid"]), bool(it["step_is_successful"])) == (ref.step_is_valid, ref.step_is_successful)

    row = {}
    if ref.step_is_successful:
        y_o = S.step_error(*S.delta_of(x_o, x_prev), ref)
        y_t = S.step_error(twin.delta_c, twin.delta_p, ref)
        y_m = S.step_error(model.delta_c, model.delta_p, ref)
        yard = tuple(max(a) for a in zip(y_o, y_t, y_m))
        for on, y in zip((mode != S.STRUCT_ONLY, mode != S.POSE_ONLY), yard):
            # the reference's own error is irrelevant to this cap
            assert not on or 1000 * S.ref_self_error(mode, radius) <= 8 * max(y, S.YARD_FLOOR), (y, radius)
        row["cameras"], row["points"] = S.delta_ratio(x_k, x_prev, ref, *yard)
        # blocks outside the system do not move
        d_c, d_p = S.delta_of(x_k, x_prev)
        assert not d_c[~ref.act_c].any() and not d_p[~ref.act_p].any()
    else:
        assert _same(x_k, x_prev), "a rejected step moved the parameters"

    refs, twins, models = S.scalar_refs(ref), S.scalar_refs(twin), S.scalar_refs(model)
    for q in S.SCALARS:
        yards = [twins[q][0], models[q][0]]
        if q != "trust_region_radius" or ref.step_is_successful:   # (the restarted oracle's decrease factor is 2)
            yards.append(tr_o[1][q])
        row[q] = S.scalar_ratio(it[q], refs[q][0], refs[q][1], yards)
    row["cost_before"] = S.scalar_ratio(before["cost"], ref.cost, 1.0, [twin.cost, model.cost, tr_o[0]["cost"]])
    row["gradient_before"] = S.scalar_ratio(before["gradient_max_norm"], ref.gradient_max_norm, ref.gradient_cond,
                                            [twin.gradient_max_norm, model.gradient_max_norm, tr_o[0]["gradient_max_norm"]])
    _rows[(case, k)] = (kind, row)
    print(f"{case} step {k} {kind} radius {radius:.4g}: error / cap " + " ".join(f"{q} {v:.3g}" for q, v in row.items()))
    for q, v in row.items():
        assert v <= 1.0, (case, k, q, v)
