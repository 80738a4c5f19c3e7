"""Helpers shared by tests/test_gpu_step_prep.py and tests/test_gpu_irregular.py
for scenes whose LM trajectory rejects steps: the device loop against the
host loop (bitwise), and either against the oracle within the branch tests'
tolerances (tests/test_gpu_lm_branches.py), scaled by the oracle's recorded
disagreement with the dense numpy restatement of the loop.

`c` is a scene's fixture entry (mode, options, trace, numpy_* figures);
`oracle` is (scene, summary, trace, (rot, t, X)) of the live oracle solve.
"""
import numpy as np

import lm_cases as L
import sfm_amd
from oracle import ffi as O


def seq_of(trace):
    return "".join("I" if not it["step_is_valid"] else ("A" if it["step_is_successful"] else "R") for it in trace[1:])


def rel(a, b, floor=1e-3):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), floor)))


def residuals(uv, cam_idx, pt_idx, K, rot, t, X):
    return O.residuals_jacobians(uv, cam_idx, pt_idx, K, rot, t, X, jacobian=False)[0]


def solve_oracle(c, s):
    r, t, X = s.copy_params()
    sm, tr = O.solve(s.uv, s.cam_idx, s.pt_idx, s.K, r, t, X, mode=c["mode"], options=O.default_options(**c["options"]))
    return s, sm, tr, (r, t, X)


def solve_device_and_host(c, s, monkeypatch):
    out = {}
    for host in (False, True):
        if host:
            monkeypatch.setenv("SFM_HOST_LM", "1")
        else:
            monkeypatch.delenv("SFM_HOST_LM", raising=False)
        r, t, X = s.copy_params()
        sm, tr = sfm_amd.solve(s.uv, s.cam_idx, s.pt_idx, s.K, r, t, X, mode=c["mode"],
                               options=sfm_amd.make_options(**c["options"]))
        out[host] = (sm, tr, (r, t, X))
    return out[False], out[True]


def assert_loops_equal(dev, host):
    (sa, ta, pa), (sb, tb, pb) = dev, host
    assert ta == tb, (seq_of(ta), seq_of(tb))
    for f in ("termination_type", "num_iterations", "num_successful_steps", "num_unsuccessful_steps",
              "num_invalid_steps", "num_residual_evaluations", "num_jacobian_evaluations", "num_linear_solves"):
        assert getattr(sa, f) == getattr(sb, f), f
    assert sa.final_cost == sb.final_cost
    for a, b in zip(pa, pb):
        assert a.tobytes() == b.tobytes()


def assert_branch_parity(name, c, oracle, got):
    """test_gpu_lm_branches.test_branch_trajectory_matches_oracle's assertions."""
    s, sm_o, tr_o, sol_o = oracle
    sm_g, tr_g, sol_g = got
    assert seq_of(tr_o) == seq_of(c["trace"])  # the live oracle is the fixture's
    assert seq_of(tr_g) == seq_of(tr_o), (seq_of(tr_g), seq_of(tr_o))
    assert sm_g.termination_type == sm_o["termination_type"]
    assert sm_g.num_iterations == sm_o["num_iterations"]
    assert sm_g.num_successful_steps == sm_o["num_successful_steps"]
    assert sm_g.num_unsuccessful_steps == sm_o["num_unsuccessful_steps"]
    assert sm_g.num_invalid_steps == sm_o["num_invalid_steps"]
    d_np, r_np = c["numpy_cost_rel_diff"], c["numpy_radius_rel_diff"]
    worst_c = worst_r = 0.0
    for i, (a, b) in enumerate(zip(tr_g, tr_o)):
        worst_c = max(worst_c, abs(a["cost"] - b["cost"]) / b["cost"])
        worst_r = max(worst_r, abs(a["trust_region_radius"] - b["trust_region_radius"]) / b["trust_region_radius"])
    par = max(rel(a, b) for a, b in zip(sol_g, sol_o))
    res, al = L.gauge_invariant_diff(residuals, s, sol_g, sol_o)
    print(f"{name}: {seq_of(tr_g)} cost {worst_c:.2e} radius {worst_r:.2e} params {par:.2e} residuals {res:.2e} px "
          f"aligned {al:.2e}")
    for i, (a, b) in enumerate(zip(tr_g, tr_o)):
        tol = max(1e-9, 20 * d_np[i])
        assert abs(a["cost"] - b["cost"]) <= tol * b["cost"], (i, a["cost"], b["cost"], tol)
        tol = max(1e-6, 20 * r_np[i])
        assert abs(a["trust_region_radius"] - b["trust_region_radius"]) <= tol * b["trust_region_radius"], \
            (i, a["trust_region_radius"], b["trust_region_radius"])
    assert abs(sm_g.final_cost - sm_o["final_cost"]) <= max(1e-9, 20 * d_np[-1]) * sm_o["final_cost"]
    assert par < max(1e-6, 20 * c["numpy_param_max_rel"])
    assert res <= max(1e-6, 20 * c["numpy_residual_max_abs"]), res
    assert al <= max(1e-6, 20 * c["numpy_aligned_max_rel"]), al
