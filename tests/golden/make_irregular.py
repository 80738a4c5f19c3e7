#!/usr/bin/env python3
"""Generates tests/golden/irregular.json: for every scene of
tests/irregular_cases.py the oracle's trajectory, termination and the scene's
structural counts; for the two rejecting scenes also the cross-check against
the dense numpy restatement of the trust-region loop
(make_lm_branches.np_lm: equal sequences and termination asserted here) and
the per-iteration disagreement of the two that scales the GPU test's
tolerances, under tests/golden/step_prep.json's keys.  The numpy run takes
10-30 s per scene, so it is done here and not in a test.

Run from the repository root:  python tests/golden/make_irregular.py
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from make_lm_branches import np_lm, opts_dict, run_oracle, seq_of  # noqa: E402

TERMINATION = ["CONVERGENCE", "NO_CONVERGENCE", "FAILURE"]


def decisiveness(tr, od):
    """(min |rho - min_relative_decrease| over the non-final iterations,
    |cost_change| / cost of the final iteration, of the one before it)."""
    rho = min(abs(it["relative_decrease"] - od["min_relative_decrease"]) for it in tr[1:-1])
    return rho, abs(tr[-1]["cost_change"]) / tr[-1]["cost"], abs(tr[-2]["cost_change"]) / tr[-2]["cost"]


def main():
    import lm_cases as L
    import irregular_cases as IC
    from oracle import ffi as O

    out = {}
    for name in IC.SCENES:
        s = IC.build(name)
        od = opts_dict(O)
        sm, tr, (r, t, X) = run_oracle(O, s, 2, od)
        term = TERMINATION[sm["termination_type"]]
        rho, last, before = decisiveness(tr, od)
        # (without the oracle's wall-clock fields, so that a rerun reproduces the file)
        summary = {k: v for k, v in sm.items() if not k.endswith("_time_s")}
        out[name] = dict(mode=2, options=od, summary=summary, trace=tr, sequence=seq_of(tr), termination=term,
                         counts=IC.structure(s, IC.SCENES[name][3]))
        line = (f"{name:12s} {term:12s} {seq_of(tr):16s} rho margin {rho:.3f} last change {last:.2e} "
                f"before it {before:.2e}")
        if name in IC.REJECTING:
            ntr, nterm, nx = np_lm(s.uv, s.cam_idx, s.pt_idx, s.K, s.rot.copy(), s.t.copy(), s.X.copy(), 2, od)
            assert seq_of(tr) == seq_of(ntr), (name, seq_of(tr), seq_of(ntr))
            assert term == nterm, (name, term, nterm)
            C_, P_ = s.rot.shape[0], s.X.shape[0]
            nxc = nx[:6 * C_].reshape(C_, 6)
            res_fn = lambda *a: O.residuals_jacobians(*a, jacobian=False)[0]
            gi_res, gi_al = L.gauge_invariant_diff(res_fn, s, (r, t, X),
                                                   (nxc[:, :3], nxc[:, 3:], nx[6 * C_:].reshape(P_, 3)))
            xf = np.concatenate([np.hstack([r, t]).ravel(), X.ravel()])
            out[name].update(
                numpy_termination=nterm,
                numpy_cost_rel_diff=[abs(a["cost"] - b["cost"]) / b["cost"] for a, b in zip(tr, ntr)],
                numpy_radius_rel_diff=[abs(a["trust_region_radius"] - b["trust_region_radius"]) /
                                       b["trust_region_radius"] for a, b in zip(tr, ntr)],
                numpy_param_max_rel=float(np.max(np.abs(xf - nx) / np.maximum(np.abs(nx), 1e-3))),
                numpy_residual_max_abs=gi_res, numpy_aligned_max_rel=gi_al)
            line += (f" | numpy: cost {max(out[name]['numpy_cost_rel_diff']):.1e} "
                     f"radius {max(out[name]['numpy_radius_rel_diff']):.1e} "
                     f"params {out[name]['numpy_param_max_rel']:.1e} res {gi_res:.1e} aligned {gi_al:.1e}")
        print(line)
    with open(os.path.join(HERE, "irregular.json"), "w") as f:
        json.dump(out, f, indent=0)


if __name__ == "__main__":
    main()
