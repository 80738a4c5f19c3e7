#!/usr/bin/env python3
"""Writes tests/golden/lm_replay.txt from tests/golden/lm_branches.json: the
oracle's options, summary counters and trace records of every branch case as
plain numbers (doubles as hex floats), for the CPU sanitizer program
(tests/asan/asan_main.cpp), which replays them through sfm_amd/csrc/ba_lm.h.

The first line is the number of cases; then one line per case, blank-separated:
    case <name> <records>
    <max_num_iterations> <max_num_consecutive_invalid_steps> <function_tolerance> <gradient_tolerance>
        <parameter_tolerance> <initial_trust_region_radius> <max_trust_region_radius>
        <min_trust_region_radius> <min_relative_decrease>
    <termination_type> <num_iterations> <num_successful_steps> <num_unsuccessful_steps> <num_invalid_steps>
        <num_residual_evaluations> <num_jacobian_evaluations> <num_linear_solves>
    per record: <iteration> <step_is_valid> <step_is_successful> <cost> <cost_change>
        <gradient_max_norm> <step_norm> <relative_decrease> <trust_region_radius>

Run from the repository root:  python tests/golden/make_lm_replay.py
"""
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
OPTS = ("function_tolerance", "gradient_tolerance", "parameter_tolerance", "initial_trust_region_radius",
        "max_trust_region_radius", "min_trust_region_radius", "min_relative_decrease")
COUNTS = ("termination_type", "num_iterations", "num_successful_steps", "num_unsuccessful_steps", "num_invalid_steps",
          "num_residual_evaluations", "num_jacobian_evaluations", "num_linear_solves")
REC = ("cost", "cost_change", "gradient_max_norm", "step_norm", "relative_decrease", "trust_region_radius")


def main():
    fix = json.load(open(os.path.join(HERE, "lm_branches.json")))
    lines = [str(len(fix))]
    for name, c in fix.items():
        o, sm, tr = c["options"], c["summary"], c["trace"]
        w = [f"case {name} {len(tr)}", str(o["max_num_iterations"]), str(o["max_num_consecutive_invalid_steps"])]
        w += [float(o[k]).hex() for k in OPTS] + [str(sm[k]) for k in COUNTS]
        for it in tr:
            w += [str(it["iteration"]), str(it["step_is_valid"]), str(it["step_is_successful"])]
            w += [float(it[k]).hex() for k in REC]
        lines.append(" ".join(w))
    with open(os.path.join(HERE, "lm_replay.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
