"""What a solve leaves behind, recorded bit for bit, on the scenes whose
trajectories take every branch of the LM loop: every case of
tests/golden/lm_branches.json and the two rejecting irregular scenes (more
than 64 cameras: the step preparation folds into the evaluation, so a rejected
step pauses and re-arms the loop), under the three ways the loop is driven
(default: device loop with the bookkeeping fused into the reductions;
SFM_LM_UNFUSED=1: the k_lm_* launches; SFM_HOST_LM=1: the host driver), and one
two-rank solve through the host all-reduce hook (the host driver with
collectives).

Shared by tests/golden/make_lm_loop_parent.py, which records
tests/golden/lm_loop_parent.json on the commit before a change to the loop,
and tests/test_gpu_lm_loop_parent.py, which asserts equality after it.
"""
from __future__ import annotations

import functools
import hashlib
import json
import os

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

ENVS = {"default": {}, "host": {"SFM_HOST_LM": "1"}, "unfused": {"SFM_LM_UNFUSED": "1"}}
LOOP_VARS = ("SFM_HOST_LM", "SFM_LM_UNFUSED", "SFM_LM_BATCH", "SFM_NO_ACCEPT_FOLD")
IRREGULAR = ("rej_100_irr", "rej_130_irr")
TWO_RANKS = "two_ranks_host_comm"
SUMMARY_FIELDS = ("termination_type", "num_iterations", "num_successful_steps", "num_unsuccessful_steps",
                  "num_invalid_steps", "num_residual_evaluations", "num_jacobian_evaluations", "num_linear_solves",
                  "initial_cost", "final_cost")
TRACE_FIELDS = ("iteration", "step_is_valid", "step_is_successful", "cost", "cost_change", "gradient_max_norm",
                "step_norm", "relative_decrease", "trust_region_radius")


@functools.lru_cache(maxsize=None)
def _fixtures():
    return (json.load(open(os.path.join(G, "lm_branches.json"))), json.load(open(os.path.join(G, "irregular.json"))))


def scene_names():
    return list(_fixtures()[0]) + list(IRREGULAR)


@functools.lru_cache(maxsize=4)
def build(name):
    """-> (scene, mode, options dict)"""
    branches, irregular = _fixtures()
    if name in IRREGULAR:
        import irregular_cases as IC
        return IC.build(name), irregular[name]["mode"], irregular[name]["options"]
    import lm_cases as L
    make, _, mode = L.cases()[name]
    return make(), mode, branches[name]["options"]


def _hex(v):
    return float(v).hex() if isinstance(v, float) else int(v)


def as_record(sm, trace, rot, t, X):
    """Trace records (each a list in TRACE_FIELDS order) and summary with
    every double as a hex float, and a SHA-256 of the parameter bytes."""
    h = hashlib.sha256()
    for a in (rot, t, X):
        h.update(a.tobytes())
    return dict(trace=[[_hex(it[k]) for k in TRACE_FIELDS] for it in trace],
                summary={f: _hex(getattr(sm, f)) for f in SUMMARY_FIELDS}, params_sha256=h.hexdigest())


def dump_fixture(entries, path):
    """entries: key -> dict(reproduces=..., record=...).  Equal records are
    stored once (the three loop settings leave the same bits on a scene), one
    per line, and every entry names its record by index."""
    records, index, named = [], {}, {}
    for key, e in entries.items():
        blob = json.dumps(e["record"], sort_keys=True)
        if blob not in index:
            index[blob] = len(records)
            records.append(blob)
        named[key] = dict(e, record=index[blob])
    with open(path, "w") as f:
        f.write('{"trace_fields": %s,\n"entries": %s,\n"records": [\n%s\n]}\n'
                % (json.dumps(TRACE_FIELDS), json.dumps(named), ",\n".join(records)))


def load_fixture(path=os.path.join(G, "lm_loop_parent.json")):
    """-> key -> dict(reproduces=..., record=...)"""
    fix = json.load(open(path))
    assert tuple(fix["trace_fields"]) == TRACE_FIELDS
    return {key: dict(e, record=fix["records"][e["record"]]) for key, e in fix["entries"].items()}


def record(name, env):
    """One-shot solve (sfm_ba_solve) of scene `name` under ENVS[env]."""
    import sfm_amd
    s, mode, opts = build(name)
    saved = {k: os.environ.pop(k, None) for k in LOOP_VARS}
    try:
        os.environ.update(ENVS[env])
        r, t, X = s.copy_params()
        sm, tr = sfm_amd.solve(s.uv, s.cam_idx, s.pt_idx, s.K, r, t, X, mode=mode, options=sfm_amd.make_options(**opts))
    finally:
        for k in LOOP_VARS:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]
    return as_record(sm, tr, r, t, X)


def _rank_body(rank, world, port, q):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    import torch.distributed as dist
    import sfm_amd
    from sfm_amd import scene
    import test_gpu_shards as TS
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    per = TS.P // world
    sc = scene.generate(TS.C, TS.P, views=TS.VIEWS, seed=TS.SEED, p_begin=rank * per, p_end=(rank + 1) * per)

    def allreduce(arr, op):
        dist.all_reduce(torch.from_numpy(arr), op=dist.ReduceOp.MAX if op == 1 else dist.ReduceOp.SUM)

    with sfm_amd.BundleAdjuster(0) as ba:
        ba.set_host_comm(world, rank, allreduce)
        ba.set_problem(sc.uv, sc.cam_idx, sc.pt_idx, sc.K, sc.rot, sc.t, sc.X)
        sm, tr = ba.solve()
        rot, t, X = ba.parameters()
    q.put((rank, as_record(sm, tr, rot, t, X)))
    dist.barrier()
    dist.destroy_process_group()


def _rank(rank, world, port, q):
    import test_gpu_shards as TS
    TS._guarded(_rank_body)(rank, world, port, q)


def record_two_ranks():
    """test_gpu_shards.py's smallest configuration (two ranks, STRUCT_AND_POSE,
    replicated factor) through sfm_ba_set_host_comm over gloo -> one record per
    rank.  (A two-rank sum is the same in either order.)"""
    import torch.multiprocessing as mp
    import test_gpu_shards as TS
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = TS._free_port()
    procs = [ctx.Process(target=_rank, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = TS._collect(procs, q, world, 150)
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    return [r[1] for r in res]
