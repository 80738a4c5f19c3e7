"""CPU: bench.py's multi-GPU launch contract.

`bench.py --gpus N` started without a launcher (no WORLD_SIZE) must start
N ranks itself -- one process per GPU through torch.distributed.run on
127.0.0.1 -- before any GPU call, and report n_gpus from the communicator's
rank count.  --dry-run stops each rank after the rendezvous and one gloo
all-reduce (no GPU call), so this runs here."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env_extra=None):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env.update(env_extra or {})
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True,
                       text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout   # one JSON line, from rank 0 only
    return json.loads(lines[0])


def test_gpus_2_self_launches_two_ranks():
    out = _run(["--gpus", "2", "--dry-run"])
    assert out["dry_run"] and out["n_gpus"] == 2 and out["ranks_reporting"] == 2


def test_gpus_1_runs_in_process():
    out = _run(["--gpus", "1", "--dry-run"])
    assert out["n_gpus"] == 1 and out["ranks_reporting"] == 1


def test_plain_and_full_options_parse():
    out = _run(["--gpus", "1", "--steps", "3", "--warmup", "1", "--full", "--dump-outputs", "unused", "--dry-run"])
    assert out["dry_run"] and out["n_gpus"] == 1


def test_dump_outputs_files(tmp_path):
    """--dump-outputs: float64 .npy files of the last solve's results, no
    wall-clock field among them, an oversized X cut to the same seeded sample
    of its rows on every call, below 64 MB in all."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    from sfm_amd._ffi import BASummary

    rng = np.random.default_rng(3)
    n_big = bench.DUMP_X_BYTES // 24 + 1000
    sm = BASummary()
    sm.num_iterations, sm.final_cost, sm.wall_time_s = 3, 655.0, 0.123
    trace = [{k: float(i) for k in bench.DUMP_TRACE_FIELDS} for i in range(4)]
    outs = {"rot": rng.normal(size=(5, 3)), "t": rng.normal(size=(5, 3)), "X": np.arange(3.0 * n_big).reshape(n_big, 3),
            "summary": sm, "trace": trace}
    got = []
    for d in (tmp_path / "a", tmp_path / "b"):
        bench.dump_outputs(str(d), outs, 1, 0)
        got.append({p.name: np.load(p) for p in sorted(d.iterdir())})
    a, b = got
    assert sorted(a) == ["X.npy", "rot.npy", "summary.npy", "t.npy", "trace.npy"]
    assert all(v.dtype == np.float64 for v in a.values())
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert np.array_equal(a["rot.npy"], outs["rot"]) and np.array_equal(a["t.npy"], outs["t"])
    assert a["X.npy"].shape == (bench.DUMP_X_BYTES // 24, 3)
    idx = (a["X.npy"][:, 0] / 3).astype(np.int64)   # row i of X starts with 3 i
    assert np.all(np.diff(idx) > 0) and np.array_equal(a["X.npy"], outs["X"][idx])
    assert a["summary.npy"].shape == (len(bench.DUMP_SUMMARY_FIELDS),) and 0.123 not in a["summary.npy"]
    assert a["summary.npy"][bench.DUMP_SUMMARY_FIELDS.index("final_cost")] == 655.0
    assert a["trace.npy"].shape == (4, len(bench.DUMP_TRACE_FIELDS))
    # a small X is written whole
    outs["X"] = outs["X"][:7]
    bench.dump_outputs(str(tmp_path / "c"), outs, 1, 0)
    assert np.array_equal(np.load(tmp_path / "c" / "X.npy"), outs["X"])
