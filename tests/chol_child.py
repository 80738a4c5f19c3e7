"""The dense Cholesky GPU tests' work lists, runnable in this process or in a
child (`python -m tests.chol_child MODE [ARG]`, one JSON line on stdout): the
kernels' knobs (SFM_CHOL_NO_SMALL, SFM_CHOL_HELPERS, SFM_CHOL_TEST_SKEW) are
read once per process, so every other setting needs a process of its own.
Solutions travel as hex of their bytes: the comparisons are bitwise.
"""
import json
import os
import subprocess
import sys

import numpy as np

from tests import chol_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _solve(A, b, reps=1):
    from sfm_amd.ba import dense_spd_solve
    y, _, fl = dense_spd_solve(A, b, reps=reps)
    return [y.tobytes().hex(), int(fl)]


def unhex(h):
    return np.frombuffer(bytes.fromhex(h), dtype=np.float64)


def well(n):
    """(A, b): the matrix family the suite began with (tests/test_gpu_parity.py)."""
    rng = np.random.default_rng(n)
    M = rng.standard_normal((n, n))
    return M @ M.T + n * np.eye(n), rng.standard_normal(n)


def run_spd(_arg=None):
    """Every SPD case x right-hand side, then the garbage-lower twins."""
    out = {}
    for fam, n in C.spd_ids():
        A = C.matrix(fam, n)
        B = C.rhs_block(fam, n, A)
        for k, rhs in enumerate(C.RHS):
            out[f"{fam}-{n}-{rhs}"] = _solve(A, B[:, k])
    for n in (65, 192):
        A = C.matrix("scaled", n)
        out[f"garbage-{n}"] = _solve(C.garbage_lower(A), C.rhs_block("scaled", n, A)[:, 0])
    return out


def run_nonspd(_arg=None):
    """Every non-SPD case (its fail word), each followed at once by an SPD
    solve of the same size, which must be right whatever the failed factor
    left behind."""
    out = {}
    spd = {n: C.matrix("well", n) for n in C.NONSPD_SIZES}
    rhs = {n: C.rhs_block("well", n, spd[n])[:, 0] for n in C.NONSPD_SIZES}
    for kind, n, p in C.nonspd_ids():
        A, _ = C.nonspd(kind, n, p)
        out[f"{kind}-{n}-{p}"] = _solve(A, np.ones(n))[1]
        out[f"after-{kind}-{n}-{p}"] = _solve(spd[n], rhs[n])
    return out


def run_bits(sizes):
    """y of the `well` system at each size (the knob comparisons)."""
    return {str(n): _solve(*well(n)) for n in sizes}


def run_parity(_arg=None):
    """tests/test_gpu_parity.py's dense cases."""
    out = {}
    for n in (6, 63, 64, 65, 130, 600, 3000):
        out[f"solve-{n}"] = _solve(*well(n), reps=3 if n >= 600 else 1)
    for n in (100, 700):
        A = np.eye(n)
        A[n // 2, n // 2] = -1.0
        out[f"indefinite-{n}"] = _solve(A, np.ones(n))[1]
    return out


def skew_steps():
    """(fast-path steps, steps) of the skewed walkers since the last call."""
    import ctypes
    import sfm_amd
    buf = (ctypes.c_ulonglong * 2)()
    f = sfm_amd.lib().sfm_debug_chol_skew_steps
    f.argtypes, f.restype = [ctypes.c_void_p], ctypes.c_int
    assert f(buf) == 0
    return int(buf[0]), int(buf[1])


def run_skew(sizes):
    out = {}
    for n in sizes:
        skew_steps()
        out[str(n)] = _solve(*well(n)) + list(skew_steps())
    return out


MODES = {"spd": run_spd, "nonspd": run_nonspd, "bits": run_bits, "parity": run_parity, "skew": run_skew}


def in_child(mode, arg=None, **env):
    """MODES[mode](arg) in a child process with `env` added to the environment."""
    r = subprocess.run([sys.executable, "-m", "tests.chol_child", mode, json.dumps(arg)], env=dict(os.environ, **env),
                       cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


if __name__ == "__main__":
    print(json.dumps(MODES[sys.argv[1]](json.loads(sys.argv[2]) if len(sys.argv) > 2 else None)))
