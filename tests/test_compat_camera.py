"""include/sfm_ctracker_compat.hpp: the camera templates
(getOptimalNewCameraMatrix, undistortPoints) compile against stub types and
return the restatement's Kopt exactly (host arithmetic, no GPU here)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import camera_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "sfm_amd", "libsfm_amd.so")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    assert os.path.exists(LIB), "libsfm_amd.so not built"
    out = tmp_path_factory.mktemp("compat_camera") / "compat_camera_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "compat", "compat_camera_check.cpp"), "-L", os.path.dirname(LIB),
                    "-lsfm_amd", "-Wl,-rpath," + os.path.dirname(LIB), "-o", str(out)], check=True)
    return str(out)


def _run(exe, size, K, d):
    args = [exe, str(size[0]), str(size[1])] + [float(v).hex() for v in (K[0, 0], K[1, 1], K[0, 2], K[1, 2])]
    args += [float(v).hex() for v in d]
    out = subprocess.run(args, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    return int(lines[0].split()[1]), np.array([float.fromhex(t) for t in lines[1].split()]).reshape(3, 3), lines[2]


@pytest.mark.parametrize("size", R.SIZES)
@pytest.mark.parametrize("name", ["L1", "L2", "L3", "L4"])
def test_compat_kopt_equals_the_restatement(exe, name, size):
    K, d = R.k_for(size), R.LENSES[name]
    rc, Kopt, tail = _run(exe, size, K, d)
    assert rc == 0
    assert np.array_equal(Kopt, R.optimal_new_camera_matrix(K, d, size))
    assert tail == "empty 0 size 0 bad -22"


def test_compat_reports_errors_and_leaves_kopt(exe):
    rc, Kopt, _ = _run(exe, (1280, 720), R.K_MAIN, [0.1, 0.2, 0.3])   # three coefficients
    assert rc == -22 and (Kopt == -1).all()
