"""GPU: the culling members of the C++ drop-in (sfm_compat::MapStore,
include/sfm_ctracker_compat.hpp) on the pinned case, through
tests/compat/compat_cull_gpu.cpp, which checks every output itself."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "compat", "bin", "compat_cull_gpu")


@pytest.mark.parametrize("desc_bytes", [64, 16])
def test_map_store_culling_drop_in(desc_bytes):
    assert os.path.exists(EXE), f"{EXE} missing: __graft_entry__.build() compiles it"
    out = subprocess.run([EXE, str(desc_bytes)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "compat_cull_gpu ok" in out.stdout
