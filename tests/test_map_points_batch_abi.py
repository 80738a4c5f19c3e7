"""CPU: sfm_matcher_pair_points_first is declared and exported, refuses a
NULL handle without a device, and LiveSfM's batch_pairs needs device_mapping."""
import ctypes
import os
import re

import numpy as np
import pytest

import sfm_amd
from sfm_amd._ffi import lib, ptr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "sfm_matcher_pair_points_first"


def test_symbol_is_declared_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "sfm_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    decl = re.search(r"\bint\s+" + NAME + r"\s*\(([^;]*)\)\s*;", src)
    assert decl, "not declared in include/sfm_amd.h"
    args = [a.strip() for a in decl.group(1).split(",")]
    assert len(args) == 25 and args[0] == "sfm_matcher* h" and args[1] == "int32_t n_pairs"
    assert hasattr(ctypes.CDLL(sfm_amd.LIB_PATH), NAME)
    assert NAME in sfm_amd.exported_symbols()
    assert len(getattr(lib(), NAME).argtypes) == 25


def test_null_handle_is_refused_without_a_device():
    z = np.zeros(16, np.int32)
    d = np.zeros(16)
    first = ctypes.c_int32(5)
    rc = getattr(lib(), NAME)(None, 1, ptr(z), ptr(z), ptr(z), 1, ptr(z), 2, 0.8, 1.5, 40.0, ptr(d), ptr(d), ptr(d),
                              ptr(d), ptr(d), ptr(d), 7.0, 4, ctypes.byref(first), ptr(z), ptr(z), ptr(d), ptr(z),
                              ptr(z))
    assert rc == -22 and lib().sfm_last_error()


def test_batch_pairs_needs_device_mapping():
    from sfm_amd.live import LiveSfM
    with pytest.raises(ValueError, match="device_mapping"):
        LiveSfM(batch_pairs=True)
    with pytest.raises(ValueError, match="device_mapping"):
        LiveSfM(device_mapping=False, batch_pairs=True)
