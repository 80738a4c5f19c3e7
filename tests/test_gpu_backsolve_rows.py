"""The back substitution's row groups (k_backsolve<R>, R block rows per
workgroup) leave every bit of y where the single-row kernel of the parent
commit put it.

tests/golden/backsolve_parent.json holds the SHA-256 of y's bytes and the
fail word of dense_spd_solve on tests/chol_child.py's `well(n)` systems,
recorded on the parent commit by tests/golden/make_backsolve_parent.py, on
the default path and under SFM_CHOL_NO_SMALL=1.  The sizes are the smallest
that reach every group shape (nb = ceil(n / 64) block rows): nb = 1 and 2,
both residues of nb mod 2 and all three of nb mod 3 with whole and partial
last blocks, one full group, and many groups (nb = 10, 20, 47: the bench
configurations C2's and C3's).

Every comparison is bitwise; nothing here has a tolerance.
"""
import functools
import hashlib
import json
import os

import pytest

from tests import chol_child as K

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 257, 320, 321, 384, 385, 449, 639, 1279, 3007)
PATHS = {"default": {}, "no_small": {"SFM_CHOL_NO_SMALL": "1"}}
# epoch and ticket reuse, late polls: a partial last group at R = 2 (nb = 4
# and 7 at R = 3: a partial and a partial again) with a partial last block
REUSE_SIZES = (193, 385)
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "backsolve_parent.json")


@functools.lru_cache(maxsize=None)
def _parent():
    with open(FIXTURE) as f:
        return json.load(f)


def _digest(entry):
    return dict(sha256=hashlib.sha256(bytes.fromhex(entry[0])).hexdigest(), fail=int(entry[1]))


@functools.lru_cache(maxsize=None)
def _bits(path):
    """y of every size on one path, solved once (default: in this process)."""
    if path == "default":
        return K.run_bits(list(SIZES))
    return K.in_child("bits", list(SIZES), **PATHS[path])


def test_fixture_is_complete():
    fx = _parent()
    assert sorted(fx) == sorted(f"{p}/{n}" for p in PATHS for n in SIZES)
    for key, e in fx.items():
        assert e["reproduces"] is True, key
        assert e["record"]["fail"] == 0 and len(e["record"]["sha256"]) == 64, key


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("path", list(PATHS))
def test_bits_equal_the_parent(path, n):
    got = _digest(_bits(path)[str(n)])
    assert got == _parent()[f"{path}/{n}"]["record"], (path, n)


@pytest.mark.parametrize("n", REUSE_SIZES)
def test_epoch_and_ticket_reuse_same_bits(n):
    """reps = 3 runs epochs 1..3 on the same y, flags and group tickets: the
    ticket of epoch e is counted from (e - 1) * (groups per launch)."""
    A, b = K.well(n)
    assert _digest(K._solve(A, b, reps=3)) == _parent()[f"default/{n}"]["record"]


def test_late_factor_same_bits():
    """One helper workgroup: the factor ahead of the back substitution ends
    late and in another order, so the groups' polls wait."""
    got = K.in_child("bits", list(REUSE_SIZES), SFM_CHOL_HELPERS="1")
    for n in REUSE_SIZES:
        assert _digest(got[str(n)]) == _parent()[f"default/{n}"]["record"], n
