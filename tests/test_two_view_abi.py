"""CPU: the parts of sfm_two_view_init that need no device -- the option
defaults and struct layout of include/sfm_amd.h, argument checks (non-finite
input and bad options are SFM_EINVAL), n < 15 returning model 0, and
SFM_ENODEV without a GPU, as the other entry points."""
import ctypes

import numpy as np
import pytest

import sfm_amd
from sfm_amd._ffi import TwoViewOptions, default_two_view_options
from tests import two_view_ref as T
from tests.two_view_cases import K, scene


def test_default_options_are_the_reference_constants():
    o = default_two_view_options()
    got = {name: getattr(o, name) for name, _ in TwoViewOptions._fields_}
    assert got == T.DEFAULTS                      # the restatement's defaults: CSfM.cpp:843, :849-850, :859, :35
    assert ctypes.sizeof(TwoViewOptions) == 11 * 8 + 2 * 4
    assert sfm_amd.lib().sfm_abi_version() == 1   # an addition: the ABI version stays


def test_fewer_than_fifteen_matches_give_no_model_without_a_device():
    p = np.random.default_rng(0).uniform(0, 700, (14, 2)).astype(np.float32)
    r = sfm_amd.two_view_init(p, p + 3, K)
    assert r.model == 0 and not r.ok and r.n_kept == 0 and r.keep.shape == (14,) and r.X.shape == (14, 3)
    assert sfm_amd.two_view_init(np.zeros((0, 2)), np.zeros((0, 2)), K).model == 0


def test_bad_arguments_are_rejected_before_the_device_is_touched():
    s = scene("n65")
    p1 = s["p1"].copy()
    p1[3, 0] = np.inf
    for args, kw in (((s["p0"], p1, K), {}), ((s["p0"], s["p1"], K * np.nan), {}),
                     ((s["p0"], s["p1"], K), dict(f_max_iters=5000)), ((s["p0"], s["p1"], K), dict(f_confidence=1.0)),
                     ((s["p0"], s["p1"], K), dict(max_repr_err=float("nan")))):
        with pytest.raises(sfm_amd.SfmError) as e:
            sfm_amd.two_view_init(*args, **kw)
        assert e.value.code == -22
    with pytest.raises(ValueError):
        sfm_amd.two_view_init(s["p0"], s["p1"][:-1], K)
    with pytest.raises(TypeError):
        sfm_amd.two_view_init(s["p0"], s["p1"], K, no_such_option=1)


def test_fails_loudly_without_a_device():
    if sfm_amd.device_count() > 0:
        return
    s = scene("n65")
    with pytest.raises(sfm_amd.SfmError) as e:
        sfm_amd.two_view_init(s["p0"], s["p1"], K)
    assert e.value.code == -19


def test_drivers_reject_an_unknown_init_mode():
    from sfm_amd.live import LiveSfM
    from sfm_amd.mapping import IncrementalMapper
    with pytest.raises(ValueError):
        LiveSfM(init="guess")
    with pytest.raises(ValueError):
        IncrementalMapper(init="guess")
