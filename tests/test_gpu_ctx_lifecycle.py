"""GPU: one context through every feature switch that releases and reallocates device buffers (the candidate
tables of vmTop, the double window's second arm planes, the volume sets of the placement trials), against
fresh contexts with the same settings.  All comparisons are exact (int16 maps).  Nothing here reads the
device's free memory: the cards are shared, so that number is not this process's alone.
"""
import numpy as np
import pytest

from mystereomatching_amd import StereoBatch
from mystereomatching_amd import synthetic as S

pytestmark = pytest.mark.gpu

KEYS = ("lbgr", "rbgr", "lgray", "rgray")
H, W, MD, N = 30, 52, 31, 2


@pytest.fixture(scope="module")
def batch():
    return S.make_batch(N, H, W, MD + 1, first_index=700)


def _run(sb, batch):
    sb.upload(*(batch[k] for k in KEYS))
    return sb.run(0.3)


def _fresh(batch, config=None, **overrides):
    """The maps of a new context: `config` applies the settings under test before the first run."""
    sb = StereoBatch(MD, H, W, N, device=0, **overrides)
    try:
        if config:
            config(sb)
        return _run(sb, batch)
    finally:
        sb.close()


@pytest.fixture(scope="module")
def plain(batch):
    return _fresh(batch)


def test_feature_switches_on_one_context(batch, plain):
    steps = [
        # vmTop: the candidate table is sized for num 2, then reallocated for num 4
        ("vmtop num 2", lambda sb: sb.vmtop_config(True, num=2)),
        ("vmtop num 4", lambda sb: sb.vmtop_config(True, num=4)),
        ("vmtop off", lambda sb: sb.vmtop_config(False, num=4)),
        # the double window: window 1's arm planes are padded for lag 23, then reallocated for lag 12
        ("double window, arm_l_out2 23", lambda sb: sb.cbca_double_config(True, arm_l_out2=23)),
        ("double window, arm_l_out2 12", lambda sb: sb.cbca_double_config(True, arm_l_out2=12)),
        ("double window off", lambda sb: sb.cbca_double_config(False, arm_l_out2=12)),
        ("intersection off", lambda sb: sb.cbca_intersect_config(False)),
        ("intersection on", lambda sb: sb.cbca_intersect_config(True)),
    ]
    sb = StereoBatch(MD, H, W, N, device=0)
    try:
        np.testing.assert_array_equal(_run(sb, batch), plain)
        got = plain
        for name, config in steps:
            config(sb)
            got = _run(sb, batch)
            np.testing.assert_array_equal(got, _fresh(batch, config), err_msg=name)
        np.testing.assert_array_equal(got, plain, err_msg="after the last switch")
    finally:
        sb.close()


def test_placement_trials(batch, plain):
    sb = StereoBatch(MD, H, W, N, device=0, placement_trials=2)
    try:
        for _ in range(2):   # the first run holds two volume sets and frees the slower one
            np.testing.assert_array_equal(_run(sb, batch), plain)
    finally:
        sb.close()
