"""tests/golden/refine_ext/refine_ext_small.npz: the recipe (tests/golden/make_refine_ext.py) still gives the file on
the host, and sm_run with refine()'s three extra stages on gives its maps on the GPU."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import make_refine_ext as M  # noqa: E402

PATH = os.path.join(ROOT, "tests", "golden", "refine_ext", "refine_ext_small.npz")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(PATH))


def test_fixture_is_the_recipe(fx):
    d = M.build()
    assert set(d) == set(fx)
    for k in d:
        if d[k].dtype == np.float32:
            np.testing.assert_array_equal(bits(d[k]), bits(fx[k]), err_msg=k)
        else:
            np.testing.assert_array_equal(d[k], fx[k], err_msg=k)
    assert 0.05 < fx["mask"].mean() < 0.95 and (fx["disp"] >= 0).all()
    assert (fx["se_reference"] == np.trunc(fx["se_reference"])).all() and (fx["se_float"] != fx["se_reference"]).any()
    assert os.path.getsize(PATH) < 1 << 20


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1])
def test_gpu_gives_the_fixture(fx, mode):
    from mystereomatching_amd import StereoBatch
    sb = StereoBatch(M.D - 1, M.H, M.W, 1, device=0, do_refine=1,
                     refine_ext=dict(do_pkr=True, do_bg_ipol=True, do_subpixel=True, se_mode=mode))
    try:
        sb.upload(*(fx[k][None] for k in M.KEYS))
        np.testing.assert_array_equal(sb.run(0.3)[0], fx["disp"])
        np.testing.assert_array_equal(sb.get_pkr_mask(), fx["mask"])
        np.testing.assert_array_equal(bits(sb.download_subpixel()[0]), bits(fx["se_float" if mode else "se_reference"]))
    finally:
        sb.close()
