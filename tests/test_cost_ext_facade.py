"""tests/cpp/cost_ext_facade_check.cpp: the C++ facade (include/stereo_matching.hpp) with the cost strings
of sm_cost_ext.hip.  `costcalculation = "adGrad"` gives the C ABI's map; "ZNCC" stays refused with the
facade's invalid_argument (no device needed for that)."""
import functools
import os
import subprocess

import numpy as np
import pytest

from mystereomatching_amd import StereoBatch
from mystereomatching_amd import synthetic as S
from test_cpp_facade import _compile, write_ppm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("lbgr", "rbgr", "lgray", "rgray")
H, W, MD = 20, 26, 15


@functools.lru_cache(maxsize=None)
def _exe(tmp):
    exe = os.path.join(tmp, "cost_ext_facade_check")
    _compile(os.path.join(ROOT, "tests", "cpp", "cost_ext_facade_check.cpp"), exe)
    return exe


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("cost_ext_facade")
    pair = S.make_pair(H, W, MD + 1, 980)
    pair = {k: pair[k] for k in ("lbgr", "rbgr")}
    # the facade reads the gray images from the colour files (imread flags 0: libpng's weights)
    pair["lgray"], pair["rgray"] = S.bgr_to_gray(pair["lbgr"]), S.bgr_to_gray(pair["rbgr"])
    write_ppm(tmp / "l.ppm", pair["lbgr"])
    write_ppm(tmp / "r.ppm", pair["rbgr"])
    return str(tmp), pair


def _run(tmp, cost):
    out = os.path.join(tmp, f"dp_{cost}.i16")
    r = subprocess.run([_exe(tmp), cost, os.path.join(tmp, "l.ppm"), os.path.join(tmp, "r.ppm"), str(MD), out],
                       capture_output=True, text=True, timeout=120)
    return r, out


def test_zncc_is_refused_by_the_cpp_facade(files):
    tmp, _ = files
    r, _ = _run(tmp, "ZNCC")
    assert r.returncode == 4 and "unsupported costcalculation: ZNCC" in r.stderr, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.gpu
@pytest.mark.parametrize("cost", ["adGrad", "BT"])
def test_cpp_facade_matches_the_c_abi(files, cost):
    tmp, pair = files
    r, out = _run(tmp, cost)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = np.fromfile(out, np.int16).reshape(H, W)
    sb = StereoBatch(MD, H, W, 1, device=0, cost_method=cost, num_streams=1)
    try:
        sb.upload(*(pair[k][None] for k in KEYS))
        want = sb.run(0.3)[0]
    finally:
        sb.close()
    np.testing.assert_array_equal(got, want)
    sb = StereoBatch(MD, H, W, 1, device=0, num_streams=1)
    try:
        sb.upload(*(pair[k][None] for k in KEYS))
        assert (sb.run(0.3)[0] != got).any()      # the string reached the kernels
    finally:
        sb.close()
