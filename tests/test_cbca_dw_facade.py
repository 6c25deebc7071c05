"""The facades with cbca_double_win set give the C ABI's map.

tests/cpp/cbca_dw_facade_check.cpp sets param.cbca_double_win / param.GF_double_win on the C++ facade
(include/stereo_matching.hpp), runs costCalculate -> SolveAll -> dispOptimize on one pair and writes DP[0]; the
Python mirror does the same with StereoMatching.Parameters.  Both are compared with a StereoBatch configured
through sm_cbca_double_config (that path is pinned against the restatement in tests/test_gpu_cbca_dw.py).
"""
import os
import subprocess

import numpy as np
import pytest

import pyref_cbca_dw as P
from mystereomatching_amd import SolveAll, StereoBatch, StereoMatching
from test_cpp_facade import _compile, write_ppm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, MD = 40, 56, 15


@pytest.fixture(scope="module")
def pair():
    return P.make_input(H, W, MD + 1, 0)   # (the facade reads its gray images from the colour files: the same ones)


@pytest.fixture(scope="module")
def capi_maps(pair):
    maps = {}
    for on in (False, True):
        sb = StereoBatch(MD, H, W, 1, cbca_double_win=on)
        try:
            sb.upload(*(pair[k][None] for k in ("lbgr", "rbgr", "lgray", "rgray")))
            maps[on] = sb.run(0.3)[0].copy()
        finally:
            sb.close()
    assert (maps[True] != maps[False]).any()
    return maps


def test_cpp_facade_double_win(tmp_path, pair, capi_maps):
    exe = str(tmp_path / "cbca_dw_facade_check")
    _compile(os.path.join(ROOT, "tests", "cpp", "cbca_dw_facade_check.cpp"), exe)
    write_ppm(tmp_path / "l.ppm", pair["lbgr"])
    write_ppm(tmp_path / "r.ppm", pair["rbgr"])
    for dw, gf in ((1, 0), (0, 0), (0, 1)):
        out = tmp_path / f"dp{dw}{gf}.i16"
        r = subprocess.run([exe, str(tmp_path / "l.ppm"), str(tmp_path / "r.ppm"), str(MD), str(dw), str(gf), str(out)],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert "window1 23 23 30 0" in r.stdout
        got = np.fromfile(out, np.int16).reshape(H, W)
        np.testing.assert_array_equal(got, capi_maps[bool(dw)], err_msg=f"cbca_double_win={dw} GF_double_win={gf}")


def test_python_mirror_double_win(pair, capi_maps):
    StereoMatching.costcalculation, StereoMatching.aggregation, StereoMatching.optimization = "censusGrad", "CBCA", "sgm"
    for dw, gf in ((True, False), (False, True)):
        prm = StereoMatching.Parameters(MD, H, W)
        prm.cbca_double_win, prm.GF_double_win = dw, gf
        sm = StereoMatching(pair["lbgr"], pair["rbgr"], pair["lgray"], pair["rgray"], None, None, None, None, prm)
        sm.costCalculate()
        SolveAll([sm], 1, 0.3)
        np.testing.assert_array_equal(sm.dispOptimize(), capi_maps[dw])
