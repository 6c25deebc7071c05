"""The facades with cbca_intersect = false give the C ABI's map.

tests/cpp/cbca_ni_facade_check.cpp sets param.cbca_intersect on the C++ facade (include/stereo_matching.hpp), runs
costCalculate -> SolveAll -> dispOptimize on one pair and writes DP[0]; the Python mirror does the same with
StereoMatching.Parameters.  Both are compared with a StereoBatch configured through sm_cbca_intersect_config (that
path is pinned against the restatement in tests/test_gpu_cbca_ni.py).
"""
import os
import subprocess

import numpy as np
import pytest

import pyref_cbca_ni as P
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
    for intersect in (True, False):
        sb = StereoBatch(MD, H, W, 1, cbca_intersect=intersect)
        try:
            sb.upload(*(pair[k][None] for k in ("lbgr", "rbgr", "lgray", "rgray")))
            maps[intersect] = sb.run(0.3)[0].copy()
        finally:
            sb.close()
    assert (maps[True] != maps[False]).any()
    return maps


def test_cpp_facade_intersect(tmp_path, pair, capi_maps):
    exe = str(tmp_path / "cbca_ni_facade_check")
    _compile(os.path.join(ROOT, "tests", "cpp", "cbca_ni_facade_check.cpp"), exe)
    write_ppm(tmp_path / "l.ppm", pair["lbgr"])
    write_ppm(tmp_path / "r.ppm", pair["rbgr"])
    for intersect in (0, 1):
        out = tmp_path / f"dp{intersect}.i16"
        r = subprocess.run([exe, str(tmp_path / "l.ppm"), str(tmp_path / "r.ppm"), str(MD), str(intersect), str(out)],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert "default cbca_intersect 1" in r.stdout
        got = np.fromfile(out, np.int16).reshape(H, W)
        np.testing.assert_array_equal(got, capi_maps[bool(intersect)], err_msg=f"cbca_intersect={intersect}")


def test_python_mirror_intersect(pair, capi_maps):
    StereoMatching.costcalculation, StereoMatching.aggregation, StereoMatching.optimization = "censusGrad", "CBCA", "sgm"
    for intersect in (False, True):
        prm = StereoMatching.Parameters(MD, H, W)
        prm.cbca_intersect = intersect
        sm = StereoMatching(pair["lbgr"], pair["rbgr"], pair["lgray"], pair["rgray"], None, None, None, None, prm)
        sm.costCalculate()
        SolveAll([sm], 1, 0.3)
        np.testing.assert_array_equal(sm.dispOptimize(), capi_maps[intersect], err_msg=f"cbca_intersect={intersect}")


def test_other_aggregations_ignore_the_field(pair):
    """Only the CBCA functions read cbca_intersect: with another aggregation the field changes nothing."""
    StereoMatching.costcalculation, StereoMatching.aggregation, StereoMatching.optimization = "censusGrad", "BF", "sgm"
    try:
        maps = []
        for intersect in (True, False):
            prm = StereoMatching.Parameters(MD, H, W)
            prm.cbca_intersect = intersect
            sm = StereoMatching(pair["lbgr"], pair["rbgr"], pair["lgray"], pair["rgray"], None, None, None, None, prm)
            sm.costCalculate()
            SolveAll([sm], 1, 0.3)
            maps.append(sm.dispOptimize().copy())
        np.testing.assert_array_equal(maps[0], maps[1])
    finally:
        StereoMatching.aggregation = "CBCA"
