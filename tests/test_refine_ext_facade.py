"""The facades with refine()'s extra switches set give the C ABI's maps.

tests/cpp/refine_ext_facade_check.cpp sets Do_refine, Do_calPKR, Do_bgIpol, Do_subpixelEnhancement and SE_FLOAT on
the C++ facade (include/stereo_matching.hpp), runs costCalculate -> SolveAll -> dispOptimize -> refine on one pair
and writes DP[0], SE and PKR_Err_Mask; the Python mirror does the same with StereoMatching's class attributes.
Both are compared with a StereoBatch configured through sm_refine_ext_config (that path is pinned against the
restatement in tests/test_gpu_refine_ext.py).
"""
import os
import subprocess

import numpy as np
import pytest

from mystereomatching_amd import SolveAll, StereoBatch, StereoMatching, _capi
from mystereomatching_amd import synthetic as S
from test_cpp_facade import _compile, write_ppm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, MD = 40, 56, 15
KEYS = ("lbgr", "rbgr", "lgray", "rgray")
CASES = [(1, 1, 1, 0), (1, 1, 1, 1), (0, 1, 0, 0), (0, 0, 0, 0)]   # PKR, BG, SE, SE_FLOAT


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def pair():
    p = S.make_pair(H, W, MD + 1, 640)   # (the facade reads its gray images from the colour files: the same ones)
    return {k: p[k] for k in KEYS}


@pytest.fixture(scope="module")
def capi(pair):
    out = {}
    for pkr, bg, se, flt in CASES:
        sb = StereoBatch(MD, H, W, 1, do_refine=1,
                         refine_ext=dict(do_pkr=pkr, do_bg_ipol=bg, do_subpixel=se, se_mode=_capi.SE_FLOAT if flt else _capi.SE_REFERENCE))
        try:
            sb.upload(*(pair[k][None] for k in KEYS))
            r = {"disp": sb.run(0.3)[0].copy()}
            if pkr:
                r["mask"] = sb.get_pkr_mask()
            if se:
                r["se"] = sb.download_subpixel()[0].copy()
        finally:
            sb.close()
        out[(pkr, bg, se, flt)] = r
    assert (out[(1, 1, 1, 0)]["disp"] != out[(0, 0, 0, 0)]["disp"]).any()
    assert (out[(1, 1, 1, 0)]["se"] != out[(1, 1, 1, 1)]["se"]).any()
    return out


def test_cpp_facade_refine_ext(tmp_path, pair, capi):
    exe = str(tmp_path / "refine_ext_facade_check")
    _compile(os.path.join(ROOT, "tests", "cpp", "refine_ext_facade_check.cpp"), exe)
    write_ppm(tmp_path / "l.ppm", pair["lbgr"])
    write_ppm(tmp_path / "r.ppm", pair["rbgr"])
    for case in CASES:
        tag = "".join(str(x) for x in case)
        dp, se, mask = (tmp_path / f"{n}{tag}" for n in ("dp", "se", "mask"))
        r = subprocess.run([exe, str(tmp_path / "l.ppm"), str(tmp_path / "r.ppm"), str(MD), *(str(x) for x in case),
                            str(dp), str(se), str(mask)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert "DISP_PKR -64 bgIplDepth 1000" in r.stdout
        want = capi[case]
        np.testing.assert_array_equal(np.fromfile(dp, np.int16).reshape(H, W), want["disp"], err_msg=tag)
        if case[0]:
            np.testing.assert_array_equal(np.fromfile(mask, np.uint8).reshape(H, W), want["mask"], err_msg=tag)
        if case[2]:
            np.testing.assert_array_equal(bits(np.fromfile(se, np.float32).reshape(H, W)), bits(want["se"]), err_msg=tag)


def test_python_mirror_refine_ext(pair, capi):
    cls = StereoMatching
    saved = (cls.costcalculation, cls.aggregation, cls.optimization, cls.Do_refine, cls.Do_calPKR, cls.Do_bgIpol,
             cls.Do_subpixelEnhancement, cls.SE_FLOAT)
    try:
        cls.costcalculation, cls.aggregation, cls.optimization, cls.Do_refine = "censusGrad", "CBCA", "sgm", True
        for case in CASES:
            cls.Do_calPKR, cls.Do_bgIpol, cls.Do_subpixelEnhancement, cls.SE_FLOAT = (bool(x) for x in case)
            sm = StereoMatching(pair["lbgr"], pair["rbgr"], pair["lgray"], pair["rgray"], None, None, None, None,
                                StereoMatching.Parameters(MD, H, W))
            sm.costCalculate()
            SolveAll([sm], 1, 0.3)
            sm.dispOptimize()
            want = capi[case]
            np.testing.assert_array_equal(sm.refine(), want["disp"])
            if case[0]:
                np.testing.assert_array_equal(sm.PKR_Err_Mask, want["mask"])
            else:
                assert sm.PKR_Err_Mask is None
            if case[2]:
                np.testing.assert_array_equal(bits(sm.SE), bits(want["se"]))
            else:
                assert sm.SE is None
    finally:
        (cls.costcalculation, cls.aggregation, cls.optimization, cls.Do_refine, cls.Do_calPKR, cls.Do_bgIpol,
         cls.Do_subpixelEnhancement, cls.SE_FLOAT) = saved


def test_parameters_reach_the_stages(pair):
    """Parameters.DISP_PKR and bgIplDepth are read when the object is constructed."""
    cls = StereoMatching
    saved = (cls.costcalculation, cls.aggregation, cls.optimization, cls.Do_refine, cls.Do_calPKR, cls.Do_bgIpol,
             cls.Do_regionVote, cls.Do_properIpol, cls.Do_lastMedianBlur)
    try:
        cls.costcalculation, cls.aggregation, cls.optimization, cls.Do_refine = "censusGrad", "CBCA", "sgm", True
        cls.Do_calPKR, cls.Do_bgIpol = True, True
        cls.Do_regionVote = cls.Do_properIpol = cls.Do_lastMedianBlur = False
        prm = StereoMatching.Parameters(MD, H, W)
        prm.DISP_PKR, prm.bgIplDepth = -80, 0
        sm = StereoMatching(pair["lbgr"], pair["rbgr"], pair["lgray"], pair["rgray"], None, None, None, None, prm)
        sm.costCalculate()
        SolveAll([sm], 1, 0.3)
        sm.dispOptimize()
        dp = sm.refine()
        assert (dp == -80).any() and not (dp == -64).any()
        assert ((dp == -80) <= (sm.PKR_Err_Mask > 0)).all()   # depth 0 filled nothing: every mark is still there
    finally:
        (cls.costcalculation, cls.aggregation, cls.optimization, cls.Do_refine, cls.Do_calPKR, cls.Do_bgIpol,
         cls.Do_regionVote, cls.Do_properIpol, cls.Do_lastMedianBlur) = saved
