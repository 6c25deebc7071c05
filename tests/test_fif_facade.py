"""The C++ facade (include/stereo_matching.hpp) with aggregation "FIF".

tests/cpp/fif_facade_check.cpp defines the static selectors with aggregation = "FIF", runs
costCalculate -> SolveAll -> dispOptimize on one pair and writes DP[0].  CPU: it compiles against
the facade and the library (as tests/test_cpp_facade.py compiles main_shaped.cpp).  GPU: its map
equals the Python path's for one 24 x 30 pair, for FIF_Improve and for the plain form.
"""
import os
import subprocess

import numpy as np
import pytest

from test_cpp_facade import _compile, write_ppm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "fif_facade_check.cpp")


def test_fif_facade_check_compiles(tmp_path):
    _compile(SRC, str(tmp_path / "fif_facade_check"))


@pytest.mark.gpu
def test_fif_facade_matches_python_path(tmp_path):
    from mystereomatching_amd import StereoBatch
    from mystereomatching_amd import synthetic as S
    exe = str(tmp_path / "fif_facade_check")
    _compile(SRC, exe)
    H, W, md = 24, 30, 15
    pair = S.make_pair(H, W, md + 1, 770)
    pair = {k: pair[k] // 32 * 32 for k in ("lbgr", "rbgr", "lgray", "rgray")}
    # the facade reads the gray images from the colour files (imread flags 0: libpng's weights)
    pair["lgray"], pair["rgray"] = S.bgr_to_gray(pair["lbgr"]), S.bgr_to_gray(pair["rbgr"])
    write_ppm(tmp_path / "l.ppm", pair["lbgr"])
    write_ppm(tmp_path / "r.ppm", pair["rbgr"])
    for plain in (0, 1):
        out = tmp_path / f"dp{plain}.i16"
        r = subprocess.run([exe, str(tmp_path / "l.ppm"), str(tmp_path / "r.ppm"), str(md), str(plain), str(out)],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        got = np.fromfile(out, np.int16).reshape(H, W)
        sb = StereoBatch(md, H, W, 1, device=0, aggregation="FIF", fif_mode=plain, num_streams=1)
        try:
            sb.upload(*(pair[k][None] for k in ("lbgr", "rbgr", "lgray", "rgray")))
            want = sb.run(0.3)[0]
        finally:
            sb.close()
        np.testing.assert_array_equal(got, want)
