"""The C++ facade (include/stereo_matching.hpp) with aggregation "AWS".

tests/cpp/aws_facade_check.cpp defines the static selectors with aggregation = "AWS", sets the
facade's aws_radius_v / aws_radius_u / aws_gamma_c, runs costCalculate -> SolveAll -> dispOptimize
on one pair and writes DP[0].  CPU: it compiles against the facade and the library.  GPU: its map
equals the Python path's for one 20 x 26 pair, at the defaults and with the identity window.
"""
import os
import subprocess

import numpy as np
import pytest

from test_cpp_facade import _compile, write_ppm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "aws_facade_check.cpp")


def test_aws_facade_check_compiles(tmp_path):
    _compile(SRC, str(tmp_path / "aws_facade_check"))


@pytest.mark.gpu
def test_aws_facade_matches_python_path(tmp_path):
    from mystereomatching_amd import StereoBatch
    from mystereomatching_amd import synthetic as S
    exe = str(tmp_path / "aws_facade_check")
    _compile(SRC, exe)
    H, W, md = 20, 26, 15
    pair = S.make_pair(H, W, md + 1, 870)
    pair = {k: (128 + (pair[k].astype(np.int32) - 128) // 16).astype(np.uint8) for k in ("lbgr", "rbgr")}
    # the facade reads the gray images from the colour files (imread flags 0: libpng's weights)
    pair["lgray"], pair["rgray"] = S.bgr_to_gray(pair["lbgr"]), S.bgr_to_gray(pair["rbgr"])
    write_ppm(tmp_path / "l.ppm", pair["lbgr"])
    write_ppm(tmp_path / "r.ppm", pair["rbgr"])
    maps = []
    for k, (rv, ru, gamma) in enumerate([(17, 17, 5.0), (0, 0, 1.5)]):
        out = tmp_path / f"dp{k}.i16"
        r = subprocess.run([exe, str(tmp_path / "l.ppm"), str(tmp_path / "r.ppm"), str(md), str(rv), str(ru), str(gamma),
                            str(out)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        got = np.fromfile(out, np.int16).reshape(H, W)
        sb = StereoBatch(md, H, W, 1, device=0, aggregation="AWS", num_streams=1,
                         aws_radius_v=rv, aws_radius_u=ru, aws_gamma_c=gamma)
        try:
            sb.upload(*(pair[k][None] for k in ("lbgr", "rbgr", "lgray", "rgray")))
            want = sb.run(0.3)[0]
        finally:
            sb.close()
        np.testing.assert_array_equal(got, want)
        maps.append(got)
    assert (maps[0] != maps[1]).any()   # the constants reached the kernels (raw against aggregated costs)
