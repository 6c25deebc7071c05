"""The C++ facade's static SO_VARIANT (include/stereo_matching.hpp) through tests/cpp/so_variants_facade_check.cpp: it
compiles against the facade and the library without a GPU; on the GPU its maps of both views equal the Python
facade's and the restatement's (tests/pyref_so.py)."""
import os
import subprocess

import numpy as np
import pytest

from test_cpp_facade import _compile, write_ppm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "so_variants_facade_check.cpp")


def test_so_variants_facade_check_compiles(tmp_path):
    _compile(SRC, str(tmp_path / "so_variants_facade_check"))
    text = open(SRC).read()
    assert "StereoMatching::SO_VARIANT = atoi(argv[4]);" in text


@pytest.mark.gpu
def test_cpp_static_selects_the_variant(tmp_path):
    import pyref_so as P
    from mystereomatching_amd import synthetic as S
    from test_gpu_so_variants import PYREF, staged
    H, W, D = 30, 52, 16
    p = S.make_pair(H, W, D, 730)
    exe = str(tmp_path / "so_variants_facade_check")
    _compile(SRC, exe)
    # (the C++ facade reads its gray images from the colour files; the synthetic pair's are that conversion)
    write_ppm(tmp_path / "l.ppm", p["lbgr"])
    write_ppm(tmp_path / "r.ppm", p["rbgr"])
    vol = staged(p, H, W, D, "so")["vol"]
    maps = {}
    for code, name in enumerate(("so", "so_R2L", "so_T2D")):
        d0, d1 = tmp_path / f"d0_{code}", tmp_path / f"d1_{code}"
        r = subprocess.run([exe, str(tmp_path / "l.ppm"), str(tmp_path / "r.ppm"), str(D - 1), str(code), str(d0), str(d1)],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert f"SO_VARIANT {code}" in r.stdout
        for view, path in enumerate((d0, d1)):
            got = np.fromfile(path, np.int16).reshape(H, W)
            np.testing.assert_array_equal(got, PYREF[name](vol[view], p["lbgr"])[0], err_msg=f"{name} view {view}")
        maps[name] = np.fromfile(d0, np.int16)
    assert (maps["so_R2L"] != maps["so"]).any() and (maps["so_T2D"] != maps["so"]).any()
    assert P.R2L_PN == P.T2D_PN
