"""Host logic of tools/bench_cbca_dw.py: its input softening and host mask are the tests' (pyref_cbca_dw), the
selection's byte count is 8 B per selected element plus 1 B per pixel, and the summary picks the double window's
kernels out of a profile."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bench_cbca_dw as B  # noqa: E402
import pyref_cbca_dw as P  # noqa: E402
from mystereomatching_amd import synthetic as S  # noqa: E402


def test_input_and_mask_are_the_fixture_recipe():
    pair = S.make_pair(40, 56, 16, 0)
    want = P.soften(pair)
    np.testing.assert_array_equal(B.soften(pair["lbgr"]), want["lbgr"])
    np.testing.assert_array_equal(B.soften(pair["rbgr"]), want["rbgr"])
    fx = np.load(os.path.join(ROOT, "tests", "golden", "cbca_dw", "cbca_dw_main.npz"))
    np.testing.assert_array_equal(B.mask_from_arms(fx["arms"]), fx["mask"])
    assert B.WINDOW1 == (23, 23, 30, 0, 5.0)


def test_select_bytes():
    assert B.select_bytes(0, 1000, 64) == 1000
    assert B.select_bytes(10, 1000, 64) == 8 * 10 * 64 + 1000
    assert B.select_bytes(10, 1000, 64, views=2) == 2 * (8 * 10 * 64 + 1000)


def test_summarise():
    k = lambda ms, n=1.0: {"ms_per_launch": ms, "launches_per_step": n, "bytes_per_launch": 0.0}
    kern = {"cbca_h_scan_cost": k(0.3), "cbca_v_norm_scan": k(0.7), "cbca_h_norm": k(0.4),
            "cbca_h_scan_cost_dw": k(0.31), "cbca_v_norm_scan_dw": k(0.8), "cbca_h_norm_dw": k(0.45), "prep_dw": k(0.1),
            "dw_mask": k(0.01), "dw_select": k(0.05), "sgm_last_wta": k(0.5)}
    s = B.summarise(kern, 2_000_000_000 // 10, 4000.0)
    assert s["dw_mask_ms"] == 0.01 and s["dw_select_ms"] == 0.05
    assert s["second_run_ms"] == round(0.31 + 0.8 + 0.45 + 0.1, 4) and s["first_run_ms"] == round(0.3 + 0.7 + 0.4, 4)
    assert set(s["second_run_kernels"]) == {"cbca_h_scan_cost_dw", "cbca_v_norm_scan_dw", "cbca_h_norm_dw", "prep_dw"}
    assert s["dw_select_gbs"] == 4000.0 and s["dw_select_frac_of_copy_ceiling"] == 1.0
    # the unfused path's raw-cost copy belongs to the second run
    kern["dw_copy_raw"] = k(0.2)
    assert B.summarise(kern, 1, 4000.0)["second_run_ms"] == round(0.31 + 0.8 + 0.45 + 0.1 + 0.2, 4)
    # no double-window kernels in the profile: nothing to report, no division
    assert B.summarise({"cbca_h_norm": k(0.4)}, 0, 0.0)["dw_select_ms"] is None


def test_arguments():
    a = B.parse(["--steps", "5", "--warmup", "2"])
    assert (a.steps, a.warmup, a.batch, a.rows, a.cols, a.max_disp) == (5, 2, 16, 375, 450, 63)
