"""Host logic of tools/bench_cbca_ni.py: which kernels count as the aggregation, the share of the step, and the
`_ni` kernels' bytes per element and share of the copy ceiling picked out of a profile."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bench_cbca_ni as B  # noqa: E402


def k(ms, n=1.0, b=0.0):
    return {"ms_per_launch": ms, "launches_per_step": n, "bytes_per_launch": b}


def test_is_cbca():
    for n in ("cbca_h_scan_cost", "cbca_v_norm_scan", "cbca_h_prefix_ni", "cbca_v_window_norm_r_ni", "cost_volume",
              "cost_volume_right"):
        assert B.is_cbca(n), n
    for n in ("prep", "sgm_ck_a", "solve_all_scale", "dw_select", "refine_median3"):
        assert not B.is_cbca(n), n


def test_cbca_share():
    kern = {"prep": k(0.3), "cost_volume": k(0.1), "cbca_h_prefix_ni": k(0.2, 2.0), "cbca_h_window_ni": k(0.1),
            "sgm_ck_a": k(0.4)}
    agg, total, share = B.cbca_share(kern)
    assert agg == round(0.1 + 0.4 + 0.1, 4) and total == round(0.3 + 0.1 + 0.4 + 0.1 + 0.4, 4)
    assert share == round(agg / total, 4)
    assert B.cbca_share({}) == (0, 0, None)


def test_summarise_ni():
    elements = 1_000_000.0
    kern = {"cbca_h_prefix_ni": k(0.002, 2.0, 8.0 * elements), "cbca_v_window_norm_ni": k(0.004, 1.0, 8.0 * elements),
            "cbca_h_norm": k(0.4, 1.0, 8.0 * elements), "prep": k(0.3)}
    s = B.summarise_ni(kern, elements, 4000.0)
    assert set(s) == {"cbca_h_prefix_ni", "cbca_v_window_norm_ni"}
    assert s["cbca_h_prefix_ni"]["bytes_per_element"] == B.NI_BYTES_PER_ELEMENT == 8.0
    assert s["cbca_h_prefix_ni"]["gbs"] == 4000.0 and s["cbca_h_prefix_ni"]["frac_of_copy_ceiling"] == 1.0
    assert s["cbca_v_window_norm_ni"]["gbs"] == 2000.0 and s["cbca_v_window_norm_ni"]["frac_of_copy_ceiling"] == 0.5
    assert s["cbca_h_prefix_ni"]["launches_per_step"] == 2.0
    # a kernel that took no measurable time: no division
    z = B.summarise_ni({"cbca_h_prefix_ni": k(0.0, 1.0, 8.0)}, 1.0, 0.0)
    assert "gbs" not in z["cbca_h_prefix_ni"]


def test_arguments():
    a = B.parse(["--steps", "5", "--warmup", "2"])
    assert (a.steps, a.warmup, a.batch, a.rows, a.cols, a.max_disp) == (5, 2, 16, 375, 450, 63)
