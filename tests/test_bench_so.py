"""Host logic of tools/bench_so.py: its arguments, which profile names belong to which variant, and the shape of
the per-variant summary (GB/s and the share of the copy ceiling) picked out of a profile."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bench_so as B  # noqa: E402


def k(ms, n=1.0, b=0.0):
    return {"ms_per_launch": ms, "launches_per_step": n, "bytes_per_launch": b}


def test_arguments():
    a = B.parse(["--steps", "5", "--warmup", "2"])
    assert (a.steps, a.warmup, a.batch, a.rows, a.cols, a.max_disp, a.out) == (5, 2, 16, 375, 450, 63, None)
    a = B.parse([])
    assert (a.steps, a.warmup) == (20, 3)
    assert B.parse(["--out", "x.json", "--batch", "4"]).out == "x.json"
    for bad in (["--steps", "0"], ["--warmup", "-1"], ["--variant", "so"]):
        with pytest.raises(SystemExit):
            B.parse(bad)


def test_kernel_names():
    assert B.VARIANTS == ("so", "so_R2L", "so_T2D")
    assert B.is_so_kernel("so", "so") and B.is_so_kernel("so_r", "so")
    assert B.is_so_kernel("so_r2l", "so_R2L") and B.is_so_kernel("so_r2l_r", "so_R2L")
    assert B.is_so_kernel("so_t2d", "so_T2D") and B.is_so_kernel("so_t2d_r", "so_T2D")
    for name, v in (("so_r2l", "so"), ("so_t2d_r", "so"), ("so", "so_R2L"), ("so_r", "so_T2D"), ("solve_all_scale", "so"),
                    ("cbca_h_norm", "so_T2D")):
        assert not B.is_so_kernel(name, v), (name, v)


def test_summary_shape():
    kern = {"so_t2d": k(0.5, 1.0, 2.0e9), "so_t2d_r": k(0.25, 1.0, 2.0e9), "cbca_h_norm": k(0.4, 1.0, 8.0e9), "so": k(9.0)}
    s = B.summarise(kern, "so_T2D", 8000.0)
    assert set(s) == {"kernels", "ms_per_step"} and set(s["kernels"]) == {"so_t2d", "so_t2d_r"}
    assert s["ms_per_step"] == 0.75
    assert s["kernels"]["so_t2d"]["gbs"] == 4000.0 and s["kernels"]["so_t2d"]["frac_of_copy_ceiling"] == 0.5
    assert s["kernels"]["so_t2d_r"]["gbs"] == 8000.0 and s["kernels"]["so_t2d_r"]["frac_of_copy_ceiling"] == 1.0
    z = B.summarise({"so": k(0.0, 2.0, 8.0)}, "so", 0.0)          # no measurable time: no division
    assert "gbs" not in z["kernels"]["so"] and z["ms_per_step"] == 0
    summary = {"so": {"ms_per_step": 0.5}, "so_R2L": {"ms_per_step": 0.5}, "so_T2D": {"ms_per_step": 0.75}}
    assert B.ratios(summary) == {"so_R2L": 1.0, "so_T2D": 1.5}
    summary["so"]["ms_per_step"] = 0
    assert B.ratios(summary) == {"so_R2L": None, "so_T2D": None}
    json.dumps(s)
