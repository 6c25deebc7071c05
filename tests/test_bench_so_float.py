"""Host logic of tools/bench_so_float.py: its arguments, its jobs, and the ratio of the two so kernels over the
alternating rounds."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bench_so_float as B  # noqa: E402


def test_arguments():
    a = B.parse(["--steps", "5", "--warmup", "2"])
    assert (a.steps, a.warmup, a.rounds, a.batch, a.rows, a.cols, a.max_disp, a.out) == (5, 2, 3, 16, 375, 450, 63, None)
    a = B.parse([])
    assert (a.steps, a.warmup, a.rounds) == (20, 3, 3)
    assert B.parse(["--out", "x.json", "--rounds", "5"]).rounds == 5
    for bad in (["--steps", "0"], ["--warmup", "-1"], ["--rounds", "0"], ["--variant", "so"]):
        with pytest.raises(SystemExit):
            B.parse(bad)


def test_jobs():
    assert list(B.JOBS) == ["cbca_so", "cbca_so_fm", "gf_so", "gf_wta", "bf_grad_so", "cbca_so_pkr"]
    assert B.PAIR == ("cbca_so", "cbca_so_fm")
    assert B.JOBS["cbca_so"] == dict(optimization="so") and B.JOBS["cbca_so_fm"]["so_float_minima"] is True
    assert "so_float_minima" not in B.JOBS["gf_so"]            # the facade opts in by itself
    assert B.JOBS["gf_wta"]["optimization"] == "" and B.JOBS["bf_grad_so"]["cost_method"] == "grad"
    assert B.JOBS["cbca_so_pkr"]["refine_ext"] == dict(do_pkr=True) and B.JOBS["cbca_so_pkr"]["do_refine"] == 1
    json.dumps(B.JOBS)


def test_kernel_ratio():
    k = {"ms_per_launch": 0.5, "launches_per_step": 1.0, "bytes_per_launch": 1e9}
    s = B.summarise({"so": k, "so_r": dict(k, ms_per_launch=0.25), "cbca_h_norm": k}, "so", 4000.0)
    assert B.so_ms_per_launch(s) == 0.5 and s["ms_per_step"] == 0.75
    assert B.so_ms_per_launch(B.summarise({"wta": k}, "so", 4000.0)) is None
    r = B.kernel_ratio([(0.5, 0.55), (0.5, 0.5), (0.4, 0.6)])
    assert r == {"per_round": [1.1, 1.0, 1.5], "median": 1.1}
    assert B.kernel_ratio([(0.0, 0.5), (None, 0.5)]) == {"per_round": [], "median": None}
