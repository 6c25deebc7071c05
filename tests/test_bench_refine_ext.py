"""Host logic of tools/bench_refine_ext.py: its arguments, its list of configurations (every name maps onto
StereoBatch.refine_ext_config's keywords) and the per-kernel share of the copy ceiling."""
import inspect
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bench_refine_ext as B  # noqa: E402
from mystereomatching_amd import StereoBatch  # noqa: E402


def test_arguments():
    a = B.parse(["--steps", "5", "--warmup", "2"])
    assert (a.steps, a.warmup, a.batch, a.rows, a.cols, a.max_disp) == (5, 2, 16, 375, 450, 63)
    assert B.parse([]).steps == 20 and B.parse([]).warmup == 3


def test_configurations():
    names = [n for n, _ in B.CONFIGS]
    assert names[:5] == ["all_off", "pkr", "bg_ipol", "subpixel", "all_on"]
    accepted = set(inspect.signature(StereoBatch.refine_ext_config).parameters)
    for _, cfg in B.CONFIGS:
        assert set(cfg) <= accepted
    assert dict(B.CONFIGS)["all_off"] == {} and len(dict(B.CONFIGS)["all_on"]) == 3


def test_kernel_shares():
    k = lambda ms, by: {"ms_per_launch": ms, "launches_per_step": 1.0, "bytes_per_launch": by}
    kern = {"refine_pkr": k(0.5, 2e9), "vmtop_select": k(1.0, 2e9), "refine_bg_ipol": k(0.0, 10.0), "sgm_path1": k(0.4, 1e9)}
    s = B.kernel_shares(kern, 5000.0)
    assert set(s) == {"refine_pkr", "vmtop_select", "refine_bg_ipol"}
    assert s["refine_pkr"]["gbs"] == 4000.0 and s["refine_pkr"]["frac_of_copy_ceiling"] == 0.8
    assert s["vmtop_select"]["frac_of_copy_ceiling"] == 0.4
    assert s["refine_bg_ipol"]["gbs"] is None and s["refine_bg_ipol"]["frac_of_copy_ceiling"] is None   # no division by zero
    assert B.kernel_shares(kern, 0.0)["refine_pkr"]["frac_of_copy_ceiling"] is None
