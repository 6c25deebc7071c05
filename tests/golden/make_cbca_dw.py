"""Writes tests/golden/cbca_dw/*.npz (a directory of their own: tests/test_gpu_parity.py takes every
tests/golden/*.npz for a pipeline fixture): inputs, arm_Mask and composed volumes of CBCA()'s double-window
branch, from the restatement tests/pyref_cbca_dw.py (the C oracle's cost volume, its cbca_core once per window,
its window-0 left arms and pyref_box.box_filter).

    python tests/golden/make_cbca_dw.py

cbca_dw_main.npz   40 x 56 x 16, both views (Do_refine): synthetic pair `index`, the left two thirds of its columns
                   softened (pyref_cbca_dw.soften) so that long and short arms both occur.  The raw texture alone
                   selects every pixel.  The index is the first one from 0 that meets every condition below.
cbca_dw_odd.npz    23 x 37 x 13, view 0: neither D nor W * D is a multiple of 4 (the selection's scalar pieces).

Each file holds lbgr, rbgr, lgray, rgray, mask, arms (window 0, left image), vm0 (and vm1) composed, and index.
The conditions a fixture must meet are asserted here and again in tests/test_cbca_dw_host.py.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "cbca_dw")
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import pyref_cbca_dw as P  # noqa: E402


def conditions(r: dict, need_edge_sums: bool = True) -> list:
    """The list of unmet conditions (empty: the fixture exercises the branch)."""
    bad = []
    share = float(r["mask"].mean())
    if not 0.2 <= share <= 0.8:
        bad.append(f"selected share {share:.3f} outside [0.2, 0.8]")
    s = P.nine_sum(P.arm_max(r["arms"]))
    if need_edge_sums and not ((s == 44).any() and (s == 45).any()):
        bad.append("no pixel at sum 44 or none at sum 45")
    if not ((r["vm0"] != r["small0"]).any() and (r["vm0"] != r["large0"]).any()):
        bad.append("the composed volume equals a single-window volume")
    if not (P.wta(r["vm0"]) != P.wta(r["small0"])).any():
        bad.append("the composed volume's WTA map equals the single-window one")
    return bad


def build(H, W, D, refine, first_index=0, need_edge_sums=True):
    for index in range(first_index, first_index + 32):
        pair = P.make_input(H, W, D, index)
        r = P.compose(pair, D, refine=refine)
        if not conditions(r, need_edge_sums):
            return index, pair, r
    raise SystemExit("no index in range meets the conditions")


def save(name, index, pair, r, refine):
    os.makedirs(OUT, exist_ok=True)
    d = {k: pair[k] for k in ("lbgr", "rbgr", "lgray", "rgray")}
    d.update(mask=r["mask"], arms=r["arms"].astype(np.uint16), vm0=r["vm0"], index=np.int32(index))
    if refine:
        d["vm1"] = r["vm1"]
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **d)
    print(f"{name}: index {index}, selected {float(r['mask'].mean()):.4f}, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    i, pair, r = build(40, 56, 16, True)
    save("cbca_dw_main", i, pair, r, True)
    i, pair, r = build(23, 37, 13, False, need_edge_sums=False)
    save("cbca_dw_odd", i, pair, r, False)
