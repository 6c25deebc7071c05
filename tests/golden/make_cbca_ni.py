"""Writes tests/golden/cbca_ni/*.npz: inputs, aggregated volumes and areas of cross-based aggregation without arm
intersection (Parameters::cbca_intersect == false), from the restatement tests/pyref_cbca_ni.py (the C oracle's
cost volumes and arms, the aggregation in numpy).

    python tests/golden/make_cbca_ni.py

cbca_ni_main.npz   pyref_cbca_dw.make_input(40, 56, 16, 0): long arms on the left two thirds, short ones on the
                   right.  vm0, vm1, area0, area1 for two iterations; vm0_n1, vm0_n3 for one and three.
cbca_ni_odd.npz    make_input(23, 37, 13, 0): neither D nor W * D is a multiple of 4.  vm0, vm1, area0, area1.

Each file also holds lbgr, rbgr, lgray, rgray and index.  The conditions a fixture must meet are asserted here and
again in tests/test_cbca_ni_host.py.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "cbca_ni")
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import pyref_cbca_ni as P  # noqa: E402


def conditions(r: dict) -> list:
    """The list of unmet conditions (empty: the fixture exercises both branches of cal1DCost in both passes)."""
    bad = []
    for name in ("armsL", "armsR"):
        for inner, axis in zip(P.inner_masks(r[name]), "HV"):
            if inner.all() or not inner.any():
                bad.append(f"{name}: `inner` of the {axis} pass is constant")
    if not (r["area0"] != r["area1"]).any():
        bad.append("the two views' areas are equal")
    return bad


def save(name, H, W, D, index=0, more=False):
    pair = P.make_input(H, W, D, index)
    r = P.aggregate(pair, D, 2)
    assert conditions(r) == [], conditions(r)
    d = {k: pair[k] for k in ("lbgr", "rbgr", "lgray", "rgray")}
    d.update({k: r[k] for k in ("vm0", "vm1", "area0", "area1")}, index=np.int32(index))
    if more:
        d["vm0_n1"] = P.aggregate(pair, D, 1, refine=False)["vm0"]
        d["vm0_n3"] = P.aggregate(pair, D, 3, refine=False)["vm0"]
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **d)
    print(f"{name}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    save("cbca_ni_main", 40, 56, 16, more=True)
    save("cbca_ni_odd", 23, 37, 13)
