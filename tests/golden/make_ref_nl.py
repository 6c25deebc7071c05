"""Writes tests/golden/ref_nl.npz and tests/golden/ref_nl_gpu.npz: recorded outputs of the reference's
own NL/ code (oracle/_ref/ref_nl_driver, built by oracle/ref_nl.mk beside a reference checkout), so
that a clone without the binary still compares with something that is not a restatement.

    python tests/golden/make_ref_nl.py

ref_nl.npz (the oracle's cases, tests/test_ref_nl.py).  Per case i: c{i}_bgr, c{i}_vol, c{i}_sigma,
c{i}_sha256 (of bgr, vol, sigma), and the binary's c{i}_median, c{i}_parent / nchild / child / weight /
order / rank, c{i}_filter (aggreCV of vol) and c{i}_filter_ones (aggreCV of a volume of ones, one plane).

ref_nl_gpu.npz (the kernels' cases, tests/test_gpu_ref_nl.py; ref_nl_cases.gpu_cases()).  Per key:
in_{key}, the sha256 of the raw costs, guide image and sigma; sha_{key}, the sha256 of the bits of NL()
of the reference build (oracle/ref_nl.nl); vol_{key}, that volume itself where it is small."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import ref_nl_cases as K  # noqa: E402
from oracle import ref_nl as R  # noqa: E402

# (family, H, W, P, sigma): 24 x 30 with P = 8 and two thin shapes
CASES = (("make_pair", 24, 30, 8, 0.1), ("levels4", 3, 90, 4, 0.5), ("stripes", 130, 5, 4, 0.005))
OUT = os.path.join(HERE, "ref_nl.npz")
OUT_GPU = os.path.join(HERE, "ref_nl_gpu.npz")


def record():
    d = {"n_cases": np.int32(len(CASES))}
    for i, (fam, H, W, P, sigma) in enumerate(CASES):
        bgr, vol, sg = K.image(fam, H, W, seed=5), K.volume(H, W, P, seed=5), np.float64(sigma)
        d.update({f"c{i}_bgr": bgr, f"c{i}_vol": vol, f"c{i}_sigma": sg,
                  f"c{i}_sha256": np.array(K.sha256(bgr, vol, sg)),
                  f"c{i}_median": R.median(bgr), f"c{i}_filter": R.filter(vol, bgr, sigma),
                  f"c{i}_filter_ones": R.filter(np.ones((H, W, 1), np.float32), bgr, sigma)})
        d.update({f"c{i}_{k}": v for k, v in R.tree(bgr).items()})
    return d


def record_gpu():
    d = {}
    for key, (raw, bgr, sigma) in K.gpu_cases().items():
        vol = R.nl(raw, bgr, sigma)
        d[f"in_{key}"] = np.array(K.input_digest(raw, bgr, sigma))
        d[f"sha_{key}"] = np.array(K.sha256(K.bits(vol)))
        if vol.nbytes <= K.FULL_VOLUME_BYTES:
            d[f"vol_{key}"] = vol
        if key == "both_view1_if_filtered":   # the share of vm[1] a (wrong) filtering of the right view would change
            d["frac_both_view1_changed"] = np.float64((K.bits(vol) != K.bits(raw)).mean())
    return d


if __name__ == "__main__":
    for path, rec in ((OUT, record()), (OUT_GPU, record_gpu())):
        np.savez_compressed(path, **rec)
        print(path, os.path.getsize(path), "bytes")
