"""Records outputs of oracle/_ref/ref_core_driver (the reference's own functions, oracle/ref_core.mk):

  ref_core.npz      every stage of three small pipelines, arrays in full: what tests/test_ref_core.py compares the
                    oracle with on machines without the binary;
  ref_core_gpu.npz  what tests/test_gpu_ref_core.py expects (tests/ref_core_cases.gpu_keys()): per case the
                    sha256 of its inputs, per expected array the sha256 of its bits and, up to K.SMALL bytes, the
                    array itself.

Every run goes through ref_core.run_defined: each case runs with two fill bytes for the build's new buffers and
is recorded only if both runs agree (so_T2D at W > 1: fill 0 only).  Run from the repository
root beside a reference checkout, after build():  python tests/golden/make_ref_core.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import ref_core_cases as K  # noqa: E402
import so_float_cases as SC  # noqa: E402
from oracle import ref_core as R  # noqa: E402

OUT = os.path.join(HERE, "ref_core.npz")
OUT_GPU = os.path.join(HERE, "ref_core_gpu.npz")


def record():
    out = {"n_cases": np.int32(len(K.GOLDEN_CASES))}
    for i, (kind, H, W, D) in enumerate(K.GOLDEN_CASES):
        p = K.pair(kind, H, W, D)
        c, c8 = K.chain(kind, H, W, D), K.chain(kind, H, W, D, paths=8)
        g = {"in_sha256": np.str_(K.sha256(*(p[k] for k in R.KEYS)))}
        for view in (0, 1):
            for name in ("census", "arms", "cost", "agg", "scaled", "sgm", "disp"):
                g[f"{name}{view}"] = c[name][view]
            g[f"census_cost{view}"] = K.chain(kind, H, W, D, cost="Census")["cost"][view]
            g[f"agg_ni{view}"] = K.chain(kind, H, W, D, intersect=False)["agg"][view]
            g[f"sgm8_{view}"] = c8["sgm"][view]
        for variant in K.VARIANTS:
            dp, acc = K.so_chain(kind, H, W, D, variant)[0]
            g[f"{variant}_disp"], g[f"{variant}_acc"] = dp, acc
            crafted = SC.craft(c["scaled"][0], 17 + i, lines="cols" if variant == "so_T2D" else "rows")
            dp, acc = R.so(crafted, p["lbgr"], variant)
            g[f"{variant}_crafted"], g[f"{variant}_crafted_disp"], g[f"{variant}_crafted_acc"] = crafted, dp, acc
        out.update({f"c{i}_{k}": v for k, v in g.items()})
    return out


def record_gpu():
    out = {}
    for key, spec in K.gpu_keys().items():
        arrays = K.gpu_expected(spec)
        out[f"in_{key}"] = np.str_(K.gpu_input_digest(spec))
        out[f"names_{key}"] = np.str_(",".join(arrays))
        for name, a in arrays.items():
            out[f"sha_{key}_{name}"] = np.str_(K.sha256(a))
            if a.nbytes <= K.SMALL:
                out[f"arr_{key}_{name}"] = a
    return out


if __name__ == "__main__":
    for fn, path in ((record, OUT), (record_gpu, OUT_GPU)):
        np.savez_compressed(path, **fn())
        print(f"wrote {path}: {os.path.getsize(path)} bytes")
