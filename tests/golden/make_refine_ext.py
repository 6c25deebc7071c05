"""Writes tests/golden/refine_ext/refine_ext_small.npz (a directory of its own: tests/test_gpu_parity.py takes every
tests/golden/*.npz for a pipeline fixture): one 40 x 60 pair, D = 16, censusGrad + CBCA + SolveAll(0.3) + sgm with
Do_refine and refine()'s three extra stages on, from the C oracle's maps and path sum and the restatement
tests/pyref_refine_ext.py.

    python tests/golden/make_refine_ext.py

The file holds lbgr, rbgr, lgray, rgray, the PKR mask, the refined map, both SE forms (se_reference, se_float) and
the synthetic pair's index.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "refine_ext")
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import pyref_refine_ext as R  # noqa: E402

H, W, D, INDEX = 40, 60, 16, 620
KEYS = ("lbgr", "rbgr", "lgray", "rgray")


def build():
    from mystereomatching_amd import synthetic as S
    from oracle import oracle as O
    pair = S.make_pair(H, W, D, INDEX)
    cfg = O.config(H, W, D - 1, do_refine=1)
    ref = O.run_ex(pair, cfg, dumps=("final", "disp_raw", "disp_right"))
    arms = O.arms(pair["lbgr"], cfg)
    out = {k: pair[k] for k in KEYS}
    for name, mode in (("se_reference", R.SE_REFERENCE), ("se_float", R.SE_FLOAT)):
        r = R.refine_ext(O, cfg, ref["disp_raw"], ref["disp_right"], arms, pair["lbgr"], ref["final"], do_pkr=True,
                         do_bg=True, do_se=True, mode=mode)
        out[name] = r["se"]
    out.update(mask=r["mask"], disp=r["disp"], index=np.int32(INDEX))
    return out


if __name__ == "__main__":
    d = build()
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, "refine_ext_small.npz")
    np.savez_compressed(path, **d)
    print(f"refine_ext_small: marked {float(d['mask'].mean()):.4f}, holes left {int((d['disp'] < 0).sum())}, "
          f"{os.path.getsize(path)} bytes")
