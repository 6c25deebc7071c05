"""Writes tests/golden/vmtop/vmtop_*.npz (a directory of their own: tests/test_gpu_parity.py takes every
tests/golden/*.npz for a pipeline fixture): crafted volumes for dispOptimize's Do_vmTop branch with the tables, maps and
branch counters of the restatement tests/pyref_vmtop.py.

    python tests/golden/make_vmtop.py

Every fixture holds vol [H][W][D] f32, bgr [H][W][3] u8 (the left colour image), num, thres, ts, the expected
table and counts, one expected map per decision setting (`map_<method><has_cir2><color_limit>`) and that
setting's counters (`cnt_...`, in pyref_vmtop.COUNTERS order).  Costs are integer-valued (or multiples of 1/2) so
that equal cost keys, the container's dedup, are common; nothing here is left to chance: the counts each fixture
set must reach are asserted below and again in tests/test_vmtop_host.py.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "vmtop")
sys.path.insert(0, os.path.dirname(HERE))
import pyref_vmtop as V  # noqa: E402

f32 = np.float32
SETTINGS = [(0, 1, 0), (0, 0, 0), (0, 1, 1), (0, 0, 1), (1, 1, 0), (2, 1, 0)]   # method, has_cir2, color_limit


def image(rng, H, W):
    """Patches of close colours with jumps between them, so judgeColorDif(.., 10, 3) goes both ways and the
    colour steps of method 2 differ."""
    base = rng.integers(40, 200, (H // 4 + 1, W // 5 + 1, 3))
    img = np.kron(base, np.ones((4, 5, 1), np.int64))[:H, :W]
    return (img + rng.integers(0, 9, (H, W, 3))).astype(np.uint8)


def vol_mix(rng, H, W, D):
    """Integer costs in a narrow range: ties, near and far candidate pairs in one volume."""
    return rng.integers(6, 14, (H, W, D)).astype(f32)


def vol_case2(rng, H, W, D):
    """Two candidates per pixel at least ts = 10 apart (an empty container): every pixel off row 0 and
    column 0 is case 2, one dependency chain through the whole map."""
    vol = np.full((H, W, D), 100, f32)
    a = rng.integers(0, 8, (H, W))
    b = a + 11 + rng.integers(0, D - 19, (H, W))
    vv, uu = np.mgrid[0:H, 0:W]
    vol[vv, uu, a] = 10 + 0.5 * rng.integers(0, 2, (H, W))
    vol[vv, uu, b] = 10 + 0.5 * rng.integers(0, 2, (H, W))
    return vol


def vol_rows(rng, H, W, D):
    """A slowly varying surface with a second, sometimes distant minimum: methods 1 and 2 find a candidate next
    to the previous output, next to the following pixel's first candidate, next to both, or next to neither."""
    vol = rng.integers(30, 60, (H, W, D)).astype(f32)
    surf = np.clip((D / 2 + np.cumsum(rng.integers(-1, 2, (H, W)), axis=1)), 1, D - 2).astype(np.int64)
    jump = rng.random((H, W)) < 0.25
    surf = np.where(jump, rng.integers(0, D, (H, W)), surf)
    vv, uu = np.mgrid[0:H, 0:W]
    vol[vv, uu, surf] = 10
    other = np.clip(surf + rng.integers(-6, 7, (H, W)), 0, D - 1)
    vol[vv, uu, other] = np.minimum(vol[vv, uu, other], 10 + rng.integers(0, 2, (H, W)))
    return vol


def vol_signed(rng, H, W, D):
    """Multiples of 1/2 of both signs (the guided filter's costs can be negative); thres < 1 keeps several."""
    return (rng.integers(-12, 12, (H, W, D)) * 0.5).astype(f32)


FIXTURES = [
    # name, maker, H, W, D, num, thres, ts
    ("mix", vol_mix, 20, 28, 16, 4, 1.5, 4),
    ("mix_m8", vol_mix, 12, 17, 10, 8, 1.26, 3),
    ("case2", vol_case2, 33, 41, 32, 2, 1.09, 10),
    ("rows", vol_rows, 14, 40, 20, 3, 1.15, 10),
    ("signed", vol_signed, 9, 13, 60, 6, 0.75, 12),
]


def build(name, maker, H, W, D, num, thres, ts, seed):
    rng = np.random.default_rng(seed)
    vol = maker(rng, H, W, D)
    bgr = image(rng, H, W)
    table, counts = V.select(vol, num, f32(thres))
    out = dict(vol=vol, bgr=bgr, num=np.int32(num), thres=f32(thres), ts=np.int32(ts), table=table, counts=counts)
    total = {k: 0 for k in V.COUNTERS}
    for m, cir2, col in SETTINGS:
        disp, cnt = V.decide(table, counts, bgr, m, ts, cir2, col)
        out[f"map_{m}{cir2}{col}"] = disp
        out[f"cnt_{m}{cir2}{col}"] = np.array([cnt[k] for k in V.COUNTERS], np.int64)
        for k in V.COUNTERS:
            total[k] += cnt[k]
    return out, total


def main():
    grand = {k: 0 for k in V.COUNTERS}
    size = 0
    os.makedirs(OUT, exist_ok=True)
    for seed, fx in enumerate(FIXTURES):
        out, total = build(*fx, seed=9100 + seed)
        path = os.path.join(OUT, f"vmtop_{fx[0]}.npz")
        np.savez_compressed(path, **out)
        size += os.path.getsize(path)
        print(fx[0], {k: v for k, v in total.items() if v})
        for k in V.COUNTERS:
            grand[k] += total[k]
        if fx[0] == "case2":   # every pixel off the first row and column
            H, W = fx[2], fx[3]
            assert int(out["cnt_010"][V.COUNTERS.index("case2")]) == (H - 1) * (W - 1)
    need = ("case1", "case2", "case3", "case3_tie_by_cost", "dedup", "m1_fallback", "m2_pre", "m2_aft", "m2_none", "m2_both")
    assert all(grand[k] >= 20 for k in need), grand
    assert size < 200 * 1024, size
    print("total bytes", size)


if __name__ == "__main__":
    main()
