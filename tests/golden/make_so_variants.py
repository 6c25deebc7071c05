"""Writes tests/golden/so_variants/so_variants.npz (a folder of its own: tests/test_gpu_parity.py reads every
tests/golden/*.npz as a pipeline fixture): the maps of so_R2L and so_T2D (tests/pyref_so.py), both views, on the two
synthetic pairs of tests/test_so_variants_host.py, with the volumes the C oracle computes (censusGrad + CBCA +
SolveAll).  Run from the repository root: python tests/golden/make_so_variants.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from oracle import oracle as O  # noqa: E402
from test_so_variants_host import GOLDEN, golden_outputs  # noqa: E402

if __name__ == "__main__":
    out = golden_outputs(O)
    np.savez_compressed(GOLDEN, **out)
    print(GOLDEN, {k: v.shape for k, v in out.items()}, os.path.getsize(GOLDEN), "bytes")
