"""Crafted volumes for the float-minima scan-line optimisers (so_float_minima): signed costs, the two zeros and NaN.

craft() starts from a CBCA volume of a synthetic.make_pair pair (every cost >= +0), subtracts its median, so that about
half of the entries are negative, and then sets, deterministically from the seed:
  * at about 2 % of the pixels, and on every line at the scan's two end columns, two equal minima of the
    pixel's costs, one -0.0 and one +0.0, in both orders (the pixel's costs are first shifted so that its minimum is
    0).  The end columns matter: a raw zero is compared as it stands only where a scan starts (an accumulated cost is
    a sum, and x + -0 == x), so that is where an ordering with -0 < +0 shows; there the pixel's other costs are also
    raised by 8, above Pn3, so that the next step's choice is the jump to the minimum's index;
  * NaN at d = 0 at about 1 % of the pixels (the loop's sticky NaN);
  * NaN at a random d > 0 at about 2 % (never wins);
  * every cost NaN at about 0.5 % (the line is NaN from there on);
  * one whole line NaN.
A line is a row (so, so_R2L) or, with lines="cols", a column (so_T2D): the construction is then made on the
transposed volume.

wrong_maps() gives, from the restatement alone, what three wrong minima would return; the tests assert on every
sizeable shape that the right map differs from each (conditions (a), (b), (c) in test_so_float_host.py).
"""
import numpy as np

import pyref_so_float as PF

F = np.float32


def sizeable(steps, lines, D):
    return steps >= 16 and lines >= 12 and D >= 10


def craft(vol, seed, lines="rows"):
    if lines == "cols":
        return np.ascontiguousarray(craft(np.asarray(vol).transpose(1, 0, 2), seed).transpose(1, 0, 2))
    v = np.array(vol, F, copy=True)
    L, S, D = v.shape                       # lines, steps along a line, disparities
    rng = np.random.default_rng(seed)
    v -= F(np.median(v))
    u = rng.random((L, S))
    if D >= 2:
        zero = u < 0.02
        zero[:, 0] = True                   # where the scans start (so: step 0; so_R2L: step S - 1)
        zero[:, S - 1] = True
        for k, (l, s) in enumerate(zip(*np.nonzero(zero))):
            c = v[l, s]
            c -= c.min()
            if s == 0 or s == S - 1:
                c += F(8)                   # every other cost above Pn3: the next step jumps to the minimum's index (code 3)
            i, j = sorted(rng.choice(D, 2, replace=False))
            c[i], c[j] = (F(-0.0), F(0.0)) if k % 2 else (F(0.0), F(-0.0))
        later = (u >= 0.03) & (u < 0.05)
        for l, s in zip(*np.nonzero(later)):
            v[l, s, rng.integers(1, D)] = np.nan
    v[(u >= 0.02) & (u < 0.03), 0] = np.nan
    v[(u >= 0.05) & (u < 0.055)] = np.nan
    if L >= 3:
        v[L // 2] = np.nan
    return v


FUNCS = {"so": PF.so, "so_R2L": PF.so_r2l, "so_T2D": PF.so_t2d}
WRONG = {"unsigned": PF.first_min_unsigned, "nan_dropping": PF.first_min_nan_dropping, "signed_zero": PF.first_min_signed_zero}


def wrong_maps(variant, vol, img):
    """{name: the fraction of pixels at which the right map differs from the map a wrong minimum gives}."""
    right = FUNCS[variant](vol, img)[0]
    return {k: float((FUNCS[variant](vol, img, first_min=fm)[0] != right).mean()) for k, fm in WRONG.items()}


def assert_not_vacuous(variant, vol, img):
    """(a) > 5 % of the pixels against minima on unsigned bit patterns (the kernels for costs >= +0); (b) >= 1 pixel
    against NaN-dropping minima (v_min_f32); (c) >= 1 pixel against -0 < +0."""
    w = wrong_maps(variant, vol, img)
    assert w["unsigned"] > 0.05, w
    assert w["nan_dropping"] > 0, w
    assert w["signed_zero"] > 0, w
    return w
