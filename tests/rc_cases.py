"""Inputs and cases of the runtime-constant tests (a plain module shared by the host conditions in
test_degenerate_host.py and the GPU parity in test_gpu_runtime_constants.py).

Every case names one sm_params field (or SolveAll's lambda) at a value other than the default;
`oracle_kw` is the same setting in the oracle's field names.
"""
import numpy as np

from mystereomatching_amd import synthetic as S

KEYS = ("lbgr", "rbgr", "lgray", "rgray")
H, W, MD = 48, 70, 23
H2, W2, MD2 = 21, 30, 199            # SGM's checkpointed dwordx4 lanes
HT, WT, MDT = 67, 513, 15            # several prep tiles in both directions

# sm_params field -> oracle config field, where they differ
ORACLE_NAME = {"sgm_cor_dif_thres": "sgm_cor_thres", "sgm_redu_coeff": "sgm_redu", "arm_l_out": "arm_L_out"}


def oracle_kw(kw):
    return {ORACLE_NAME.get(k, k): v for k, v in kw.items()}


def _half_quantised(pair, q=64):
    """Top half quantised: flat regions with long arms and large vote regions next to texture."""
    h = pair["lbgr"].shape[0] // 2
    for k in ("lbgr", "rbgr"):
        pair[k][:h] = (pair[k][:h] // q * q).astype(np.uint8)
    pair["lgray"], pair["rgray"] = S.bgr_to_gray(pair["lbgr"]), S.bgr_to_gray(pair["rbgr"])
    return {k: pair[k] for k in KEYS}


def pair():
    return _half_quantised(S.make_pair(H, W, MD + 1, 700))


def pair_d200():
    p = S.make_pair(H2, W2, MD2 + 1, 701)
    return {k: p[k] for k in KEYS}


def pair_tiles():
    return _half_quantised(S.make_pair(HT, WT, MDT + 1, 70 + HT), 96)


FLAT_ROWS = 32     # vote_pair(): rows of flat colour
WHITE_COLS = 40    # of them, the columns that are white (the rest is grey 200)
SEED_COLS = 6      # given_maps(): the white columns that hold valid pixels
TEX_COLS = 25      # and the columns of the textured rows that do


def vote_pair():
    """pair() with the left image made so that the region vote and properIpol disagree.  The top
    FLAT_ROWS rows are flat: white in the first WHITE_COLS columns, grey 200 beyond.  Arms in the
    white part run to L_out = 34 and stop at the grey (a difference of 55 > cT = 20), so a hole's
    vote region is the white part only, while properIpol accepts any colour difference below 255
    and so reaches into the grey.  The textured rows below get a blue channel of 0: arms of a
    pixel or two, and a colour difference of 255 to the white rows, which properIpol rejects."""
    p = {k: v.copy() for k, v in pair().items()}
    p["lbgr"][:FLAT_ROWS, :WHITE_COLS] = 255
    p["lbgr"][:FLAT_ROWS, WHITE_COLS:] = 200
    p["lbgr"][FLAT_ROWS:, :, 0] = 0
    p["lgray"] = S.bgr_to_gray(p["lbgr"])
    return p


def given_maps(seed=80):
    """DP[0] / DP[1] for sm_set_disp on vote_pair(), made so that every refine constant decides
    something.  Flat rows: half of the first SEED_COLS white columns is valid with disparity 7,
    half of the grey part with disparity 3, the white columns between them are holes.  The holes
    more than 20 columns from the seeds see only 7s in their vote region (about 100 > rv_s = 20
    votes) but only 3s along properIpol's 20-step rays: the vote's fill and the interpolation's
    differ (rv_ratio > 1, rv_s = 10^6, region_vote_nums).  Textured rows: constant on 8 x 10
    blocks, 60 % valid in the first TEX_COLS columns and holes beyond; regions hold a few votes
    (rv_s 0 and 5) and properIpol crosses the 45 columns of holes in three passes, not two
    (region_vote_nums 1 and 5).  DP[1] is the LR-consistent partner (DP[1](u - d) = d) except
    that a quarter of the valid pixels is off by 1, 2 or 3 (lr_max_diff)."""
    rng = np.random.default_rng(seed)
    vv, uu = np.mgrid[0:H, 0:W]
    d0 = np.empty((H, W), np.int64)
    d0[:FLAT_ROWS, :WHITE_COLS] = 7
    d0[:FLAT_ROWS, WHITE_COLS:] = 3
    base = rng.integers(2, 12, size=((H - FLAT_ROWS) // 8 + 1, W // 10 + 1))
    d0[FLAT_ROWS:] = np.kron(base, np.ones((8, 10), np.int64))[:H - FLAT_ROWS, :W]
    flat = vv < FLAT_ROWS
    valid = rng.random((H, W)) < np.where(flat, 0.5, 0.6)
    valid &= np.where(flat, (uu < SEED_COLS) | (uu >= WHITE_COLS), uu < TEX_COLS)
    d0 = np.where(valid, d0, -1)
    d1 = np.full((H, W), 1, np.int64)
    ok = valid & (uu - d0 >= 0)
    off = np.where(rng.random((H, W)) < 0.25, rng.integers(1, 4, (H, W)), 0)
    d1[vv[ok], (uu - d0)[ok]] = (d0 + off)[ok]
    return d0.astype(np.int16), d1.astype(np.int16)


P1P2 = [(0.5, 2.0), (0.0, 0.0), (2.0, 1.0), (7.25, 100.0)]
REDU = [1, 3, 7]
COR_THRES = [-1, 0, 1, 254, 255, 300]
LR_MAX_DIFF = [0.5, 1.0, 2.5, 3.0, 2.0]
RV_S = [0, 5, 10 ** 6]
RV_RATIO = [0.01, 1.0, 1.5, float(np.nextafter(np.float32(1), np.float32(2))), 2.0]
REGION_VOTE_NUMS = [0, 1, 5]
DISP_OCC = [-2, -100]
REG_LAMBDA = [0.05, 1.0]

# Values of the lists above that cannot move the reference, and why (the host test asserts that
# they do not, and that every other value does):
#   lr_max_diff 0.5   |d - D2(u - d)| is an integer: `> 0.5` is `> 0`, the default
#   rv_ratio 0.01, 1  regionVote_my compares hist[most] / validNum, an INTEGER division
#                     (cpp:7270) that is 1 or 0, with the ratio: every ratio in (0, 1] fills
#                     exactly where all valid votes agree, as the default 0.4 does
INERT = {("lr_max_diff", 0.5), ("rv_ratio", 0.01), ("rv_ratio", 1.0)}
