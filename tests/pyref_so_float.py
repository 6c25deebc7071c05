"""numpy restatement of the reference's scan-line optimisers for costs of either sign, +-0 and NaN: so
(stereoMatching.cpp:6272-6394), so_R2L (cpp:6683-6826) and so_T2D (cpp:6580-6681) with every first minimum taken as
the C++ loop takes it (cpp:6354-6363, 6396-6406):

    m = c[0], i = 0;  for d = 1 .. D-1: if (c[d] < m) { m = c[d]; i = d; }

so -0 == +0 (the first of equal values wins), a NaN at index 0 is sticky ((NaN, 0) whatever follows) and a NaN at any
other index never wins.  tests/pyref_so.py takes np.argmin, which returns the first NaN wherever it stands; it is right
for the finite volumes it is used on and stays as it is.  The forward step is pyref_so's text with the minimum handed
in: every `<` is false when a side is NaN, as in C.

`first_min` is a parameter so that the tests can also compute what a *wrong* minimum would give (first_min_unsigned:
bit patterns as unsigned integers, the kernels for costs >= +0; first_min_nan_dropping: a v_min_f32 reduction;
first_min_signed_zero: an ordering with -0 < +0).  With a +inf cost the reference's backtrack leaves its trace; here,
as in the kernels, the backtrack's disparity is clipped to [0, D) (the affected line's map is unspecified).
"""
import numpy as np

from pyref_so import F, FLT_MAX, R2L_PN, SO_PN, T2D_PN, _is_disc

__all__ = ["first_min_c", "so", "so_r2l", "so_t2d", "SO_PN", "R2L_PN", "T2D_PN"]


def first_min_c(c):
    """c [L][D] float32 -> the loop's index i per line, int32."""
    c = np.asarray(c, F)
    nan = np.isnan(c)
    # with c[0] a number, the loop returns the first index of the smallest number (c[0] <= +inf wins every tie against a
    # NaN replaced by +inf); with c[0] NaN, 0
    i = np.argmin(np.where(nan, F(np.inf), c), axis=1)
    return np.where(nan[:, 0], 0, i).astype(np.int32)


def _ordered_key(c, fold_zero):
    """Unsigned keys that order like the floats (NaN aside): negative values have every bit flipped, the others the
    sign bit set; fold_zero maps -0 onto +0 first."""
    b = np.ascontiguousarray(c, F).view(np.uint32).copy()
    if fold_zero:
        b[(b << np.uint32(1)) == 0] = 0
    neg = (b >> np.uint32(31)).astype(bool)
    return np.where(neg, ~b, b | np.uint32(0x80000000))


def first_min_unsigned(c):
    """The first index of the smallest bit pattern, as an unsigned integer (k_so for costs >= +0)."""
    return np.argmin(np.ascontiguousarray(c, F).view(np.uint32), axis=1).astype(np.int32)


def first_min_nan_dropping(c):
    """np.nanargmin-style: a NaN never wins, at index 0 either (what a v_min_f32 reduction gives); all NaN: 0."""
    c = np.asarray(c, F)
    return np.argmin(np.where(np.isnan(c), F(np.inf), c), axis=1).astype(np.int32)


def first_min_signed_zero(c):
    """first_min_c with -0 ordered below +0 (an ordered-integer key that keeps the two zeros apart)."""
    c = np.asarray(c, F)
    nan = np.isnan(c)
    key = np.where(nan, np.uint32(0xFFFFFFFF), _ordered_key(c, False))
    return np.where(nan[:, 0], 0, np.argmin(key, axis=1)).astype(np.int32)


def _step(pre, cur, disc, pn2, pn3, normalised, first_min):
    """pyref_so._step with the minimum handed in: pre, cur [L][D], disc [L] -> (cur + addend, the chosen disparity)."""
    L, D = pre.shape
    P2 = np.where(disc, F(pn2) / F(2), F(pn2)).astype(F)[:, None]   # float Pn2 = ..; if (L_isDisc) Pn2 /= 2;
    P3 = np.where(disc, F(pn3) / F(2), F(pn3)).astype(F)[:, None]
    d_cmin = first_min(pre)                                         # c_min = vmPre[0]; if (vmPre[d_l] < c_min) ..
    c_min = pre[np.arange(L), d_cmin]
    c_minus = np.full((L, D), FLT_MAX, F)
    c_plus = np.full((L, D), FLT_MAX, F)
    with np.errstate(invalid="ignore", over="ignore"):
        c_minus[:, 1:] = pre[:, :-1] + P2                           # d > 0 ? vmPre[d - 1] + Pn2 : max
        c_plus[:, :-1] = pre[:, 1:] + P2                            # d < d_ - 1 ? vmPre[d + 1] + Pn2 : max
        c_min = (c_min[:, None] + P3).astype(F)                     # c_min += Pn3
        d_min = np.tile(np.arange(D, dtype=np.int32), (L, 1))
        cost_min = pre.copy()
        m = c_minus < cost_min                                      # false when a side is NaN, as in C
        d_min = np.where(m, d_min - 1, d_min)
        cost_min = np.where(m, c_minus, cost_min)
        m = c_plus < cost_min
        d_min = np.where(m, np.arange(D, dtype=np.int32)[None, :] + 1, d_min)
        cost_min = np.where(m, c_plus, cost_min)
        m = c_min < cost_min
        d_min = np.where(m, d_cmin[:, None], d_min)
        cost_min = np.where(m, np.broadcast_to(c_min, (L, D)), cost_min)
        add = (cost_min - c_min).astype(F) if normalised else cost_min
        out = (cur + add).astype(F)
    assert out.dtype == F and P2.dtype == F and c_min.dtype == F
    return out, d_min.astype(np.int32)


def so(vol, img, pn2=SO_PN[0], pn3=SO_PN[1], first_min=first_min_c):
    vm = np.array(vol, F, copy=True)
    H, W, D = vm.shape
    trace = np.zeros((H, W, D), np.int32)
    for u in range(1, W):                                          # cpp:6282: u = 1 .. w_-1, pre = (v, u - 1)
        vm[:, u], trace[:, u] = _step(vm[:, u - 1], vm[:, u], _is_disc(img[:, u], img[:, u - 1]), pn2, pn3, False, first_min)
    DP = np.zeros((H, W), np.int16)
    rows = np.arange(H)
    d = first_min(vm[:, W - 1])                                    # cpp:6372-6383
    DP[:, W - 1] = d
    for u in range(W - 1, 0, -1):                                  # cpp:6384-6391
        d = np.clip(trace[rows, u, d], 0, D - 1)
        DP[:, u - 1] = d
    return DP, vm


def so_r2l(vol, img, pn2=R2L_PN[0], pn3=R2L_PN[1], first_min=first_min_c):
    vm = np.array(vol, F, copy=True)
    H, W, D = vm.shape
    trace = np.zeros((H, W, D), np.int32)
    for u in range(W - 2, -1, -1):                                 # cpp:6691: u = w_-2 .. 0, pre = (v, u + 1)
        vm[:, u], trace[:, u] = _step(vm[:, u + 1], vm[:, u], _is_disc(img[:, u], img[:, u + 1]), pn2, pn3, False, first_min)
    DP = np.zeros((H, W), np.int16)
    rows = np.arange(H)
    d = first_min(vm[:, 0])                                        # cpp:6806-6817
    DP[:, 0] = d
    for u in range(0, W - 1):                                      # cpp:6818-6824
        d = np.clip(trace[rows, u, d], 0, D - 1)
        DP[:, u + 1] = d
    return DP, vm


def so_t2d(vol, img, pn2=T2D_PN[0], pn3=T2D_PN[1], normalised=True, first_min=first_min_c):
    """The accumulated volume is the reference's local clone vm_res (cpp:1095); vm[i] itself stays as it was."""
    vm = np.array(vol, F, copy=True)
    H, W, D = vm.shape
    trace = np.zeros((H, W, D), np.int32)
    for v in range(1, H):                                          # cpp:6588: v = 1 .. h_-1, pre = (v - 1, u)
        vm[v], trace[v] = _step(vm[v - 1], vm[v], _is_disc(img[v], img[v - 1]), pn2, pn3, normalised, first_min)
    DP = np.zeros((H, W), np.int16)
    cols = np.arange(W)
    d = first_min(vm[H - 1])                                       # cpp:6654-6665: if (c_min > vP[d])
    DP[H - 1] = d
    for v in range(H - 1, 0, -1):                                  # cpp:6667-6679
        d = np.clip(trace[v, cols, d], 0, D - 1)
        DP[v - 1] = d
    return DP, vm


def same_floats(a, b):
    """NaN at the same positions, and the same bits everywhere else (NaN payloads and signs are not pinned)."""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])
