"""numpy restatement of the reference's scan-line optimisers, written from its text: so (stereoMatching.cpp:6272-6394),
so_R2L (cpp:6683-6826) and so_T2D (cpp:6580-6681).

Each function takes the volume [H][W][D] float32 and the LEFT colour image [H][W][3] uint8 (I[0], for both views) and
returns (DP [H][W] int16, the accumulated volume [H][W][D] float32).  The penalties are parameters (the functions'
literals are SO_PN / R2L_PN / T2D_PN); so_t2d also takes `normalised`: True is the shipped line
`vmP[d] += (cost_min - c_min)` (cpp:6644), False the commented `vmP[d] += cost_min` (cpp:6645).

One step of the programme is the same in all three (cpp:6305-6334, 6606-6646, 6715-6797) and is vectorised over the
lines that are independent of each other (all rows of a column step for so / so_R2L, all columns of a row step for
so_T2D); the scan order, the predecessor, the discontinuity pair and the backtrack are written per function.
"""
import numpy as np

F = np.float32
FLT_MAX = np.finfo(np.float32).max
SO_PN = (1.2, 3.6)     # cpp:6305-6306
R2L_PN = (0.3, 0.9)    # cpp:6716-6717
T2D_PN = (0.3, 0.9)    # cpp:6607-6608


def _is_disc(a, b):
    """float sum = 0; sum += abs(IP[c] - IP_pre[c]) (c = 0 .. 2); sum /= 3; sum > 15 — per line."""
    s = np.abs(a.astype(np.int32) - b.astype(np.int32)).sum(axis=-1).astype(F)   # integers <= 765: exact in any order
    return (s / F(3)) > F(15)


def _step(pre, cur, disc, pn2, pn3, normalised):
    """pre, cur [L][D] float32, disc [L] bool -> (cur + addend [L][D] float32, the chosen disparity [L][D] int32)."""
    L, D = pre.shape
    P2 = np.where(disc, F(pn2) / F(2), F(pn2)).astype(F)[:, None]   # float Pn2 = ..; if (L_isDisc) Pn2 /= 2;
    P3 = np.where(disc, F(pn3) / F(2), F(pn3)).astype(F)[:, None]
    d_cmin = _first_min(pre)                                        # c_min = vmPre[0]; if (vmPre[d_l] < c_min) ..
    c_min = pre[np.arange(L), d_cmin]
    c_minus = np.full((L, D), FLT_MAX, F)
    c_plus = np.full((L, D), FLT_MAX, F)
    c_minus[:, 1:] = pre[:, :-1] + P2                               # d > 0 ? vmPre[d - 1] + Pn2 : max
    c_plus[:, :-1] = pre[:, 1:] + P2                                # d < d_ - 1 ? vmPre[d + 1] + Pn2 : max
    c_min = (c_min[:, None] + P3).astype(F)                         # c_min += Pn3
    d_min = np.tile(np.arange(D, dtype=np.int32), (L, 1))
    cost_min = pre.copy()
    m = c_minus < cost_min
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


def _first_min(c):
    """c_min = c[0]; for d = 1 ..: if (c[d] < c_min) — per line; `c_min > c[d]` (cpp:6659) is the same test."""
    # numpy's argmin returns the first index of the smallest value and orders -0 == +0: the loop's strict <
    return np.argmin(c, axis=1).astype(np.int32)


def so(vol, img, pn2=SO_PN[0], pn3=SO_PN[1]):
    vm = np.array(vol, F, copy=True)
    H, W, D = vm.shape
    trace = np.zeros((H, W, D), np.int32)
    for u in range(1, W):                                          # cpp:6282: u = 1 .. w_-1, pre = (v, u - 1)
        vm[:, u], trace[:, u] = _step(vm[:, u - 1], vm[:, u], _is_disc(img[:, u], img[:, u - 1]), pn2, pn3, False)
    DP = np.zeros((H, W), np.int16)
    rows = np.arange(H)
    d = _first_min(vm[:, W - 1])                                   # cpp:6372-6383
    DP[:, W - 1] = d
    for u in range(W - 1, 0, -1):                                  # cpp:6384-6391
        d = trace[rows, u, d]
        DP[:, u - 1] = d
    return DP, vm


def so_r2l(vol, img, pn2=R2L_PN[0], pn3=R2L_PN[1]):
    vm = np.array(vol, F, copy=True)
    H, W, D = vm.shape
    trace = np.zeros((H, W, D), np.int32)
    for u in range(W - 2, -1, -1):                                 # cpp:6691: u = w_-2 .. 0, pre = (v, u + 1)
        vm[:, u], trace[:, u] = _step(vm[:, u + 1], vm[:, u], _is_disc(img[:, u], img[:, u + 1]), pn2, pn3, False)
    DP = np.zeros((H, W), np.int16)
    rows = np.arange(H)
    d = _first_min(vm[:, 0])                                       # cpp:6806-6817
    DP[:, 0] = d
    for u in range(0, W - 1):                                      # cpp:6818-6824
        d = trace[rows, u, d]
        DP[:, u + 1] = d
    return DP, vm


def so_t2d(vol, img, pn2=T2D_PN[0], pn3=T2D_PN[1], normalised=True):
    """The accumulated volume is the reference's local clone vm_res (cpp:1095); vm[i] itself stays as it was."""
    vm = np.array(vol, F, copy=True)
    H, W, D = vm.shape
    trace = np.zeros((H, W, D), np.int32)
    for v in range(1, H):                                          # cpp:6588: v = 1 .. h_-1, pre = (v - 1, u)
        vm[v], trace[v] = _step(vm[v - 1], vm[v], _is_disc(img[v], img[v - 1]), pn2, pn3, normalised)
    # the backtrack of cpp:6651-6679 runs once per column of the outer loop; its last execution sees every column's
    # forward pass and overwrites all of DP, so it alone is the result
    DP = np.zeros((H, W), np.int16)
    cols = np.arange(W)
    d = _first_min(vm[H - 1])                                      # cpp:6654-6665: if (c_min > vP[d])
    DP[H - 1] = d
    for v in range(H - 1, 0, -1):                                  # cpp:6667-6679
        d = trace[v, cols, d]
        DP[v - 1] = d
    return DP, vm
