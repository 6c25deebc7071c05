"""Plain-loop restatement of refine()'s discontinuity adjustment (discontinuityAdjust, stereoMatching.cpp:6057-6136)
with the three OpenCV calls in the integer forms DESIGN 19 records: DP[0] to 8 bits, equalizeHist, GaussianBlur
(3 x 3, sigma 4, BORDER_REFLECT_101, 8.8 fixed point), Canny(20, 60, aperture 3, L1 gradient) with a stack-based
hysteresis, then the in-place raster-order adjustment.  Written from those definitions and the reference's loop,
independent of the kernels: it is what the GPU stage is compared against.  refine_da composes it with the C
oracle's stages and tests/pyref_refine_ext.py's.
"""
import math

import numpy as np

import pyref_refine_ext as RX

f32 = np.float32
CANNY_LOW, CANNY_HIGH = 20, 60
DIRECTIONS_H = (-1, 1, -1, 1, -1, 1, 0, 0)   # cpp:6069
DIRECTIONS_W = (-1, 1, 0, 0, 1, -1, -1, 1)   # cpp:6070


def cv_round(x):
    """cvRound: round half to even."""
    return int(np.rint(x))


def gaussian_taps(sigma=4.0, ksize=3):
    """getGaussianKernel in double, normalised, each tap cvRound(k * 256): OpenCV's 8-bit fixed-point kernel."""
    r = ksize // 2
    k = [math.exp(-(i - r) * (i - r) / (2.0 * sigma * sigma)) for i in range(ksize)]
    s = sum(k)
    return tuple(cv_round(x / s * 256.0) for x in k)


BLUR_SIDE, BLUR_CENTRE = gaussian_taps()[:2]


def to_u8(dp):
    return np.clip(np.asarray(dp, np.int32), 0, 255).astype(np.uint8)


def equalize_lut(hist, total):
    """The LUT of equalizeHist for a 256-bin histogram, or None where the image is one constant."""
    i = 0
    while hist[i] == 0:
        i += 1
    if hist[i] == total:
        return None
    scale = f32(255.0) / f32(total - hist[i])
    lut = [0] * 256
    s = 0
    for j in range(i + 1, 256):
        s += int(hist[j])
        lut[j] = min(max(cv_round(f32(s) * scale), 0), 255)   # one float multiply
    return lut


def equalize(img):
    img = np.asarray(img, np.uint8)
    hist = [0] * 256
    for x in img.ravel():
        hist[x] += 1
    lut = equalize_lut(hist, img.size)
    if lut is None:
        return img.copy()
    out = np.empty_like(img)
    H, W = img.shape
    for h in range(H):
        for w in range(W):
            out[h, w] = lut[img[h, w]]
    return out


def reflect101(i, n):
    if n == 1:
        return 0
    if i < 0:
        return -i
    if i >= n:
        return 2 * n - 2 - i
    return i


def blur(img, ks=BLUR_SIDE, kc=BLUR_CENTRE):
    H, W = img.shape
    a = np.asarray(img, np.int64)
    rows = np.empty((H, W), np.int64)
    for h in range(H):
        for w in range(W):
            rows[h, w] = ks * a[h, reflect101(w - 1, W)] + kc * a[h, w] + ks * a[h, reflect101(w + 1, W)]
    out = np.empty((H, W), np.uint8)
    for h in range(H):
        for w in range(W):
            c = ks * rows[reflect101(h - 1, H), w] + kc * rows[h, w] + ks * rows[reflect101(h + 1, H), w]
            out[h, w] = min((c + 32768) >> 16, 255)
    return out


def sobel(img):
    H, W = img.shape
    a = np.asarray(img, np.int32)
    dx = np.empty((H, W), np.int32)
    dy = np.empty((H, W), np.int32)
    for h in range(H):
        hu, hd = max(h - 1, 0), min(h + 1, H - 1)
        for w in range(W):
            wl, wr = max(w - 1, 0), min(w + 1, W - 1)
            dx[h, w] = (a[hu, wr] + 2 * a[h, wr] + a[hd, wr]) - (a[hu, wl] + 2 * a[h, wl] + a[hd, wl])
            dy[h, w] = (a[hd, wl] + 2 * a[hd, w] + a[hd, wr]) - (a[hu, wl] + 2 * a[hu, w] + a[hu, wr])
    return dx, dy


def candidates(dx, dy, low):
    """(candidate mask, magnitude): m > low and the non-maximum suppression of Canny's integer path."""
    H, W = dx.shape
    mag = np.abs(dx) + np.abs(dy)
    p = np.zeros((H + 2, W + 2), np.int64)   # magnitudes outside the image are 0
    p[1:-1, 1:-1] = mag

    def M(h, w):
        return p[h + 1, w + 1]

    cand = np.zeros((H, W), bool)
    for h in range(H):
        for w in range(W):
            m = int(mag[h, w])
            if m <= low:
                continue
            x, y = abs(int(dx[h, w])), abs(int(dy[h, w])) << 15
            t22 = x * 13573
            if y < t22:
                ok = m > M(h, w - 1) and m >= M(h, w + 1)
            elif y > t22 + (x << 16):
                ok = m > M(h - 1, w) and m >= M(h + 1, w)
            else:
                s = -1 if (int(dx[h, w]) ^ int(dy[h, w])) < 0 else 1
                ok = m > M(h - 1, w - s) and m > M(h + 1, w + s)
            cand[h, w] = ok
    return cand, mag


def hysteresis(cand, mag, high):
    """255 on every candidate 8-connected, through candidates, to a candidate with m > high (a stack, as Canny's)."""
    H, W = cand.shape
    edges = np.zeros((H, W), np.uint8)
    stack = [(h, w) for h in range(H) for w in range(W) if cand[h, w] and mag[h, w] > high]
    for h, w in stack:
        edges[h, w] = 255
    while stack:
        h, w = stack.pop()
        for dh in (-1, 0, 1):
            for dw in (-1, 0, 1):
                a, b = h + dh, w + dw
                if 0 <= a < H and 0 <= b < W and cand[a, b] and not edges[a, b]:
                    edges[a, b] = 255
                    stack.append((a, b))
    return edges


def canny(img, low=CANNY_LOW, high=CANNY_HIGH):
    """Returns (edges, candidates, strong)."""
    if low > high:
        low, high = high, low
    dx, dy = sobel(img)
    cand, mag = candidates(dx, dy, low)
    return hysteresis(cand, mag, high), cand, cand & (mag > high)


def image_stages(img, first=0, low=CANNY_LOW, high=CANNY_HIGH, ks=BLUR_SIDE, kc=BLUR_CENTRE):
    """The image enters at stage `first`: 0 equalise, 1 blur, 2 Canny.  Returns dict(eq, blur, edges) (None for the
    stages before `first`)."""
    eq = bl = None
    x = np.asarray(img, np.uint8)
    if first <= 0:
        x = eq = equalize(x)
    if first <= 1:
        x = bl = blur(x, ks, kc)
    return {"eq": eq, "blur": bl, "edges": canny(x, low, high)[0]}


def direction_of(E, h, w):
    """cpp:6079-6098, the two nested ifs that leave -1 included."""
    if E[h - 1, w - 1] and E[h + 1, w + 1]:
        return 4
    if E[h - 1, w + 1] and E[h + 1, w - 1]:
        return 0
    if E[h - 1, w] or E[h - 1, w - 1] or E[h - 1, w + 1]:
        if E[h + 1, w] or E[h + 1, w - 1] or E[h + 1, w + 1]:
            return 6
        return -1
    if E[h - 1, w - 1] or E[h, w - 1] or E[h + 1, w - 1]:
        if E[h - 1, w + 1] or E[h, w + 1] or E[h + 1, w + 1]:
            return 2
    return -1


def adjust(dp, edges, vm, stats=None):
    """cpp:6069-6135 in place on a copy, in raster order.  The one deviation: a disparity >= D reads its
    cost as -1 where the reference reads outside the volume.  stats (a dict) receives `changed`, the pixels
    rewritten, and `chained`, the pixels that read a neighbour that had itself been rewritten."""
    d = np.array(dp, np.int16)
    H, W = d.shape
    D = vm.shape[2]
    rewritten = np.zeros((H, W), bool)
    chained = 0
    minus1 = f32(-1)

    def cost_at(h, w, x):
        return vm[h, w, x] if 0 <= x < D else minus1

    for h in range(1, H - 1):
        for w in range(1, W - 1):
            if not edges[h, w]:
                continue
            k = direction_of(edges, h, w)
            if k == -1:
                continue
            x = int(d[h, w])
            if x < 0:
                continue
            h1, w1 = h + DIRECTIONS_H[k], w + DIRECTIONS_W[k]
            h2, w2 = h + DIRECTIONS_H[k + 1], w + DIRECTIONS_W[k + 1]
            assert not rewritten[h2, w2]   # the second side is later in raster order
            chained += bool(rewritten[h1, w1])
            cost = cost_at(h, w, x)
            d1, d2 = int(d[h1, w1]), int(d[h2, w2])
            cost1 = cost_at(h1, w1, d1) if d1 >= 0 else minus1
            cost2 = cost_at(h2, w2, d2) if d2 >= 0 else minus1
            new = x
            if cost1 >= 0 and cost1 < cost:      # a NaN compares false
                new, cost = d1, cost1
            if cost2 != -1 and cost2 < cost:
                new = d2
            if new != x:
                d[h, w] = new
                rewritten[h, w] = True
    if stats is not None:
        stats["changed"] = int(rewritten.sum())
        stats["chained"] = chained
    return d


def discontinuity_adjust(dp, vm, low=CANNY_LOW, high=CANNY_HIGH, ks=BLUR_SIDE, kc=BLUR_CENTRE, edges=None, stats=None):
    """The whole stage on one map.  Returns (map, edge map); `edges` replaces Canny's map."""
    if edges is None:
        edges = image_stages(to_u8(dp), 0, low, high, ks, kc)["edges"]
    return adjust(dp, edges, vm, stats), edges


def refine_da(O, cfg, d0, d1, arms_l, bgr, vm, do_da=True, do_pkr=False, do_bg=False, do_se=False, **da_kw):
    """refine() (cpp:1364-1506) with the oracle module O's stages, pyref_refine_ext's and the adjustment in the
    reference's order: ... -> BGIpol -> DA -> SE -> last median.  Returns dict(disp, edges, mask, se)."""
    d = O.lr_check(d0, d1, cfg)
    mask = se = edges = None
    if do_pkr:
        mask = RX.cal_pkr(vm)
        d = RX.sign_dp(d, mask)
    if cfg.do_region_vote:
        for _ in range(cfg.region_vote_nums):
            d = O.region_vote(d, arms_l, cfg)
    if cfg.do_proper_ipol:
        for _ in range(cfg.region_vote_nums):
            d = O.proper_ipol(d, bgr, cfg)
    if do_bg:
        d = RX.bg_ipol(d, RX.BG_IPL_DEPTH)
    if do_da:
        d, edges = discontinuity_adjust(d, vm, **da_kw)
    if do_se:
        se = RX.median3_f32(RX.subpixel(d, vm))
    if cfg.do_last_median:
        d = O.median3(d)
    return {"disp": d, "edges": edges, "mask": mask, "se": se}
