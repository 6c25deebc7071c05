"""Restatement of dispOptimize's Do_vmTop branch (stereoMatching.cpp:1108-1128) in plain Python / numpy with
f32 scalars: selectTopCostFromVolumn (h:2405-2461) and genDispFromTopCostVm2 (cpp:1514-1885).

select(vol, num, thres)   -> (table [H][W][num + 1][2] f32, counts [H][W] int32); table entries past a pixel's
                             count stay 0 (the reference never writes or reads them), the count is also in
                             table[v, u, num, 0]
decide(table, counts, bgr_left, method, ts, has_cir2, color_limit) -> (int16 map, branch counters)

Counters of method 0: case1, case2, case3, case3_tie_by_cost (the largest num is shared, the cost sum decides),
dedup (a cost key already in the container: insert does not overwrite); method 1: m1_match, m1_fallback;
method 2: m2_pre, m2_aft, m2_none, m2_both.
"""
import numpy as np

f32 = np.float32
FLT_MAX = np.finfo(np.float32).max


def select(vol, num, thres):
    vol = np.asarray(vol, f32)
    H, W, D = vol.shape
    thres = f32(thres)
    table = np.zeros((H, W, num + 1, 2), f32)
    counts = np.zeros((H, W), np.int32)
    for v in range(H):
        for u in range(W):
            vm = vol[v, u].copy()   # vm[i].clone(): the volume itself is not modified
            first = f32(0)
            for k in range(num):
                small, disp = vm[0], 0
                for d in range(1, D):   # strict >: the lowest d wins a tie
                    if small > vm[d]:
                        small, disp = vm[d], d
                if k == 0:
                    first = small
                elif not (small < f32(first * thres)):   # one f32 multiply, one compare
                    break
                vm[disp] = FLT_MAX
                table[v, u, k, 0] = f32(disp)
                table[v, u, k, 1] = small
                counts[v, u] = k + 1
            table[v, u, num, 0] = f32(counts[v, u])
    return table, counts


def select_fast(vol, num, thres):
    """The same table by sorting: the k-th scan yields the k-th smallest (cost, d) pair while fewer than D are
    masked.  Only for num <= D and costs below FLT_MAX (used to prepare large fixtures; tests compare it with
    select on the small ones)."""
    vol = np.asarray(vol, f32)
    H, W, D = vol.shape
    assert num <= D
    thres = f32(thres)
    order = np.argsort(vol, axis=2, kind="stable")[:, :, :num]   # stable: the lowest d first among equals
    cost = np.take_along_axis(vol, order, axis=2)
    lim = (cost[:, :, :1] * thres).astype(f32)
    ok = cost < lim
    ok[:, :, 0] = True
    ok = np.logical_and.accumulate(ok, axis=2)   # the loop breaks at the first failure
    counts = ok.sum(axis=2).astype(np.int32)
    table = np.zeros((H, W, num + 1, 2), f32)
    table[:, :, :num, 0] = np.where(ok, order.astype(f32), f32(0))
    table[:, :, :num, 1] = np.where(ok, cost, f32(0))
    table[:, :, num, 0] = counts.astype(f32)
    return table, counts


NEIGH_V = (0, -1, 0, 1, -1, 1, -1, 1)   # l, u, r, d, lu, rd, ru, ld
NEIGH_U = (-1, 0, 1, 0, -1, 1, 1, -1)
INT_MAX = 2 ** 31 - 1


def _color_ok(a, b, thres=10):
    return all(abs(int(a[c]) - int(b[c])) <= thres for c in range(3))


def _decide0(table, counts, bgr, ts, has_cir2, color_limit, cnt):
    H, W = counts.shape
    disp = np.zeros((H, W), np.int16)
    for v in range(H):
        for u in range(W):
            n = int(counts[v, u])
            cand = [(int(table[v, u, k, 0]), f32(table[v, u, k, 1])) for k in range(n)]
            if u == 0 or v == 0 or n == 1:
                disp[v, u] = cand[0][0]
                cnt["case1"] += 1
                continue
            # std::map<float, int> keyed by cost; insert does not overwrite
            cont = {}

            def insert(c, d):
                key = float(c) + 0.0   # -0 and +0 are one key
                if key in cont:
                    cnt["dedup_ins"] += 1
                    if cont[key][1] != d:
                        cnt["dedup"] += 1
                else:
                    cont[key] = (c, d)

            for i in range(n):
                d0, c0 = cand[i]
                if not has_cir2:
                    insert(c0, d0)
                else:
                    for j in range(i + 1, n):
                        d1, c1 = cand[j]
                        if abs(d0 - d1) < ts:
                            insert(c0, d0)
                            insert(c1, d1)
            if not cont:   # case 2: the nearest candidate to four output values
                cnt["case2"] += 1
                pre1, pre2, lt = int(disp[v, u - 1]), int(disp[v - 1, u]), int(disp[v - 1, u - 1])
                rt = int(disp[v - 1, u + 1]) if u != W - 1 else 10000
                best = [[INT_MAX, -1] for _ in range(4)]
                for d, _ in cand:
                    for k, ref in enumerate((pre1, pre2, rt, lt)):
                        dif = abs(d - ref)
                        if dif < best[k][0]:
                            best[k] = [dif, d]
                m = min(b[0] for b in best)
                if m == best[3][0]:
                    e = best[3][1]
                elif m == best[0][0]:
                    e = best[0][1]
                elif m == best[1][0]:
                    e = best[1][1]
                else:
                    e = best[2][1]
                disp[v, u] = e if m < 1000 else cand[0][0]
                continue
            cnt["case3"] += 1
            num, cost = {}, {}
            for key in sorted(cont):   # the map iterates by ascending cost
                c, d = cont[key]
                num[d] = num.get(d, 0) + 1
                cost[d] = f32(cost.get(d, f32(0)) + c)
            for i in range(8):
                v_, u_ = v + NEIGH_V[i], u + NEIGH_U[i]
                if not (0 <= v_ < H and 0 <= u_ < W):
                    continue
                if color_limit and not _color_ok(bgr[v, u], bgr[v_, u_]):
                    continue
                for x in range(int(counts[v_, u_])):
                    d, c = int(table[v_, u_, x, 0]), f32(table[v_, u_, x, 1])
                    if d in num:
                        num[d] += 1
                        cost[d] = f32(cost[d] + c)
            d_a, num_most, cost_a = -1, -1, FLT_MAX
            for d in sorted(num):
                if num[d] > num_most or (num[d] == num_most and cost[d] < cost_a):
                    num_most, cost_a, d_a = num[d], cost[d], d
            if sum(1 for d in num if num[d] == num_most) > 1:
                cnt["case3_tie_by_cost"] += 1
            disp[v, u] = d_a
    return disp


def _nearest(cand_d, ref, limit):
    """`dif < 2 && dif < best` over the candidates in order; -1 when none matches."""
    best, out = limit, -1
    for d in cand_d:
        dif = int(abs(f32(d) - f32(ref)))   # int s = abs(short - float)
        if dif < 2 and dif < best:
            best, out = dif, int(d)
    return out


def _decide12(table, counts, bgr, method, cnt):
    H, W = counts.shape
    disp = np.zeros((H, W), np.int16)
    for v in range(H):
        for u in range(W):
            n = int(counts[v, u])
            ds = [int(table[v, u, k, 0]) for k in range(n)]
            if u == 0 or n == 1:
                disp[v, u] = ds[0]
                continue
            d0 = _nearest(ds, int(disp[v, u - 1]), 10000 if method == 1 else 1000000)
            if method == 1:
                cnt["m1_fallback" if d0 == -1 else "m1_match"] += 1
                disp[v, u] = ds[0] if d0 == -1 else d0
                continue
            d1 = -1
            if u < W - 1:
                d1 = _nearest(ds, int(table[v, u + 1, 0, 0]), 1000000)
            if d0 != -1 and d1 == -1:
                cnt["m2_pre"] += 1
                disp[v, u] = d0
            elif d0 == -1 and d1 != -1:
                cnt["m2_aft"] += 1
                disp[v, u] = d1
            elif d0 == -1 and d1 == -1:
                cnt["m2_none"] += 1
                disp[v, u] = ds[0]
            else:
                cnt["m2_both"] += 1
                pre = sum(abs(int(bgr[v, u, c]) - int(bgr[v, u - 1, c])) for c in range(3))
                aft = sum(abs(int(bgr[v, u, c]) - int(bgr[v, u + 1, c])) for c in range(3))
                disp[v, u] = d0 if pre <= aft else d1
    return disp


COUNTERS = ("case1", "case2", "case3", "case3_tie_by_cost", "dedup", "dedup_ins", "m1_match", "m1_fallback",
            "m2_pre", "m2_aft", "m2_none", "m2_both")


def decide(table, counts, bgr_left, method=0, ts=10, has_cir2=True, color_limit=False):
    """genDispFromTopCostVm2.  The colour image is I_c[0] (the left one) for both views."""
    cnt = {k: 0 for k in COUNTERS}
    table = np.asarray(table, f32)
    if method == 0:
        disp = _decide0(table, counts, bgr_left, int(ts), bool(has_cir2), bool(color_limit), cnt)
    elif method in (1, 2):
        disp = _decide12(table, counts, bgr_left, method, cnt)
    else:
        raise ValueError("vmTop_method must be 0, 1 or 2")
    return disp, cnt


def vmtop(vol, bgr_left, num=2, thres=f32(1.09), method=0, ts=10, has_cir2=True, color_limit=False):
    """The whole branch for one view: the int16 map."""
    table, counts = select(vol, num, thres) if num > vol.shape[2] else select_fast(vol, num, thres)
    return decide(table, counts, bgr_left, method, ts, has_cir2, color_limit)[0]
