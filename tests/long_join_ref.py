"""A plain model of mg_lchain_rmq's scoring pass (the "long join": oracle/mm_rmq.c mmo_lchain_rmq_fill, csrc/sh_long.h lr_rmq_fill), written
from what the pass asks of its two trees and not from either implementation:

  step i, anchors sorted by x:  the anchors of strictly smaller x enter the look-back window; those of another strand / contig or more than
  max_dist = max(max_gap, bw_long) reference bases back leave it (and the oldest beyond rmq_size_cap); among the window's anchors with
  q_i - max_dist < y < q_i (or y == q_i for anchor 0) the one of smallest priority -(f + 0.5 * pen_gap * (x + y)) is scored; unless it
  is an exact continuation the inner window (min(rmq_inner_dist, max_dist) bases) is walked in descending (y, index) from y <= q_i - 1 down to
  y >= q_i - inner with mg_lchain_dp's skip rule.

The trees only matter where the smallest priority is SHARED: which of the tied anchors a tree returns depends on its shape.  The model reports
those steps and sorts them into the classes the device's tie rule knows, and it measures what the device's fixed-size structures must hold
(same-x group, inner window, look-back window, the window while a tied stretch is open), from which verdict() says whether an instance of
lr_rmq_fill must decline the case.  tests/test_long_oracle_cpu.py and tests/test_long_join_cases_cpu.py compare it with the oracle."""
import numpy as np

# the five instances the product launches: sh_dbg_long_join's fill variant -> (NR, TREE)
INSTANCES = {1: (512, False), 2: (4096, False), 3: (4096, False), 4: (1024, True), 5: (4096, True)}
TCAP = {1024: 1664, 4096: 1792}      # nodes of the LDS tree beside the ring (k_long_chains)
TIE_NONE_ACCEPTED, TIE_IMPROVED, TIE_MATTERS = "a", "b", "m"


def rblk(nr):
    """completed 64-anchor blocks that are always inside the ring (LRQ_RBLK)"""
    return nr // 64 - 4


def samex(nr):
    """anchors that may wait on one reference position (LRQ_SAMEX): 191 for every ring"""
    return nr - 1 - (rblk(nr) + 1) * 64


def log2_f32(x):
    """minimap2's mg_log2 on a float32 array, operation for operation in float32"""
    z = np.ascontiguousarray(x, np.float32).view(np.uint32).copy()
    l2 = (((z >> np.uint32(23)) & np.uint32(255)).astype(np.int32) - 128).astype(np.float32)
    z &= ~np.uint32(255 << 23)
    z += np.uint32(127 << 23)
    zf = z.view(np.float32)
    return l2 + ((np.float32(-0.34484843) * zf + np.float32(2.02466578)) * zf - np.float32(0.67487759))


def sc_simple(dr, dq, span, pen_gap, pen_skip):
    """comput_sc_simple over arrays: (score, exact, width)"""
    dr, dq, span = np.asarray(dr, np.int64), np.asarray(dq, np.int64), np.asarray(span, np.int64)
    dd, dg = np.abs(dr - dq), np.minimum(dr, dq)
    sc = np.minimum(span, dg)
    exact = (dd == 0) & (dg <= span)
    lin = np.float32(pen_gap) * dd.astype(np.float32) + np.float32(pen_skip) * dg.astype(np.float32)
    lg = np.where(dd >= 1, log2_f32((dd + 1).astype(np.float32)), np.float32(0)).astype(np.float32)
    pen = (lin + np.float32(0.5) * lg).astype(np.int64)      # (int32_t) of a float: towards zero
    return np.where((dd != 0) | (dq > span), sc - pen, sc), exact, dd


def stretch_starts(x, max_gap, bw_long):
    """anchors at which the look-back window is empty whatever came before: another strand / contig, or more than max_dist bases on"""
    x = np.asarray(x, np.uint64)
    md = np.uint64(max(max_gap, bw_long))
    j = np.nonzero(((x[1:] >> np.uint64(32)) != (x[:-1] >> np.uint64(32))) | (x[1:] > x[:-1] + md))[0] + 1
    return [int(v) for v in j]


def join_model(x, y, max_gap, bw_long, inner, max_skip, cap, pen_gap, pen_skip, follow=None):
    """x, y (= q_span << 32 | qpos): the anchors, ascending in x.  follow = (f, p) of an implementation with trees: at a shared minimum that
    matters the model then takes the tied anchor that leads to follow's f[i], p[i] (steps where none does are listed in follow_fail) and so
    stays on that implementation's trajectory; without it the smallest index is taken.
    Returns a dict: F, P; shared = [(step, class)], tied = {step: the tied anchors}; matter; pending_max (largest same-x group waiting to enter); inner_span_max (the inner
    window, the arriving anchor included, as it stands when an anchor arrives); list_max (entries of the inner window's list when one is
    added); lookback_max; tree_need (nodes a tree needs that is built for, and kept over, every stretch with a shared minimum: the window
    after the additions, plus one spare node while anchors leave); starts; BJ, ST, I0, ST_IN (per step: the scored anchor or -1, the
    window [ST, I0), the inner window's start); scan_len (inner-scan entries looked at, per step); skip_breaks (positions in the scan where the skip rule ended it);
    equal_hits ((step, anchor) where a scanned anchor's score equalled the maximum so far and was, rightly, not taken)."""
    x, y = np.ascontiguousarray(x, np.uint64), np.ascontiguousarray(y, np.uint64)
    n = len(x)
    xl = (x & np.uint64(0xffffffff)).astype(np.int64); hi = (x >> np.uint64(32)).astype(np.int64)
    ql = (y & np.uint64(0xffffffff)).astype(np.int64); span = ((y >> np.uint64(32)) & np.uint64(0xff)).astype(np.int64)
    xq = [int(v) for v in x]
    md = max(max_gap, bw_long); mdi = min(max(inner, 0), md)
    half = 0.5 * float(np.float32(pen_gap))
    F = np.zeros(n, np.int64); PRI = np.zeros(n, np.float64)
    P, T = [-1] * n, [0] * n
    stamp = [0]
    BJ, ST, I0, ST_IN = [-1] * n, [0] * n, [0] * n, [0] * n
    scan_len, skip_breaks, shared, follow_fail, equal_hits = [0] * n, [], [], [], []
    pending_max = inner_span_max = list_max = lookback_max = tree_need = 0
    i0 = st = st_in = 0
    peak, tied_stretch, tied_at = 0, False, {}

    def step(i, bj, qi):
        sc, ex, w = sc_simple([xl[i] - xl[bj]], [qi - ql[bj]], [span[bj]], pen_gap, pen_skip)
        sc, ex, w = int(sc[0]) + int(F[bj]), bool(ex[0]), int(w[0])
        max_f, max_j, seen, brk = int(span[i]), -1, 0, -1
        if w <= bw_long and sc > max_f: max_f, max_j = sc, bj
        if not ex and mdi > 0 and i0 > st_in and qi > 0:
            yy = ql[st_in:i0]
            idx = np.nonzero((yy <= qi - 1) & (yy >= qi - mdi))[0]
            if len(idx):
                idx = idx[np.lexsort((idx, yy[idx]))[::-1]] + st_in      # descending (y, index)
                s2, _, w2 = sc_simple(xl[i] - xl[idx], qi - ql[idx], span[idx], pen_gap, pen_skip)
                s2 = (s2 + F[idx]).tolist(); okw = (w2 <= bw_long).tolist(); js = idx.tolist()
                stamp[0] += 1
                mark, n_skip = stamp[0], 0
                for e in range(len(js)):
                    seen = e + 1
                    if not okw[e]: continue
                    j = js[e]
                    if s2[e] == max_f and T[j] != mark: equal_hits.append((i, j))
                    if s2[e] > max_f:
                        max_f, max_j = s2[e], j
                        if n_skip > 0: n_skip -= 1
                    elif T[j] == mark:
                        if s2[e] == max_f: equal_hits.append((i, j))
                        n_skip += 1
                        if n_skip > max_skip: brk = e; break
                    if P[j] >= 0: T[P[j]] = mark
        return max_f, max_j, seen, brk

    for i in range(n):
        qi = int(ql[i])
        seg = i > 0 and hi[i] != hi[i - 1]
        pending_max = max(pending_max, i - i0)
        if mdi > 0: inner_span_max = max(inner_span_max, 0 if seg else i - st_in)
        grown = st
        if i0 < i and xq[i0] != xq[i]:
            PRI[i0:i] = -(F[i0:i].astype(np.float64) + half * (xl[i0:i] + ql[i0:i]).astype(np.float64))
            if mdi > 0: list_max = max(list_max, i - 1 - st_in)
            i0 = i
        while st < i and (hi[st] != hi[i] or xq[i] > xq[st] + md): st += 1
        if i0 - st > cap: st = i0 - cap
        if mdi > 0:
            while st_in < i and (hi[st_in] != hi[i] or xq[i] > xq[st_in] + mdi): st_in += 1
            if i0 - st_in > cap: st_in = i0 - cap
        peak = max(peak, i0 - grown + (1 if min(st, i0) > grown else 0))
        lookback_max = max(lookback_max, i0 - st)
        ST[i], I0[i], ST_IN[i] = st, i0, st_in
        max_f, max_j = int(span[i]), -1
        if i0 > st:
            yy = ql[st:i0]
            m = (yy > qi - md) & (yy < qi)
            if st == 0 and yy[0] == qi: m[0] = True      # the key bound (q_i, 0): anchor 0 alone may share q_i
            idx = np.nonzero(m)[0]
            if len(idx):
                pr = PRI[st:i0][idx]
                tied = (idx[pr == pr.min()] + st).tolist()
                bj = tied[0]
                if len(tied) == 1:
                    max_f, max_j, scan_len[i], brk = step(i, bj, qi)
                else:
                    tied_stretch = True
                    ta = np.array(tied)
                    sc, ex, w = sc_simple(xl[i] - xl[ta], qi - ql[ta], span[ta], pen_gap, pen_skip)
                    sc = sc + F[ta]
                    acc = (w <= bw_long) & (sc > span[i])
                    n_acc, n_ex = int(acc.sum()), int(ex.sum())
                    max_f, max_j, scan_len[i], brk = step(i, bj, qi)
                    if n_acc == 0 and n_ex in (0, len(tied)): cls = TIE_NONE_ACCEPTED
                    elif n_acc == len(tied) and n_ex == 0 and int(sc.min()) == int(sc.max()) and max_f > int(sc[0]): cls = TIE_IMPROVED
                    else: cls = TIE_MATTERS
                    if cls == TIE_MATTERS and follow is not None:
                        want = (int(follow[0][i]), int(follow[1][i]))
                        for b in tied:
                            r = step(i, b, qi)
                            if (r[0], r[1]) == want: bj = b; max_f, max_j, scan_len[i], brk = r; break
                        else: follow_fail.append(i)
                    shared.append((i, cls)); tied_at[i] = tied
                if brk >= 0: skip_breaks.append((i, brk))
                BJ[i] = bj
        else:      # the window is empty (and so are upstream's trees): nothing before matters from here on
            if tied_stretch: tree_need = max(tree_need, peak)
            peak, tied_stretch = 0, False
        F[i], P[i] = max_f, max_j
    if tied_stretch: tree_need = max(tree_need, peak)
    return {"F": F.astype(np.int32), "P": np.array(P, np.int32), "shared": shared, "matter": any(c == TIE_MATTERS for _, c in shared),
            "follow_fail": follow_fail, "tied": tied_at, "pending_max": pending_max, "inner_span_max": inner_span_max, "list_max": list_max,
            "lookback_max": lookback_max, "tree_need": tree_need, "starts": stretch_starts(x, max_gap, bw_long),
            "BJ": BJ, "ST": ST, "I0": I0, "ST_IN": ST_IN, "scan_len": scan_len, "skip_breaks": skip_breaks, "equal_hits": equal_hits, "inner_on": mdi > 0}


def declines(m, nr, tree, cap):
    """must lr_rmq_fill<nr, tree> return false on the case whose model is m?  (cap: rmq_size_cap)
    - its windows live in a ring of nr anchors, so it leaves a cap below nr to the one-lane version;
    - at most samex(nr) anchors wait on one reference position;
    - the inner window, with the arriving anchor, and its list stay below nr;
    - tree: the LDS tree holds TCAP[nr] nodes."""
    if cap < nr: return True
    if m["pending_max"] > samex(nr): return True
    if m["inner_on"] and (m["inner_span_max"] >= nr or m["list_max"] >= nr): return True
    if tree and m["tree_need"] > TCAP[nr]: return True
    return False


def ring_place(m, nr, i):
    """where step i's scored anchor lies for a ring of nr anchors: 'new' (the block being filled), 'ring' (a completed block in LDS), 'old'
    (behind the ring: HBM), and how many completed blocks of the window lie behind the ring"""
    bj, st, i0 = m["BJ"][i], m["ST"][i], m["I0"][i]
    done = i0 // 64
    ring_lo = max(done - rblk(nr), 0) * 64
    n_old = max(ring_lo // 64 - st // 64, 0)
    place = None if bj < 0 else "new" if bj >= done * 64 else "ring" if bj >= ring_lo else "old"
    return place, n_old, (None if bj < 0 else i - bj < nr - 64)
