"""A plain model of minimap2's chaining: mg_lchain_dp and mg_chain_backtrack as the textbook sequential programme, in
Python integers.  It is the third voice beside the oracle (oracle/mm_oracle.c, through mmo_chain_arrays) and the device variants of
csrc/sh_chain.h: tests/test_chain_cases_cpu.py holds it against the oracle, tests/test_chain_gpu.py holds the device against both.

Only the pair score is borrowed: mmo_comput_sc, which tests/golden/chain_kat.json pins, so that there is one float path.

Besides f and p the model reports, per anchor, what happened on the way - the events the coverage checks of the case table need.
"""
from collections import namedtuple

NONE = -(1 << 31)

Opt = namedtuple("Opt", "k is_sr min_cnt min_sc max_gap max_gap_ref max_frag_len bw max_skip max_iter gap_scale skip_scale")
# per anchor: the window [st, i), whether max_iter cut it, the valid predecessors the scan met (all of the window's unless it broke off, and
# then more than max_skip), the scan position (0 = i - 1) at which the
# scan broke off (None: it ran to st), whether a new maximum came while n_skip was 0 after it had been above 0, how many times n_skip came
# back to 0 from above, whether max_ii was consulted, whether it won, whether it had been dropped as far and searched again, where it was,
# the scan's length, whether two predecessors gave the same best sum, whether the search for max_ii met its top f twice
Event = namedtuple("Event", "st cut n_valid brk dec_at_zero touch_zero consulted won far max_ii scanned tie ii_tie")
Result = namedtuple("Result", "f p chains t n_u best events")


def dists(o, qlen):
    """max_dist_x, max_dist_y as mm_map_frag and mg_lchain_dp settle them"""
    mdy = max(qlen, o.max_gap) if o.is_sr else o.max_gap
    if o.max_gap_ref > 0:
        mdx = o.max_gap_ref
    elif o.max_frag_len > 0:
        mdx = max(o.max_frag_len - qlen, o.max_gap)
    else:
        mdx = o.max_gap
    return max(mdx, o.bw), max(mdy, o.bw)


class Scorer:
    """sc(i, j) through the oracle's mmo_comput_sc, remembered per (dq, dr)"""

    def __init__(self, L, o, qlen):
        import numpy as np
        self.L, self.o = L, o
        self.mdx, self.mdy = dists(o, qlen)
        self.pen_gap = float(np.float32(float(np.float32(o.gap_scale)) * 0.01 * o.k))
        self.pen_skip = float(np.float32(float(np.float32(o.skip_scale)) * 0.01 * o.k))
        self.memo = {}

    def __call__(self, xi, qi, xj, qj):
        # the score only looks at the low 32 bits of x: the window keeps other strands and contigs out
        dq, dr = qi - qj, ((xi & 0xffffffff) - (xj & 0xffffffff)) & 0xffffffff
        dr = dr - (1 << 32) if dr >= 1 << 31 else dr
        key = (dq, dr)
        if key not in self.memo:
            y = self.o.k << 32
            self.memo[key] = self.L.mmo_comput_sc(1 << 20, y | (1 << 20), (1 << 20) - dr, y | ((1 << 20) - dq), self.mdx, self.mdy, self.o.bw,
                                                  self.pen_gap, self.pen_skip) if abs(dr) < 1 << 20 and abs(dq) < 1 << 20 else NONE
        return self.memo[key]


def chain_dp(L, o, qlen, x, q, slack=0, low_tie=False, ii_low=False):
    """f, p, events and t (t[j] = the last anchor whose scan marked j, 0 = none) of mg_lchain_dp over anchors sorted by x.  slack and low_tie make a WRONG programme on purpose (a scan that breaks `slack`
    marks late; of equal sums the smaller index; of equal f in the search for max_ii the smaller index): the coverage checks ask that the case table tells them from the right one."""
    n = len(x)
    sc = Scorer(L, o, qlen)
    mdx = sc.mdx
    f, p, t = [0] * n, [-1] * n, [0] * n      # anchor 0 marks nothing, so 0 is free to mean `never`
    events = []
    st, max_ii = 0, -1
    for i in range(n):
        xi, qi, gi = x[i], q[i], x[i] >> 32
        while st < i and (x[st] >> 32 != gi or xi > x[st] + mdx):
            st += 1
        cut = i - st > o.max_iter
        if cut:
            st = i - o.max_iter
        best, best_j, n_skip = o.k, -1, 0
        brk, dec0, touch0, n_valid, tie, ii_tie, rose = None, False, 0, 0, False, False, False
        j = i - 1
        while j >= st:
            s = sc(xi, qi, x[j], q[j])
            if s != NONE:
                n_valid += 1
                s += f[j]
                if s > best or (low_tie and s == best and best_j >= 0):
                    best, best_j = s, j
                    if n_skip > 0:
                        n_skip -= 1
                        touch0 += n_skip == 0
                    else:
                        dec0 |= rose
                else:
                    tie |= s == best and best_j >= 0
                    if t[j] == i:
                        n_skip += 1
                        rose = True
                        if n_skip > o.max_skip + slack:
                            brk = i - 1 - j
                            break
                if p[j] >= 0:
                    t[p[j]] = i
            j -= 1
        end_j = j
        scanned = i - 1 - end_j if brk is None else brk + 1
        far = max_ii >= 0 and (x[max_ii] >> 32 != gi or xi - x[max_ii] > mdx)
        if max_ii < 0 or far:
            max_ii, top = -1, NONE
            for j in range(i - 1, st - 1, -1):
                if f[j] > top or (ii_low and f[j] == top):
                    top, max_ii = f[j], j
                    ii_tie = False
                elif f[j] == top:
                    ii_tie = True
        consulted = max_ii >= 0 and max_ii < end_j
        won = False
        if consulted:
            s = sc(xi, qi, x[max_ii], q[max_ii])
            if s != NONE and best < s + f[max_ii]:
                best, best_j, won = s + f[max_ii], max_ii, True
        f[i], p[i] = best, best_j
        events.append(Event(st, cut, n_valid, brk, dec0, touch0, consulted, won, far, max_ii, scanned, tie, ii_tie))
        if max_ii < 0 or (x[max_ii] >> 32 == gi and xi - x[max_ii] <= mdx and f[max_ii] < best):
            max_ii = i
    return f, p, events, t


def backtrack(o, f, p, first_only=False, late=False):
    """mg_chain_backtrack: candidates f >= min_sc visited in descending (f, index) order; each walks back until it meets an anchor already
    taken or has dropped more than bw below the best point of the walk, and keeps the part up to that best point.  Returns the accepted
    chains (zi, end_i, score, cnt, zf) in visit order, t (1 on every anchor a kept or a rejected walk took), and per visited candidate
    (zi, accepted, ran_into_taken, max_drop_seen)."""
    n = len(f)
    t = [0] * n
    order = sorted((i for i in range(n) if f[i] >= o.min_sc), key=lambda i: (f[i], i), reverse=True)
    chains, visits = [], []
    for zi in order:
        if t[zi]:
            continue
        zf = f[zi]
        i, top_s, top_i, hit, drop = zi, 0, zi, False, 0
        seen = set()
        while True:
            seen.add(i)
            i = p[i]
            s = zf if i < 0 else zf - f[i]
            if s > top_s or (late and s == top_s):      # late: wrong on purpose, like slack above
                top_s, top_i = s, i
            else:
                drop = max(drop, top_s - s)
                if top_s - s > o.bw:
                    break
            if i < 0:
                break
            if t[i] or i in seen:
                hit = True
                break
        cnt, i = 0, zi
        while i != top_i:
            t[i] = 1
            cnt += 1
            i = p[i]
        score = zf if top_i < 0 else zf - f[top_i]
        ok = score >= o.min_sc and cnt >= 1 and cnt >= o.min_cnt
        visits.append((zi, ok, hit, drop, score, cnt))
        if ok:
            chains.append((zi, top_i, score, cnt, zf))
            if first_only:
                break
        # the anchors of a rejected walk stay taken (t = 1), only the list forgets them
    return chains, t, visits


def run(L, o, qlen, x, q):
    f, p, events, _ = chain_dp(L, o, qlen, x, q)
    chains, t, _ = backtrack(o, f, p)
    return Result(f, p, chains, t, len(chains), max([c[2] for c in chains], default=0), events)


# ---- what the block-parallel fills may and must do ------------------------------------------------------------------------------------
def cluster_starts(o, qlen, x):
    """the marks the product puts in bit 31 of q: a new strand / contig, or more than max_dist_x from the anchor before"""
    mdx, _ = dists(o, qlen)
    return [i == 0 or x[i] >> 32 != x[i - 1] >> 32 or (x[i] & 0xffffffff) - (x[i - 1] & 0xffffffff) > mdx for i in range(len(x))]


def par_fill_model(o, qlen, x, q, events, q_cap=1024, rank_cap=128, dirty_cap=64):
    """(applicable, dirty cluster starts): the premise of par_fill_block is broken by an anchor with more than max_skip valid predecessors
    or a cut window; its cluster is dirty.  Not applicable: qlen beyond q_cap, more than rank_cap distinct query positions, more than
    dirty_cap dirty anchors."""
    starts = cluster_starts(o, qlen, x)
    bad = [i for i, e in enumerate(events) if e.n_valid > o.max_skip or e.cut]
    ok = qlen <= q_cap and len(set(q)) <= rank_cap and len(bad) <= dirty_cap
    dirty = set()
    for i in bad:
        while not starts[i]:
            i -= 1
        dirty.add(i)
    return ok, dirty, starts
