"""The lane-wise schemes of csrc/sh_chain.h restated in plain Python, beside the sequential model of tests/chain_ref.py: the scan of
chain_dp_wave / chain_dp_ring, 64 predecessors a step (marks of a chunk written first, prefix maximum, n_skip as a walk reflected at zero,
the break lane, the tie ballot), and the eight-lane split of par_fill_tiled with its pairwise combine.  Each takes the deliberate breaks
the chaining tests are meant to catch as switches, so that tests/test_chain_cases_cpu.py can ask, without a device, that the case table
tells every broken scheme from the right one."""
from tests import chain_ref as R

NONE = R.NONE


def wave_dp(L, c, no_reflect=False, tie_lt=False):
    """f, p of the 64-lane scan; no_reflect drops the reflection term of n_skip, tie_lt shuts the break lane out of the tie ballot"""
    o, qlen = c["o"], c["qlen"]
    x = [int(v) for v in c["x"]]; q = [int(v) for v in c["q"]]
    n = len(x); sc = R.Scorer(L, o, qlen); mdx = sc.mdx
    f = [0]*n; p = [-1]*n; t = [0]*n
    st = 0; max_ii = -1
    for i in range(n):
        while st < i and x[i] > x[st] + mdx: st += 1
        if i - st > o.max_iter: st = i - o.max_iter
        max_f, n_skip, max_j, end_j = o.k, 0, -1, st - 1
        jb = i - 1
        while jb >= st:
            lanes = []
            for l in range(64):
                j = jb - l
                s = NONE
                if j >= st:
                    s = sc(x[i], q[i], x[j], q[j])
                    if s != NONE: s += f[j]
                lanes.append((j, s))
            for j, s in lanes:
                if s != NONE and p[j] >= 0: t[p[j]] = i
            incl = []; run = NONE
            for j, s in lanes:
                run = max(run, s); incl.append(run)
            yl = []; mn = []; y = n_skip; m = 1 << 30; brk = None; vals = []
            for l, (j, s) in enumerate(lanes):
                excl = max(incl[l-1] if l else NONE, max_f)
                has = s != NONE
                new_max = has and s > excl
                inc = has and not new_max and t[j] == i
                y += (1 if inc else 0) - (1 if new_max else 0)
                m = min(m, y)
                val = y if no_reflect else y - (m if m < 0 else 0)
                vals.append(val)
                if brk is None and inc and val > o.max_skip: brk = l
            Lb = brk if brk is not None else 63
            mm = incl[Lb]
            if mm > max_f:
                max_f = mm
                eq = [l for l, (j, s) in enumerate(lanes) if (l < Lb if tie_lt else l <= Lb) and s == mm]
                max_j = jb - eq[0] if eq else jb + 1      # an empty ballot: ffs(0) - 1 = -1
            n_skip = vals[Lb]
            if brk is not None: end_j = jb - Lb; break
            jb -= 64
        far = max_ii >= 0 and x[i] - x[max_ii] > mdx
        if max_ii < 0 or far:
            max_ii, top = -1, NONE
            for j in range(i - 1, st - 1, -1):
                if f[j] > top: top, max_ii = f[j], j
        if max_ii >= 0 and max_ii < end_j:
            s = sc(x[i], q[i], x[max_ii], q[max_ii])
            if s != NONE and max_f < s + f[max_ii]: max_f, max_j = s + f[max_ii], max_ii
        f[i], p[i] = max_f, max_j
        if max_ii < 0 or (x[i] - x[max_ii] <= mdx and f[max_ii] < max_f): max_ii = i
    return f, p

def tiled8(L, c, combine_lt=False):
    """one tile, eight lanes an anchor: per-lane maximum over every eighth predecessor, combined; clean clusters only are compared"""
    o, qlen = c["o"], c["qlen"]
    x = [int(v) for v in c["x"]]; q = [int(v) for v in c["q"]]
    n = len(x); sc = R.Scorer(L, o, qlen)
    starts = R.cluster_starts(o, qlen, x)
    f = [o.k]*n; p = [-1]*n
    order = sorted(range(n), key=lambda i: q[i])
    for i in order:
        if starts[i]: continue
        cs = i
        while not starts[cs]: cs -= 1
        best = []
        for sub in range(8):
            mf, mj = o.k, -1
            j = i - 1 - sub
            while j >= cs:
                s = sc(x[i], q[i], x[j], q[j])
                if s != NONE and q[j] < q[i]:
                    cnd = s + f[j]
                    if cnd > mf: mf, mj = cnd, j
                j -= 8
            best.append((mf, mj))
        lanes = best[:]
        for step in (1, 2, 4):
            new = []
            for l in range(8):
                (mf, mj), (of, oj) = lanes[l], lanes[l ^ step]
                if of > mf or (of == mf and (oj < mj if combine_lt else oj > mj)): mf, mj = of, oj
                new.append((mf, mj))
            lanes = new
        f[i], p[i] = lanes[0]
    return f, p
