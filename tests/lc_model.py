"""A plain model of what k_local_cluster (csrc/sh_classify.hip) may decide for one read: the kernel's argument
restated read by read in Python integers and numpy, with np.searchsorted where the kernel searches a list and the oracle's mg_lchain_dp
(oracle.chain_arrays) where it chains.  Inputs: the oracle's sketch of the read, the index as its dump() gives it (key, count, positions),
the read's bases and the contigs (for the middle check).  tests/test_lc_cases_cpu.py holds a DECIDED of this model against the oracle's
flag; tests/test_local_cluster_gpu.py holds the kernel against the model, outcome by outcome.

The outcomes are the kernel's reasons (Counters::lc_why) plus NOT_LISTED (the front end does not route the read to the repeat list) and
SCORE_TIE: K's two best chains score the same, the winner hangs on chain_z's hash, and the model predicts nothing."""
from collections import namedtuple

import numpy as np

NOT_LISTED, N_SEED, NO_SINGLETON, HIGH_SEED, APART, WINDOW, K_SIZE, MARGIN, LEMMA, DECIDED, DECIDED_FILTERED, SCORE_TIE = (
    "NOT_LISTED", "N_SEED", "NO_SINGLETON", "HIGH_SEED", "APART", "WINDOW", "K_SIZE", "MARGIN", "LEMMA", "DECIDED", "DECIDED_FILTERED", "SCORE_TIE")
OUTCOMES = (NOT_LISTED, N_SEED, NO_SINGLETON, HIGH_SEED, APART, WINDOW, K_SIZE, MARGIN, LEMMA, DECIDED, DECIDED_FILTERED)
# Counters::lc_why, in the order of the kernel's enum
LC_WHY = ("TRIED", NO_SINGLETON, HIGH_SEED, APART, WINDOW, K_SIZE, MARGIN, LEMMA, DECIDED, DECIDED_FILTERED, N_SEED)
K2_CAP, SEED_CAP = 32, 192      # anchors a read may give and stay on the LDS path; seed records a read may have and stay off the re-sketch path
OCC_CAP, MAX_GROWTHS, K_MIN, K_MAX = 16, 3, 2, 64
U32 = 0xffffffff

# what the model says of one read.  K: the anchors (x, q) sorted by x; detail: the quantities the case table places its edges by
Result = namedtuple("Result", "outcome K u_out fast top_score rounds detail")


class Table:
    """the index dump as numpy: hash -> its occurrence list, ascending"""

    def __init__(self, keys, cnt, pos):
        assert np.all(keys[1:] > keys[:-1])
        self.keys, self.cnt = keys, cnt.astype(np.int64)
        self.start = np.concatenate(([0], np.cumsum(self.cnt)))
        grp = np.repeat(np.arange(len(keys)), self.cnt)
        self.pos = pos[np.lexsort((pos, grp))]

    def find(self, h):
        i = int(np.searchsorted(self.keys, h))
        if i == len(self.keys) or self.keys[i] != h:
            return None
        return self.pos[self.start[i]:self.start[i + 1]]


def max_dist_x(o, qlen):
    m = o.max_gap_ref if o.max_gap_ref > 0 else max(o.max_frag_len - qlen, o.max_gap) if o.max_frag_len > 0 else o.max_gap
    return max(m, o.bw)


def max_dist_y(o, qlen):
    return max(max(qlen, o.max_gap) if o.is_sr else o.max_gap, o.bw)


def lemma_premises(o):
    """(ext_s1, ext_lemma) as fill_chain_params settles them with no switch set"""
    both = o.a > 0 and o.b > 0 and o.a * o.k >= o.min_dp_max and 2 * o.k >= o.min_chain_score and o.max_clip_ratio >= 1.0 and o.zdrop >= 0
    return bool(o.is_sr and (o.flags & 1) and both and o.chain_skip_scale == 0.0 and o.min_cnt <= 2 and o.bw >= 0), bool(o.is_sr and (o.flags & 1) and both)


def anchor(pw, y, qlen, k):
    """(x, q) of the occurrence pw = rid << 32 | pos << 1 | strand of a seed at y = qpos << 1 | strand"""
    pw, y = int(pw), int(y)
    if (pw & 1) == (y & 1):
        return (pw >> 32) << 32 | (pw & U32) >> 1, y >> 1
    return 1 << 63 | (pw >> 32) << 32 | (pw & U32) >> 1, qlen - ((y >> 1) + 1 - k) - 1


def seeds_of(O, o, table, read):
    """(minimizers, [(occurrence list, y)] of those the index holds, in query order)"""
    x, y = O.sketch(bytes(read), o.w, o.k)
    out = []
    for h, yy in zip(x >> np.uint64(8), y & np.uint64(U32)):
        lst = table.find(h)
        if lst is not None:
            out.append((lst, int(yy)))
    return len(x), out


def listed(o, n_mini, seeds):
    """the read kernel's routing: the repeat list takes a read with a seed above mid_occ or more than K2_CAP anchors"""
    q_occ_max = o.mid_occ if o.q_occ_frac > 0 else 1 << 32
    if not seeds or len(seeds) > SEED_CAP or n_mini > q_occ_max:
        return False
    occ = [len(l) for l, _ in seeds]
    return max(occ) > o.mid_occ or sum(occ) > K2_CAP


NT4 = np.full(256, 4, np.int64)
for _i, _c in enumerate(b"ACGT"):
    NT4[_c] = NT4[_c + 32] = _i


def middle_max_drop(o, contigs, read, rid, rev, qs, qe, rs):
    """mm_test_zdrop over the ungapped stretch: query [qs, qe) on strand rev against contig rid from rs on; the largest drop of the running score"""
    amb = -o.sc_ambi if o.sc_ambi > 0 else o.sc_ambi
    qlen, s, top, drop = len(read), 0, None, 0
    for j in range(qe - qs):
        qi = qs + j
        cq = int(NT4[read[qlen - 1 - qi if rev else qi]])
        if rev and cq < 4:
            cq = 3 - cq
        ct = int(NT4[contigs[rid][rs + j]])
        s += amb if cq > 3 or ct > 3 else o.a if cq == ct else -o.b
        top = s if top is None or s > top else top
        drop = max(drop, top - s)
    return drop


def chain_lemma(o, unc_max, x, q, p, zi, end_i):
    """mm_max_stretch over the chain zi -> end_i walked backwards, and the test on it: (code, (q_first, q_last, r_first)).  Code 1: the
    region passes mm_filter_regs from its k-mers alone; 2: it does if the stretch shows no z-drop; 0: unknown."""
    k = o.k
    run = [k, 0, zi, zi]      # score, bases outside the k-mers, first, last
    best = [-1, 0, zi, zi]
    i = zi
    while p[i] != end_i:
        j = p[i]
        lr, lq = (x[i] & U32) - (x[j] & U32), q[i] - q[j]
        if lq == lr:
            run[0] += min(lq, k); run[1] += max(lq - k, 0); run[2] = j
        else:
            if run[0] >= best[0]:      # of equal runs the earlier one
                best = list(run)
            run = [k, 0, j, j]
        i = j
    if run[0] >= best[0]:
        best = list(run)
    qf, ql = q[best[2]], q[best[3]]
    at = (qf, ql, x[best[2]] & U32)
    if not (best[0] >= o.min_chain_score and ql - qf >= k):
        return 0, at
    return (1 if best[1] <= unc_max else 2), at


def decide(O, o, table, contigs, read):
    """the outcome of k_local_cluster for `read` (bytes) under the oracle options o"""
    read = bytes(read)
    qlen, k = len(read), o.k
    ext_s1, ext_lemma = lemma_premises(o)
    assert ext_lemma and o.mid_occ > 0
    unc_max = o.zdrop // o.b
    d = {}

    def res(outcome, K=(), u_out=0, fast=False, top=0, rounds=0):
        return Result(outcome, list(K), u_out, fast, top, rounds, d)

    n_mini, seeds = seeds_of(O, o, table, read)
    d["n_seed"] = len(seeds)
    if not listed(o, n_mini, seeds):
        return res(NOT_LISTED)
    if not 2 <= len(seeds) <= 64:
        return res(N_SEED)
    occ = [len(l) for l, _ in seeds]
    high = [n > o.mid_occ for n in occ]
    single = [n == 1 and not hi_ for n, hi_ in zip(occ, high)]
    if not any(single):
        return res(NO_SINGLETON)
    d["any_high"] = any(high)
    if any(high) and o.occ_dist > 0 and o.max_max_occ > o.mid_occ and int(qlen / o.occ_dist + .499) > 0:
        return res(HIGH_SEED)      # a streak of mm_seed_select may keep a seed above mid_occ
    sx = [anchor(l[0], y, qlen, k) if s else None for (l, y), s in zip(seeds, single)]
    hiw = next(a for a in sx if a)[0] >> 32
    s_in = [a is not None and a[0] >> 32 == hiw for a in sx]      # singletons of another contig or strand lie outside K
    lo, hi = min(a[0] & U32 for a, s in zip(sx, s_in) if s), max(a[0] & U32 for a, s in zip(sx, s_in) if s)
    mdx = max_dist_x(o, qlen)
    d["apart"] = hi - lo
    d["n_single_in"], d["n_single_out"] = sum(s_in), sum(single) - sum(s_in)
    sq = sorted(a[1] for a, s in zip(sx, s_in) if s)      # what the singletons cover by themselves, were they one co-diagonal run
    d["single_cov"] = k + sum(min(b - a, k) for a, b in zip(sq, sq[1:]))
    if hi - lo > 4 * mdx:
        return res(APART)
    rid, rel = hiw & 0x7fffffff, hiw >> 31
    rounds, cap_seen = 0, 0
    while True:
        rounds += 1
        wlo, whi = max(lo - mdx, 0), min(hi + mdx, U32)
        nlo, nhi = lo, hi
        inwin = []
        for (lst, y), s, hi_ in zip(seeds, s_in, high):
            if len(lst) < 2 or hi_:
                inwin.append(None)
                continue
            i0 = np.searchsorted(lst, np.uint64(rid << 32 | wlo << 1), "left")
            i1 = np.searchsorted(lst, np.uint64(rid << 32 | whi << 1 | 1), "right")
            c = [int(pw) for pw in lst[i0:i1] if ((int(pw) & 1) != (y & 1)) == (rel != 0)]
            inwin.append(c)
            for pw in c:
                nlo, nhi = min(nlo, (pw & U32) >> 1), max(nhi, (pw & U32) >> 1)
        cap_seen = max([cap_seen] + [len(c) for c in inwin if c is not None])
        # an occurrence that sits exactly on the window's lower key, where `<` and `<=` of a lower bound part: (round, list length, index in the list)
        d.setdefault("on_lower_key", []).extend((rounds, len(lst), int(np.searchsorted(lst, np.uint64(rid << 32 | wlo << 1), "left")))
                                                 for (lst, y), c in zip(seeds, inwin) if c and (rid << 32 | wlo << 1) in c)
        d["cap"], d["rounds"] = cap_seen, rounds
        if cap_seen > OCC_CAP:
            d["window"] = "cap"
            return res(WINDOW, rounds=rounds)
        if (nlo, nhi) == (lo, hi):
            break
        if rounds == MAX_GROWTHS + 1:
            d["window"] = "rounds"
            return res(WINDOW, rounds=rounds)
        lo, hi = nlo, nhi
    d["wlo"], d["whi"], d["rid"] = wlo, whi, rid
    c_l = [1 if s else (len(c) if c is not None else 0) for s, c in zip(s_in, inwin)]
    n_k = sum(c_l)
    d["n_k"] = n_k
    if not K_MIN <= n_k <= K_MAX:
        return res(K_SIZE, rounds=rounds)
    K = []
    for (lst, y), s, a, c in zip(seeds, s_in, sx, inwin):
        K += [a] if s else [anchor(pw, y, qlen, k) for pw in (c or [])]
    K.sort(key=lambda a: a[0])      # stable: generation order among equal x
    X, Q = [a[0] for a in K], [a[1] for a in K]
    d["dup_x"] = len(set(X)) < len(X)
    starts = [i for i in range(n_k) if i == 0 or X[i] >> 32 != X[i - 1] >> 32 or (X[i] & U32) - (X[i - 1] & U32) > mdx]
    d["clusters"] = [b - a for a, b in zip(starts, starts[1:] + [n_k])]
    # U_out: the query bases under the k-mers of the seeds with an occurrence outside K, in query order
    u_out, prev_en = 0, None
    for (lst, y), n, c, hi_ in zip(seeds, occ, c_l, high):
        if hi_ or n <= c:
            continue
        en = (y >> 1) + 1
        st = en - k
        u_out += en - (prev_en if prev_en is not None and prev_en > st else st)
        prev_en = en
    d["u_out"] = u_out
    decided = DECIDED_FILTERED if any(high) else DECIDED
    outcome, code, at = LEMMA, 0, None
    # one cluster of co-diagonal anchors at most min(max_dist_x, max_dist_y) apart: the chain is K, no DP
    dq = [Q[i] - Q[i - 1] for i in range(1, n_k)]
    fast = bool(ext_s1 and len(starts) == 1 and n_k >= o.min_cnt and all((X[i] & U32) - Q[i] == (X[0] & U32) - Q[0] for i in range(n_k))
                and all(0 < g <= min(mdx, max_dist_y(o, qlen)) for g in dq))
    d["codiagonal"] = fast
    top = 0
    if fast:
        covered, unc = k + sum(min(g, k) for g in dq), sum(max(g - k, 0) for g in dq)
        d.update(covered=covered, unc=unc, span=Q[-1] - Q[0], margin=covered - u_out)
        top = covered
        if covered > u_out and Q[-1] - Q[0] >= k and covered >= o.min_chain_score:
            code, at = (1 if unc <= unc_max else 2), (Q[0], Q[-1], X[0] & U32)
        else:
            fast = False
            if covered <= u_out:
                outcome = MARGIN
    if not fast:
        chains = []      # (score, cluster base, zi, end_i, p)
        for b, n in zip(starts, d["clusters"]):
            if n >= 2:
                f, p, ch = O.chain_arrays(o, k, qlen, np.array(X[b:b + n], np.uint64), np.array(Q[b:b + n], np.uint32))
                chains += [(c[2], b, c[0], c[1], p) for c in ch]
        d["n_chain"] = len(chains)
        if chains:
            top = max(c[0] for c in chains)
            best = [c for c in chains if c[0] == top]
            d["margin_general"] = top - u_out
            if len(best) > 1 or d["dup_x"]:
                return res(SCORE_TIE, K, u_out, False, top, rounds)
            if top <= u_out:
                outcome = MARGIN
            else:
                _, b, zi, end_i, p = best[0]
                d["best_base"] = b
                code, at = chain_lemma(o, unc_max, X[b:], Q[b:], [int(v) for v in p], zi, end_i)
    d["code"] = code
    if code == 2:
        qf, ql, rf = at
        d["mid_drop"] = middle_max_drop(o, contigs, read, rid, rel, qf + 1 - k, ql + 1, rf + 1 - k)
    if code == 1 or (code == 2 and d["mid_drop"] <= o.zdrop):
        outcome = decided
    return res(outcome, K, u_out, fast, top, rounds)
