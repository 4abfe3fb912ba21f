"""Brute force of the low-complexity masking rule (DESIGN.md §7 "Low-complexity masking"), written from the rule alone.

Test infrastructure: plain Python, integers only, nothing shared with the library.

The rule.  Inside a maximal run of ACGTacgt (any other byte, and a record border, ends a run) a run of n bases has n - 2
triplets t_0 .. t_{n-3}.  An interval [i, j], i < j, holds at most W - 2 triplets.  With c_x the number of triplets of code x
in it, r = sum_x c_x (c_x - 1) / 2, l = j - i, its score is r / l.  It is perfect when 10 r > T l and no interval contained
in it scores strictly higher.  The masked bases are the union over all perfect intervals of the bases [i, j + 2] of the run.

For every end j the scores S(i, j) of all admissible starts are counted afresh, from i = j - 1 downwards.  best[i] holds the
largest score of any interval inside [i, j'] for the ends j' seen so far: by definition the maximum over the ends j' <= j of
the maximum over the starts a >= i of S(a, j'), and the inner maximum is the running maximum of the downward count.
Fractions are compared by cross-multiplication.
"""

_CODE = {65: 0, 67: 1, 71: 2, 84: 3, 97: 0, 99: 1, 103: 2, 116: 3}


def _mask_run(codes, W, T, flags, at):
    """codes: the run's bases as 0..3; sets flags[at + p] = 1 for every masked base p of the run"""
    n = len(codes)
    if n < 4:
        return
    trip = [codes[q] * 16 + codes[q + 1] * 4 + codes[q + 2] for q in range(n - 2)]
    m = len(trip)
    best_r = [0] * m
    best_l = [1] * m
    for j in range(1, m):
        lowest = max(0, j - (W - 2) + 1)          # j - i + 1 <= W - 2
        count = [0] * 64
        count[trip[j]] = 1
        r = 0
        run_r, run_l = 0, 1                       # max over starts a >= i of S(a, j)
        first = -1
        for i in range(j - 1, lowest - 1, -1):
            t = trip[i]
            r += count[t]                         # pairs the new triplet forms with its equals inside [i + 1, j]
            count[t] += 1
            l = j - i
            if r * run_l > run_r * l:
                run_r, run_l = r, l
            if run_r * best_l[i] > best_r[i] * run_l:
                best_r[i], best_l[i] = run_r, run_l
            if 10 * r > T * l and r * best_l[i] >= best_r[i] * l:
                first = i                         # perfect; every perfect interval of this end covers bases [i, j + 2]
        if first >= 0:
            for p in range(first, j + 3):
                flags[at + p] = 1


def mask_flags(seq, W=64, T=20):
    """one record -> bytearray of 0 / 1 per base"""
    flags = bytearray(len(seq))
    run, at = [], 0
    for p, ch in enumerate(bytes(seq)):
        c = _CODE.get(ch)
        if c is None:
            _mask_run(run, W, T, flags, at)
            run, at = [], p + 1
        else:
            run.append(c)
    _mask_run(run, W, T, flags, at)
    return flags


def mask_records(records, W=64, T=20, replacement=b"x"):
    """records -> masked records (bytes); replacement None / b"" = soft masking (lower case)"""
    out = []
    for seq in records:
        seq = bytes(seq)
        f = mask_flags(seq, W, T)
        b = bytearray(seq)
        for p, v in enumerate(f):
            if v:
                b[p] = replacement[0] if replacement else b[p] | 0x20
        out.append(bytes(b))
    return out


def intervals(flags):
    """0 / 1 flags -> [[start, end), ...]"""
    out, p, n = [], 0, len(flags)
    while p < n:
        if flags[p]:
            q = p
            while q < n and flags[q]:
                q += 1
            out.append([p, q])
            p = q
        else:
            p += 1
    return out


def by_enumeration(seq, W=64, T=20):
    """The definition with nothing clever at all - every interval against every interval inside it.  O(n W^3): for short inputs,
    to pin the recurrence above."""
    seq = bytes(seq)
    flags = bytearray(len(seq))
    p = 0
    while p < len(seq):
        if seq[p] not in _CODE:
            p += 1
            continue
        q = p
        while q < len(seq) and seq[q] in _CODE:
            q += 1
        codes = [_CODE[c] for c in seq[p:q]]
        trip = [codes[x] * 16 + codes[x + 1] * 4 + codes[x + 2] for x in range(len(codes) - 2)]

        def score(i, j):
            c = {}
            for t in trip[i:j + 1]:
                c[t] = c.get(t, 0) + 1
            return sum(v * (v - 1) // 2 for v in c.values()), j - i

        m = len(trip)
        sc = {(i, j): score(i, j) for i in range(m) for j in range(i + 1, min(m, i + W - 2))}
        for (i, j), (r, l) in sc.items():
            if 10 * r <= T * l:
                continue
            if all(sc[(a, b)][0] * l <= r * sc[(a, b)][1] for a in range(i, j) for b in range(a + 1, j + 1)):
                for x in range(i, j + 3):
                    flags[p + x] = 1
        p = q
    return flags
