#!/usr/bin/env python3
"""Known-answer vectors for the extension stage's aligner (oracle/mm_align.c mma_ksw_extd2), authored by this build - the reference
holds none.  The expected values do NOT come from the code under test: they are computed here by a plain
O(nm) dual-affine-gap dynamic programme written from the recurrence alone (H, E, F, E2, F2 over the full matrix, global start,
free end), so the difference-encoded, anti-diagonal, banded restatement in the oracle is pinned against an independent statement of
what ksw2's extension alignment computes: the end-to-end score, the best score anywhere, the best score with the query consumed
(mqe) and with the target consumed (mte).  usage: make_align_golden.py > align_kat.json

A second set pins the oracle where the device kernel changes path - anti-diagonals of more than 128 and more than 256 cells, targets
beyond 448 and queries beyond 336 bases - at sizes the first set (at most 47 x 63) never reaches.  The recurrence is the same; the row
it depends on is prepared with numpy and the dependency inside a row runs cell by cell as before (plain_matrix).
usage: make_align_golden.py wide > align_kat_wide.json"""
import json
import numpy as np

NEG = -0x40000000


def plain(qs, ts, a, b, amb, q, e, q2, e2):
    def sc(x, y):
        return -amb if (x > 3 or y > 3) else (a if x == y else -b)
    n, m = len(ts), len(qs)
    H = np.full((n + 1, m + 1), NEG, np.int64); E = H.copy(); F = H.copy(); E2 = H.copy(); F2 = H.copy()
    H[0, 0] = 0
    for i in range(1, n + 1):
        H[i, 0] = -min(q + i * e, q2 + i * e2)
    for j in range(1, m + 1):
        H[0, j] = -min(q + j * e, q2 + j * e2)
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            E[i, j] = max(H[i - 1, j] - q, E[i - 1, j]) - e
            E2[i, j] = max(H[i - 1, j] - q2, E2[i - 1, j]) - e2
            F[i, j] = max(H[i, j - 1] - q, F[i, j - 1]) - e
            F2[i, j] = max(H[i, j - 1] - q2, F2[i, j - 1]) - e2
            H[i, j] = max(H[i - 1, j - 1] + sc(ts[i - 1], qs[j - 1]), E[i, j], F[i, j], E2[i, j], F2[i, j])
    H = H[1:, 1:]
    return {"score": int(H[n - 1, m - 1]), "max": max(int(H.max()), 0), "mqe": int(H[:, m - 1].max()), "mte": int(H[n - 1, :].max())}


def plain_matrix(qs, ts, a, b, amb, q, e, q2, e2):
    """plain()'s recurrence a row at a time: what a cell takes from the row above (E, E2, the diagonal) for the whole row at once, what it
    takes from its left neighbour (F, F2) cell by cell.  Returns H without the boundary row and column."""
    n, m = len(ts), len(qs)
    qa, ta = np.asarray(qs, np.int64), np.asarray(ts, np.int64)
    H = np.full((n + 1, m + 1), NEG, np.int64)
    H[0, 0] = 0
    for i in range(1, n + 1):
        H[i, 0] = -min(q + i * e, q2 + i * e2)
    for j in range(1, m + 1):
        H[0, j] = -min(q + j * e, q2 + j * e2)
    E = np.full(m + 1, NEG, np.int64); E2 = E.copy()
    for i in range(1, n + 1):
        E = np.maximum(H[i - 1] - q, E) - e
        E2 = np.maximum(H[i - 1] - q2, E2) - e2
        sc = np.where((ta[i - 1] > 3) | (qa > 3), -amb, np.where(qa == ta[i - 1], a, -b))
        up = np.maximum(np.maximum(H[i - 1, :-1] + sc, E[1:]), E2[1:]).tolist()      # max(diagonal, E, E2) of cells 1..m
        h, f, f2, row = int(H[i, 0]), NEG, NEG, []
        for j in range(m):
            f = max(h - q, f) - e
            f2 = max(h - q2, f2) - e2
            h = max(up[j], f, f2)
            row.append(h)
        H[i, 1:] = row
    return H[1:, 1:]


def summary(H):
    n, m = H.shape
    return {"score": int(H[n - 1, m - 1]), "max": max(int(H.max()), 0), "mqe": int(H[:, m - 1].max()), "mte": int(H[n - 1, :].max())}


def related(ts, m, rng, sub=0.06, indel=0.08):
    out = []
    for c in ts:
        r = rng.random()
        if r < sub:
            out.append(int(rng.integers(0, 4)))
        elif r < sub + indel / 2:
            continue
        elif r < sub + indel:
            out += [int(c), int(rng.integers(0, 4))]
        else:
            out.append(int(c))
    out = out[:m]
    return np.array(out + [int(x) for x in rng.integers(0, 4, m - len(out))])


# (query, target) lengths on both sides of the device kernel's borders
WIDE_SHAPES = [(65, 65), (80, 80), (127, 127), (128, 128), (129, 129), (144, 144), (200, 200), (256, 256), (257, 257), (272, 272), (320, 320), (336, 336),
               (400, 400), (460, 460), (300, 448), (300, 449), (336, 400), (337, 400), (449, 337), (40, 400), (400, 40), (1, 300), (300, 1), (257, 129)]


def main_wide():
    rng = np.random.default_rng(20261018)
    cases = []
    scores = [(2, 8, 1, 12, 2, 24, 1), (2, 4, 1, 4, 2, 24, 1), (1, 4, 1, 6, 2, 26, 1)]
    for it, (m, n) in enumerate(WIDE_SHAPES):
        ts = rng.integers(0, 4, n)
        if it % 4 == 3:
            qs = rng.integers(0, 4, m)
        elif it % 4 == 2:      # a repeat: many cells share the maximum
            unit = rng.integers(0, 4, 5)
            ts = np.array([unit[i % 5] for i in range(n)]); qs = np.array([unit[(i + it) % 5] for i in range(m)])
            qs[rng.integers(0, m, max(1, m // 50))] = 3 - unit[0]
        else:
            qs = related(ts, m, rng)
        if it % 5 == 0:
            qs[int(rng.integers(0, len(qs)))] = 4; ts[int(rng.integers(0, len(ts)))] = 4
        a, b, amb, q, e, q2, e2 = scores[it % 3]
        x = summary(plain_matrix(list(qs), list(ts), a, b, amb, q, e, q2, e2))
        if m * n <= 4096:
            assert x == plain(list(qs), list(ts), a, b, amb, q, e, q2, e2)
        cases.append({"query": "".join("ACGTN"[int(c)] for c in qs), "target": "".join("ACGTN"[int(c)] for c in ts), "a": a, "b": b, "sc_ambi": amb,
                      "q": q, "e": e, "q2": q2, "e2": e2, "expect": x})
    print(json.dumps({"comment": "the same plain dynamic programme at the shapes where the device kernel changes path; sequences as ACGTN = codes 0..4", "cases": cases}))


def main():
    rng = np.random.default_rng(20261003)
    cases = []
    scores = [(2, 8, 1, 12, 2, 24, 1), (2, 4, 1, 4, 2, 24, 1), (1, 4, 1, 6, 2, 26, 1)]      # sr, map-ont, map-hifi
    for it in range(120):
        m, n = int(rng.integers(1, 48)), int(rng.integers(1, 64))
        ts = rng.integers(0, 4, n)
        if it % 3:
            st = int(rng.integers(0, max(1, n - 1)))
            out = []
            for c in ts[st:st + m]:
                r = rng.random()
                if r < 0.06:
                    out.append(int(rng.integers(0, 4)))
                elif r < 0.10:
                    continue
                elif r < 0.14:
                    out += [int(c), int(rng.integers(0, 4))]
                else:
                    out.append(int(c))
            qs = np.array(out[:m] if out else [0])
        else:
            qs = rng.integers(0, 4, m)
        if it % 7 == 0:
            qs[int(rng.integers(0, len(qs)))] = 4
        a, b, amb, q, e, q2, e2 = scores[it % 3]
        cases.append({"query": [int(x) for x in qs], "target": [int(x) for x in ts], "a": a, "b": b, "sc_ambi": amb, "q": q, "e": e, "q2": q2, "e2": e2,
                      "expect": plain(list(qs), list(ts), a, b, amb, q, e, q2, e2)})
    print(json.dumps({"comment": __doc__.split("\n")[0], "cases": cases}))


if __name__ == "__main__":
    import sys
    main_wide() if sys.argv[1:] == ["wide"] else main()
