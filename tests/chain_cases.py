"""The case table of the chaining DP and backtrack variants (csrc/sh_chain.h), shared by tests/test_chain_cases_cpu.py (the model against
the oracle, and whether the table reaches what it is meant to reach) and tests/test_chain_gpu.py (every device variant against the oracle).

A case is a set of anchors sorted by x (x = strand<<63 | contig<<32 | reference position, q = query position), a query length and the
chaining options.  The shapes are the smallest that reach an edge of one of the variants, not the workload's: the 64-lane chunk of the wave
variants, the ring's 192-anchor window and 256-record capacity, its 8192-bit mark bitmap, the 4096-anchor tile and 256-anchor halo of the
tiled fill, the eight-lane split, the caps of the block fill (1024 query positions, 128 ranks, 64 dirty anchors), TOPBT_MAX.  Two cases are
large because their edge is: `ring_wrap` (mark indices beyond 8192) and `tile_bounds` (clusters at three tile borders).

bt_table() holds DP states (f, p) written by hand for the edges of the backtrack that are hard to reach from anchors.
"""
import functools

import numpy as np

from tests import chain_ref as R

# the chaining fields of the presets (test_chain_cases_cpu.py holds them against the oracle's mmo_preset)
PRESETS = {
    "sr": R.Opt(21, 1, 2, 25, 100, -1, 800, 100, 25, 5000, 0.8, 0.0),
    "map-ont": R.Opt(15, 0, 3, 40, 5000, -1, 0, 500, 25, 5000, 0.8, 0.0),
    "map-hifi": R.Opt(19, 0, 3, 40, 10000, -1, 0, 500, 25, 5000, 0.8, 0.0),
    "lr:hq": R.Opt(19, 0, 3, 40, 10000, -1, 0, 500, 25, 5000, 0.8, 0.0),
}
SR, ONT, HIFI, LRHQ = (PRESETS[n] for n in ("sr", "map-ont", "map-hifi", "lr:hq"))
SRW = SR._replace(max_gap_ref=5000)      # short-read scores with room in x: what most constructions below use (max_dist_x = 5000, max_dist_y = qlen)

SIZES = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 300, 520)
FILLERS = (0, 2, 3, 5, 7, 8, 62, 63, 64, 65, 70, 127, 128, 129, 191, 192, 193, 255, 256, 257, 300)
SKIPS = (0, 1, 2, 25, 61, 62, 63, 64, 126, 127, 128)      # a dense diagonal breaks at scan position max_skip + 1
SHIFTS = (62, 63, 64, 65, 127, 128, 129, 191, 192, 193, 256)
ITERS = (50, 64, 65, 256)

# limits of the variants, restated (csrc/sh_chain.h)
RING_WIN, RING_CAP, RING_TBITS, RING_TMAX_ITER = 192, 256, 8192, 8000
PF_MAX_Q, PF_MAX_RANK, PF_DIRTY_CAP, PF_DIRTY = 1024, 128, 64, 0x7ffffff1
PFT_T, PFT_H = 4096, 256
TOPBT_MAX = 64
SMALL_CAP = 32

DP_VARIANTS = ("seq", "mask", "small", "wave", "ring", "pf_block", "pf_tiled")
DP_CODE = {"none": 0, "seq": 1, "mask": 2, "small": 3, "wave": 4, "ring": 5, "pf_block": 6, "pf_tiled": 7}
BT_VARIANTS = ("small", "mask", "heap", "wave_top", "block_top", "quick")
BT_CODE = {"none": 0, "small": 1, "mask": 2, "heap": 3, "wave_top": 4, "block_top": 5, "quick": 6}


def n_fits(variant, n):
    return n <= {"mask": 64, "small": SMALL_CAP}.get(variant, 1 << 30)


def takes(variant, n, qlen, o, groups=1):
    """whether a DP variant can take a case: its size, the query length and the options decide.  `groups` is a deliberate addition to those
    three: a SliceStore is one strand of one contig, so the variants built on it take a case only if all its anchors share x >> 32 (every
    case outside the `groups` family does).  q < max(qlen, 1024) in every case."""
    if variant == "seq":
        return True
    if variant == "mask":
        return n <= 64 and groups == 1
    if variant == "small":
        return n <= SMALL_CAP and max(qlen, PF_MAX_Q) <= 65536 and o.k * n <= 65535
    if variant == "wave":
        return groups == 1
    if variant == "ring":
        return groups == 1 and o.max_iter <= RING_TMAX_ITER
    if variant == "pf_block":
        return True
    if variant == "pf_tiled":
        return True      # with max_iter < PFT_H it declines by contract: run, and asserted
    raise KeyError(variant)


def bt_takes(variant, n):
    """backtrack_mask holds 64 anchors; backtrack_small looks at every anchor once per candidate and is the product's choice for small n only"""
    return n <= {"mask": 64, "small": 1024}.get(variant, 1 << 30)


def _case(name, fam, o, qlen, rq, group=None):
    """rq: (reference position, query position) in x order; group: x >> 32 per anchor (default 0)"""
    r = np.array([a for a, _ in rq], np.uint64)
    g = np.zeros(len(rq), np.uint64) if group is None else np.array(group, np.uint64)
    x = g << np.uint64(32) | r
    assert np.all(x[1:] >= x[:-1]), name
    q = np.array([b for _, b in rq], np.uint32)
    assert int(q.max()) < max(qlen, PF_MAX_Q), name
    return {"name": name, "fam": fam, "o": o, "qlen": qlen, "x": x, "q": q, "groups": len(set(g.tolist()))}


def _diag(n, gap, r0=1000, q0=0):
    return [(r0 + gap * t, q0 + gap * t) for t in range(n)]


def _tandem(rng, n, n_q, period, copies, q_hi, jitter=2, r0=1000):
    """copies of one set of n_q query positions, `period` apart on the reference: every anchor sees valid predecessors on several diagonals"""
    qs = np.sort(rng.choice(np.arange(1, q_hi), size=min(n_q, q_hi - 1), replace=False))
    rq = [(r0 + c * period + int(u) + int(rng.integers(0, jitter + 1)), int(u)) for c in range(copies) for u in qs]
    rq.sort(key=lambda a: a[0])
    return rq[:n]


def _colinear(rng, n, step, wobble):
    rq, r, q = [], 1000, 5
    for _ in range(n):
        r += int(rng.integers(1, step + 1))
        q += int(rng.integers(1, step + 1))
        rq.append((r + int(rng.integers(-wobble, wobble + 1)), q))
    rq.sort(key=lambda a: a[0])
    return rq


def _fill_dq(m, r, q=1000):
    """m anchors no later anchor with a smaller q can link to (dq <= 0), nor each other (dq = 0, dr = 0)"""
    return [(r, q)] * m


def _fill_dd(m, r, q=0):
    """m anchors far off the diagonal of what follows (dd > bw), and dr = 0 from each other"""
    return [(r, q)] * m


@functools.lru_cache(maxsize=None)
def table():
    T = []
    add = T.append
    # ---- sizes: both sides of the wave chunk, the ring window, the ring capacity and its wrap
    for n in SIZES:
        rng = np.random.default_rng(1000 + n)
        add(_case(f"size_tandem_{n}", "sizes", SRW._replace(max_skip=2), 1024, _tandem(rng, n, 100, 37, 8, 1000)))
        o = (SR, ONT, HIFI, LRHQ)[SIZES.index(n) % 4]
        if o is SR:
            add(_case(f"size_sr_{n}", "sizes", SR, 150, _tandem(rng, n, 60, 11, 12, 150)))
        else:
            rq = _colinear(rng, n, 9, 4)
            add(_case(f"size_long_{n}", "sizes", o, max(b for _, b in rq) + o.k + 1, rq))
    # ---- score edges, two or three anchors each
    E = SR._replace(max_gap_ref=200, bw=200)      # max_dist_x = bw = 200: what is in the window is also within the band
    S5 = SR._replace(skip_scale=0.5)
    O6 = ONT._replace(max_gap_ref=6000)           # max_dist_x = 6000 above max_dist_y = 5000
    C3 = [(958, 8), (979, 29), (1000, 50)]
    for name, o, qlen, rq in (
            # behind the pair a chain C (f = 21, 42, 63), so that the link is worth taking when it is valid: f and p differ across every edge
            ("dq0", SR, 150, C3 + [(1005, 50)]), ("dq1", SR, 150, C3 + [(1005, 51)]),
            ("dq_mdy_sr", SR, 150, [(1000, 0), (1150, 150)]), ("dq_mdy1_sr", SR, 150, [(1000, 0), (1151, 151)]),
            ("dq_mdy_long", O6, 6000, [(1000, 0), (6000, 5000)]), ("dq_mdy1_long", O6, 6000, [(1000, 0), (6001, 5001)]),
            ("dr0", SR, 150, C3 + [(1000, 55)]), ("dr1", SR, 150, C3 + [(1001, 55)]),
            ("dd_bw", SR, 150, C3 + [(1110, 60)]), ("dd_bw1", SR, 150, C3 + [(1111, 60)]),
            ("dd_bw_q", SR, 150, C3 + [(1010, 160)]), ("dd_bw1_q", SR, 150, C3 + [(1010, 161)]),
            ("dg_k", S5, 150, [(1000, 10), (1021, 31)]), ("dg_k1", S5, 150, [(1000, 10), (1022, 32)]),
            ("dg_k_noskip", SR, 150, [(1000, 10), (1021, 31), (1043, 53)]),
            ("win_mdx", E, 150, [(1000, 10), (1200, 190)]), ("win_mdx1", E, 150, [(1000, 10), (1201, 190)]),
            ("win_mdx_3", E, 150, [(1000, 10), (1001, 11), (1201, 190)])):
        add(_case("edge_" + name, "score", o, qlen, rq))
    add(_case("edge_group", "groups", SR, 150, [(1000, 10), (1010, 20)], [0, 1]))
    add(_case("edge_strand", "groups", SR, 150, [(1000, 10), (1005, 15), (1010, 20), (1012, 30)], [3, 3, (1 << 31) | 3, (1 << 31) | 3]))
    rng = np.random.default_rng(77)
    rq = _tandem(rng, 90, 30, 23, 3, 140)
    add(_case("groups_3x30", "groups", SR, 150, rq, [0] * 30 + [1] * 30 + [5] * 30))
    add(_case("groups_9x3", "groups", SR, 150, [(1000 + 3 * (t % 3), 10 + 3 * (t % 3)) for t in range(27)], [t // 3 for t in range(27)]))
    # ---- ties, and scans kept alive by invalid predecessors: two equal predecessors (equal sums: p is the later one), m anchors between
    # them that cannot be linked to.  m = 70 puts them in different 64-chunks, m % 8 on different sub-lanes of the eight-lane split;
    # m >= 192 makes the ring read the earlier one from the arena.
    for m in FILLERS:
        add(_case(f"tie_dq_{m}", "ties", SRW, 1024, [(100, 100)] + _fill_dq(m, 100) + [(100, 100), (150, 150), (160, 160)]))
        add(_case(f"tie_dd_{m}", "ties", SRW, 1024, [(100, 600)] + _fill_dd(m, 100) + [(100, 600), (150, 650), (160, 660)]))
        add(_case(f"long_dq_{m}", "long", SRW, 1024, [(90, 90), (100, 100)] + _fill_dq(m, 100) + [(150, 150)]))
    # ---- n_skip: a dense diagonal (every predecessor valid, each the predecessor of the one before: all marked) breaks at scan position
    # max_skip + 1, and the anchor with exactly max_skip + 1 predecessors does not break
    for s in SKIPS:
        add(_case(f"skip_dense_{s}", "n_skip", SRW._replace(max_skip=s), 1024, _diag(s + 8, 1)))
    # the same break moved along the scan by invalid anchors: [D0..D3] [m fillers] [D4] [D5]; D5 meets D4 (a maximum), the fillers, then D3, D2,
    # D1 marked: with max_skip = 2 the break is at position m + 3, and D0 lies behind it
    for pos in SHIFTS:
        m = pos - 3
        rq = _diag(4, 1) + [(1004 + t, 1000) for t in range(m)] + [(1004 + m, 4 + m), (1005 + m, 5 + m)]
        add(_case(f"skip_shift_{pos}", "n_skip", SRW._replace(max_skip=2), 1024, rq))
    # ---- max_ii: a strong chain; `gap` anchors nothing later can link to; a dense knot 140 off the strong diagonal (outside its band: the knot's
    # scans break and ask max_ii in vain); then three anchors 50 off the strong diagonal and 90 off the knot's: their scan breaks in the knot and
    # only the shortcut reaches the strong chain's end, gap + 12 anchors back - inside the ring's window or, from 190 on, beyond it
    for gap in (20, 150, 178, 179, 180, 181, 190, 260):
        strong = _diag(30, 9, 1000, 10)      # ends at (1261, 271)
        nothing = [(1262 + 2 * t, t % 7) for t in range(gap)]
        r_k = 1262 + 2 * gap
        knot = [(r_k + t, r_k + t - 990 + 140) for t in range(12)]
        tail = [(r_k + 111 + 3 * t, r_k + 111 + 3 * t - 990 + 50) for t in range(3)]
        add(_case(f"maxii_{gap}", "max_ii", SRW._replace(max_skip=2), 1024, strong + nothing + knot + tail))
    # equal f in the search for max_ii: M (f = 156) is max_ii until the knot J starts 301 beyond it; the search over what is left of the window
    # finds u2 and v2 with f = 42 (their predecessors lie outside J's window or band) and must keep the later one, v2.  J4's scan breaks inside J
    # and asks max_ii: v2 is out of its band, u2 would have given 38 against the 25 it has
    M = _diag(10, 15, 1015, 765)
    rq = sorted(M + [(1146, 120)], key=lambda a: a[0]) + [(1238, 10), (1436, 410), (1438, 210)] + [(1451 + t, 407 + t) for t in range(6)]
    add(_case("maxii_tie", "max_ii", SRW._replace(max_gap_ref=300, max_skip=2), 1024, rq))
    # ---- max_iter: anchor 0 is the only valid predecessor; the anchor m later has it as the last of its window, the next one is cut off
    for m in ITERS:
        o = SRW._replace(max_iter=m)
        add(_case(f"iter_{m}", "max_iter", o, 1024, [(100, 100)] + _fill_dq(m - 1, 100) + [(300, 300), (301, 300), (302, 300)]))
        rng = np.random.default_rng(500 + m)
        add(_case(f"iter_tandem_{m}", "max_iter", o._replace(max_skip=1), 1024, _tandem(rng, 300, 90, 17, 6, 1000)))
    # ---- small max_skip, a skip penalty: tandem-like sets, where scans break, maxima come late and max_ii is asked
    for seed in range(24):
        rng = np.random.default_rng(9000 + seed)
        o = SRW._replace(max_skip=seed % 3, skip_scale=(0.0, 0.3)[seed % 2])
        n = (40, 64, 90, 150, 230, 330)[seed % 6]
        add(_case(f"tandem_{seed}", "random", o, 1024, _tandem(rng, n, int(rng.integers(8, 60)), int(rng.integers(3, 45)), int(rng.integers(3, 12)), 1000,
                                                                 jitter=int(rng.integers(0, 5)))))
    for seed in range(16):      # the same at the sizes of the SmallStore
        rng = np.random.default_rng(9200 + seed)
        o = SRW._replace(max_skip=seed % 3)
        add(_case(f"tandem_small_{seed}", "random", o, 1024, _tandem(rng, (32, 27, 31, 20)[seed % 4], int(rng.integers(4, 12)), int(rng.integers(3, 30)), int(rng.integers(3, 9)), 1000,
                                                                       jitter=int(rng.integers(0, 4)))))
    for seed in range(8):
        rng = np.random.default_rng(9500 + seed)
        o = (SR, ONT, HIFI, LRHQ)[seed % 4]
        rq = _colinear(rng, (20, 50, 120, 400)[seed // 2], 14, 25)
        add(_case(f"random_{seed}", "random", o, 150 if o is SR else max(b for _, b in rq) + 20, [(a, b % 150) for a, b in rq] if o is SR else rq))
    # ---- clusters (the block fills): several clusters per read, singletons, the caps
    def clusters(sizes, q_step, gap=20000, q0=0, r_step=None):
        rq, r, q = [], 1000, q0
        for sz in sizes:
            for t in range(sz):
                rq.append((r + (r_step or q_step) * t, q + q_step * t))
            r += gap + sz * (r_step or q_step)
            q += q_step * sz
        return rq
    add(_case("clus_mixed", "clusters", SR, 1000, clusters([1, 5, 1, 1, 20, 3, 26, 1], 7)))
    add(_case("clus_ranks_128", "clusters", SR, 1024, clusters([16] * 8, 7)))
    add(_case("clus_ranks_129", "clusters", SR, 1024, clusters([16] * 8 + [1], 7)))
    add(_case("clus_qlen_1024", "clusters", SR, 1024, clusters([10, 12, 1], 9)))
    add(_case("clus_qlen_1025", "clusters", SR, 1025, clusters([10, 12, 1], 9)))
    add(_case("clus_dirty_64", "clusters", SRW._replace(max_skip=2), 1024, clusters([3, 67, 2], 1, gap=9000)))      # a dense diagonal of L anchors: L - 3 of them dirty
    add(_case("clus_dirty_65", "clusters", SRW._replace(max_skip=2), 1024, clusters([3, 68, 2], 1, gap=9000)))
    add(_case("clus_dirty_two", "clusters", SRW._replace(max_skip=2), 1024, clusters([30, 4, 30, 2], 1, gap=9000)))
    for seed in range(6):      # clean and dirty clusters side by side
        rng = np.random.default_rng(700 + seed)
        rq, r = [], 1000
        for c in range(int(rng.integers(4, 9))):
            kind = int(rng.integers(0, 3))
            q0 = int(rng.integers(0, 60)) * 8
            if kind == 0:
                part = [(r + 8 * t + int(rng.integers(0, 3)), q0 + 8 * t) for t in range(int(rng.integers(1, 22)))]
            elif kind == 1:
                part = [(r + t, q0 + t) for t in range(int(rng.integers(2, 9)))]
            else:
                part = sorted((r + c2 * 13 + 8 * t, q0 + 8 * t) for c2 in range(3) for t in range(int(rng.integers(2, 7))))
            rq += part
            r = max(a for a, _ in part) + 6000 + int(rng.integers(0, 50))
        add(_case(f"clus_random_{seed}", "clusters", SRW._replace(max_skip=2 + 3 * (seed % 2)), 1024, rq))
    # ---- marks beyond the ring's bitmap: tandem-like all the way, so that the marks of anchors past 8192 decide breaks
    rng = np.random.default_rng(4242)
    rq = _tandem(rng, 8320, 120, 97, 71, 1000)
    r = rq[-1][0] + 5      # and behind them a scan that runs 202 anchors back (the ring reads f and p from the arena), then a dense diagonal
    rq += [(r, 100)] + _fill_dq(200, r) + [(r, 100), (r + 50, 150)] + _diag(12, 1, r + 60, 160)
    add(_case("ring_wrap", "large", SRW._replace(max_gap_ref=260, max_skip=2), 1024, rq))
    # ---- the tiled fill's borders: a cluster that starts exactly at anchor 4096; one that spans 8192 from inside the halo; one that spans
    # 12288 from before the halo.  Windows stay short and no anchor has more than max_skip valid predecessors: nothing may be dirty.
    add(_case("tile_bounds", "large", SRW, 1024, _tile_bounds()))
    return T


def _saw(n, r0):
    """n anchors of one cluster, 20 apart on the reference, whose query positions climb by 40 in runs of 20 and start over: only the last
    few anchors of the same run are within the band, so no anchor has many valid predecessors however long the cluster"""
    return [(r0 + 20 * t, 8 * (5 * (t % 20)) + 8) for t in range(n)]


def _tile_bounds():
    rq, r = [], 1000
    def cluster(n):
        nonlocal r
        rq.extend(_saw(n, r))
        r += 20 * n + 20000
    while len(rq) + 23 <= PFT_T:
        cluster(23)
    cluster(PFT_T - len(rq))                 # ends at 4095
    assert len(rq) == PFT_T
    cluster(40)                              # starts exactly at 4096
    while len(rq) + 23 <= 2 * PFT_T - 100:
        cluster(23)
    cluster(2 * PFT_T - 100 - len(rq))
    cluster(300)                             # 8092 .. 8392: starts inside the halo of the third tile, spans 8192
    while len(rq) + 23 <= 3 * PFT_T - 400:
        cluster(23)
    cluster(3 * PFT_T - 400 - len(rq))
    cluster(700)                             # 11888 .. 12588: starts before the halo of the fourth tile, spans 12288
    cluster(23)
    return rq


TILE_STARTS = (PFT_T, 2 * PFT_T - 100, 3 * PFT_T - 400)


def shuffled(c):
    """the anchors of a small case in the order gen_anchors would hand them to the SmallStore: any.  Equal x keep their order (the sort is stable)."""
    rng = np.random.default_rng(len(c["name"]) * 131 + len(c["x"]))
    n = len(c["x"])
    rank = np.zeros(n, np.int64)
    for i in range(1, n):
        rank[i] = rank[i - 1] + (c["x"][i] != c["x"][i - 1])
    perm = rng.permutation(int(rank[-1]) + 1)      # a permutation of the distinct x; equal x stay together and in order
    order = sorted(range(n), key=lambda i: (perm[rank[i]], i))
    return np.array(order)


# ---- DP states by hand: the backtrack's edges -----------------------------------------------------------------------------------------
def _bt(name, o, f, p):
    assert all(-1 <= b < i for i, b in enumerate(p)) and min(f) >= 0, name
    return {"name": name, "o": o, "f": np.array(f, np.int32), "p": np.array(p, np.int32)}


@functools.lru_cache(maxsize=None)
def bt_table():
    T = []
    add = T.append
    o = SR      # bw = 100, min_sc = 25, min_cnt = 2
    # a walk 4 -> 3 -> 2 -> 1 -> 0 -> root whose score falls back by exactly bw, and by bw + 1, below its best point
    add(_bt("drop_bw", o, [50, 200, 100, 250, 300], [-1, 0, 1, 2, 3]))
    add(_bt("drop_bw1", o, [50, 201, 100, 250, 300], [-1, 0, 1, 2, 3]))
    # two walks that share a stem: the second runs into anchors the first took
    add(_bt("taken", o, [21, 42, 63, 80, 84, 100], [-1, 0, 1, 2, 2, 4]))
    add(_bt("taken_deep", o, [21, 42, 63, 84, 105, 90, 120, 70], [-1, 0, 1, 2, 3, 1, 4, 1]))
    # cnt and score on both sides of min_cnt and min_sc
    add(_bt("cnt_1", o, [25], [-1]))
    add(_bt("cnt_2", o, [21, 25], [-1, 0]))
    add(_bt("below_min_sc", o, [21, 24], [-1, 0]))
    add(_bt("sc_24_into_taken", o, [16, 30, 60, 33, 40], [-1, 0, 1, 0, 3]))
    add(_bt("sc_25_into_taken", o, [16, 30, 60, 33, 41], [-1, 0, 1, 0, 3]))
    add(_bt("cnt_3_of_3", ONT, [15, 30, 45], [-1, 0, 1]))
    add(_bt("cnt_2_of_3", ONT, [15, 45], [-1, 0]))
    # the first candidate is rejected (one anchor), the others are kept
    add(_bt("first_rejected", o, [21, 42, 500, 63, 84], [-1, 0, -1, 1, 3]))
    add(_bt("none", o, [21, 22, 23, 24], [-1, 0, 1, 2]))
    # equal f among candidates: (f, index) descending; 64 and 65 two-anchor chains at the top score
    for m in (3, TOPBT_MAX - 1, TOPBT_MAX, TOPBT_MAX + 1, 70):
        add(_bt(f"top_{m}", o, [21, 42] * m, [b for t in range(m) for b in (-1, 2 * t)]))
    add(_bt("top_64_and_less", o, [21, 42] * TOPBT_MAX + [21, 41, 21, 30], [b for t in range(TOPBT_MAX + 2) for b in (-1, 2 * t)]))
    # the walk's score stands still at its best point (f equal on two steps), then drops: the kept part ends at the FIRST of the two
    add(_bt("plateau", o, [250, 100, 100, 250, 300], [-1, 0, 1, 2, 3]))
    add(_bt("plateau_root", o, [0, 60, 60, 100], [-1, 0, 1, 2]))
    # random forests
    for seed in range(12):
        rng = np.random.default_rng(3000 + seed)
        n = (20, 64, 65, 200, 300, 600)[seed % 6]
        f, p = [], []
        for i in range(n):
            b = int(rng.integers(-1, i)) if i and rng.random() < 0.9 else -1
            b = max(b, i - 1 - int(rng.integers(0, 6))) if b >= 0 else b
            f.append(max(0, (f[b] if b >= 0 else 21) + int(rng.integers(-60, 45))))
            p.append(b)
        add(_bt(f"forest_{seed}", (SR, ONT)[seed % 2], f, p))
    return T


# ---- the three voices on a case --------------------------------------------------------------------------------------------------------
def oracle_opts(O, o):
    oo = O.preset("sr")
    oo.k, oo.is_sr, oo.min_cnt, oo.min_chain_score, oo.max_gap, oo.max_gap_ref, oo.max_frag_len = o.k, o.is_sr, o.min_cnt, o.min_sc, o.max_gap, o.max_gap_ref, o.max_frag_len
    oo.bw, oo.max_chain_skip, oo.max_chain_iter, oo.chain_gap_scale, oo.chain_skip_scale = o.bw, o.max_skip, o.max_iter, o.gap_scale, o.skip_scale
    return oo


_ORACLE, _MODEL = {}, {}


def oracle_case(O, c):
    """(f, p, chains) of mmo_chain_arrays, computed once"""
    if c["name"] not in _ORACLE:
        f, p, chains = O.chain_arrays(oracle_opts(O, c["o"]), c["o"].k, c["qlen"], c["x"], c["q"])
        _ORACLE[c["name"]] = (f, p, chains)
    return _ORACLE[c["name"]]


def model_case(O, c):
    """the model's Result, computed once"""
    if c["name"] not in _MODEL:
        _MODEL[c["name"]] = R.run(O.lib(), c["o"], c["qlen"], [int(v) for v in c["x"]], [int(v) for v in c["q"]])
    return _MODEL[c["name"]]
