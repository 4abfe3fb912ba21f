"""The case table of the long join (sh_dbg_long_join, csrc/sh_dbg_long.hip): hand-made anchor sets that sit on both sides of each premise of
lr_rmq_fill / lr_coop / the backtracks / lr_sort in csrc/sh_long.h.  tests/test_long_join_cases_cpu.py checks, with the oracle and the plain model
(tests/long_join_ref.py) alone, that each family really reaches the edge it is named for; tests/test_long_join_gpu.py runs the device code on it.

A case is a dict: name, fam, x (uint64: strand << 63 | contig << 32 | ref pos, ascending), q (query positions), o (the options, Opt), and
per family: cuts (runs), f_in / p_in (backtrack).  Shapes are the smallest that reach the edge: the largest case has about 8 400 anchors."""
import functools

import numpy as np

K = 15
PEN_GAP = float(np.float32(0.8 * 0.01 * K))      # map-ont: chain_gap_scale 0.8, k 15
TCAP_OF = {1024: 1664, 4096: 1792}               # nodes of the LDS tree beside each TREE ring


class Opt(dict):
    """the options a case runs with (map-ont's unless overridden)"""
    BASE = dict(k=K, max_gap=5000, bw_long=20000, max_skip=25, inner=1000, cap=100000, pen_gap=PEN_GAP, pen_skip=0.0, min_cnt=3, min_sc=40,
                coop_min=1, coop_run=2, max_drop=20000, cap_u=1 << 20)

    def __init__(self, **kw):
        super().__init__(Opt.BASE); self.update(kw)


def _case(name, fam, x, q, o=None, **kw):
    x, q = np.asarray(x, np.uint64), np.asarray(q, np.int64)
    assert len(x) == len(q) and len(x) >= 1 and np.all(x[1:] >= x[:-1]) and np.all(q >= 0), name
    c = {"name": name, "fam": fam, "x": x, "q": q.astype(np.uint64), "o": o or Opt()}
    c.update(kw)
    return c


def y_of(c):
    return c["q"] | np.uint64(c["o"]["k"] << 32)


def _line(n, x0, q0, step=20, qstep=None):
    i = np.arange(n, dtype=np.int64)
    return x0 + step * i, q0 + (step if qstep is None else qstep) * i


def _cat(*parts):
    return np.concatenate([np.asarray(p[0]).astype(np.uint64) for p in parts]), np.concatenate([np.asarray(p[1], np.int64) for p in parts])


def _clutter(c, x0, q_top, xstep=2):
    """c anchors that chain with nothing before them: x ascending, y descending from q_top (x + y distinct when xstep != 1)"""
    i = np.arange(c, dtype=np.int64)
    return x0 + xstep * i, q_top - i


def _noisy(rng, n, x0=1000, spread=40, jitter=30, off_frac=0.2, off=3000):
    x = np.sort(rng.integers(x0, x0 + spread * n, n))
    q = (x - x0 + 4000 + rng.integers(-jitter, jitter + 1, n) + np.where(rng.random(n) < off_frac, rng.integers(-off, off, n), 0)).clip(K, None)
    return x, q


def _reach(h, c, tail=3, inner=100, first="high", **okw):
    """ring depth: a high-scoring collinear run of h anchors and c anchors of clutter (either first), then an anchor collinear with the run's
    end that reaches back over the clutter, then `tail` more"""
    q_top = c + 200
    hx0, hq0 = 100000, q_top + 1000
    if first == "high":
        H = _line(h, hx0, hq0, 15); C = _clutter(c, H[0][-1] + 10, q_top)
        far = C[0][-1] + 100 - H[0][-1]
        R = _line(1 + tail, H[0][-1] + far, H[1][-1] + far, 15)
        return _cat(H, C, R), Opt(inner=inner, **okw)
    C = _clutter(c, hx0, q_top); H = _line(h, C[0][-1] + 10, hq0, 15)
    R = _line(1 + tail, H[0][-1] + 300, H[1][-1] + 300, 15)
    return _cat(C, H, R), Opt(inner=inner, **okw)


# the three-anchor mirror: the third anchor sees the first two at equal priority (equal f, equal x + y) and mirrored gaps
def _mirror(xc, qc, gap, near=20):
    return [xc - gap - near, xc - near, xc], [qc - near, qc - gap - near, qc]


def _tie_improved(xc=10000, qc=5000):
    """two collinear runs of ten end mirrored 1000 off the diagonal of (xc, qc) (accepted, one score, none exact); a run of five ends 15 before it:
    its priority is worse and its score better - the tie of the class that the inner scan makes harmless"""
    h1 = _line(10, xc - 1020 - 135, qc - 20 - 135, 15); h2 = _line(10, xc - 20 - 135, qc - 1020 - 135, 15); d = _line(5, xc - 75, qc - 75, 15)
    x, q = _cat(h1, h2, d, ([xc], [qc]))
    o = np.argsort(x, kind="stable")
    return x[o], q[o]


def _tie_matters(xc=10000, qc=5000, clutter=0):
    """two runs of ten end mirrored 500 off the diagonal: accepted, one score, and the inner scan finds nothing better; `clutter` anchors that
    chain with nothing lie between the two run ends in x, so that the tied anchors are that many anchors apart"""
    h1 = _line(10, xc - 520 - 135, qc - 20 - 135, 15); h2 = _line(10, xc - 20 - 135, qc - 520 - 135, 15)
    parts = [h1, h2, ([xc], [qc])]
    if clutter:
        assert clutter <= 330
        parts.append((xc - 510 + np.arange(clutter), qc - 3000 - np.arange(clutter)))
    x, q = _cat(*parts)
    o = np.argsort(x, kind="stable")
    return x[o], q[o]


def _shift(xq, dx, dq=0, hi=0):
    return (np.asarray(xq[0]).astype(np.uint64) + np.uint64(dx)) | np.uint64(hi << 32), np.asarray(xq[1], np.int64) + dq


@functools.lru_cache(maxsize=None)
def join_cases():
    rng = np.random.default_rng(20240611)
    T = []
    add = lambda *a, **k: T.append(_case(*a, **k))
    # ---- block edges: block completion and the final store of the incomplete block
    for n in (1, 2, 63, 64, 65, 128, 129):
        add(f"line{n}", "block", *_line(n, 1000, 500))
    # ---- same-x groups
    for g in (1, 2, 64, 65, 191, 192):
        pre = _line(5, 1000, 3000); grp = (np.full(g, 2000), 500 + 20 * np.arange(g)); post = _line(4, 2020, 500 + 20 * g)
        add(f"samex{g}", "samex", *_cat(pre, grp, post))
    add("samex_at0", "samex", [1000, 1000, 1000, 1010, 1030], [700, 720, 740, 700, 760])      # a later anchor with anchor 0's y: the (q_i, 0) key bound
    # ---- ring depth: the scored anchor in the block being filled, in a completed block of the ring, behind the ring
    for name, h, c, kw in (("reach_new", 80, 10, {}), ("reach_ring", 80, 100, {}), ("reach_old", 80, 400, {}), ("reach_near447", 80, 446, {}),
                           ("reach_far448", 80, 447, {}), ("reach_pml", 80, 400, {"first": "clutter"}), ("reach_old65", 80, 4500, {}),
                           ("reach_old_4096", 80, 4000, {}), ("reach_near4031", 80, 4030, {}), ("reach_far4032", 80, 4031, {}),
                           ("reach_pml_4096", 80, 4000, {"first": "clutter"}), ("reach_old65_4096", 80, 8200, {})):
        (x, q), o = _reach(h, c, **kw)
        add(name, "ring", x, q, o)
    # ---- trim
    small = dict(max_gap=50, bw_long=40, inner=30)
    add("dist_at", "trim", [1000, 1050], [500, 545], Opt(**small))
    add("dist_past", "trim", [1000, 1051], [500, 545], Opt(**small))
    add("leave100", "trim", *_cat(_line(100, 1000, 500, 1), _line(5, 1000 + 99 + 4990, 500 + 99 + 4990, 1)), Opt(max_gap=5000, bw_long=100))
    two = _line(40, 1000, 500)
    add("strand", "trim", *_cat(two, _shift(_line(40, 1400, 900), 0, hi=1 << 31)))
    add("contig", "trim", *_cat(two, _shift(_line(40, 1400, 900), 0, hi=3)))
    add("gap_lt_bw", "trim", *_noisy(rng, 200), Opt(max_gap=300, bw_long=2000))
    add("gap_gt_bw", "trim", *_noisy(rng, 200), Opt(max_gap=2000, bw_long=300))
    (x, q), o = _reach(80, 700, cap=600)
    add("cap_trims", "trim", x, q, o)
    (x, q), o = _reach(80, 700, cap=511)
    add("cap_below_ring", "trim", x, q, o)
    (x, q), o = _reach(80, 700)
    add("cap_ample", "trim", x, q, o)
    # ---- the inner window's list
    add("desc130", "inner", *_clutter(130, 1000, 900, 3))                                     # every insertion at the head, shifting 0 .. 129 entries
    add("prefix", "inner", *_line(100, 1000, 500), Opt(inner=200))
    # 101 anchors leave at once from the TOP of the (y, index) list; the arriving anchor is collinear with the oldest that stays (anchor 150, exactly
    # `inner` bases back), which only the inner scan can find
    add("compact", "inner", *_cat(_clutter(300, 1000, 2000, 3), _line(30, 1450 + 750, 1850 + 750, 5)), Opt(inner=750))
    add("wrap", "inner", *_line(4300, 1000, 500), Opt(inner=200))
    for nr in (512, 1024, 4096):
        for d in (2, 1):
            add(f"inner{nr}_{nr - d + 1}", "inner", *_line(nr + 200, 1000, 500, 1), Opt(inner=nr - d))      # windows of nr - 1 and nr anchors
    for nm, inn in (("inner0", 0), ("inner_neg", -5), ("inner_big", 50000)):
        add(nm, "inner", *_noisy(rng, 220), Opt(inner=inn))
    dense = lambda n: _noisy(rng, n, spread=2, jitter=120, off_frac=0.0)
    add("scan1", "inner", *dense(60), Opt(max_skip=1000, inner=400))
    add("scan3", "inner", *dense(400), Opt(max_skip=1000, inner=400))
    add("skip_first", "inner", *dense(400), Opt(max_skip=3, inner=400))
    add("skip_later", "inner", *dense(400), Opt(max_skip=70, inner=400))
    add("skip0", "inner", *dense(300), Opt(max_skip=0, inner=400))
    # ---- scoring edges
    add("q0", "score", [1000, 1010, 1030], [0, 0, 20])
    add("exact", "score", *_line(20, 1000, 500, 15))
    pre = _line(10, 1000, 500, 15)
    sm = Opt(max_gap=50, bw_long=40, inner=30)
    add("width_at", "score", *_cat(pre, ([1135 + 45], [635 + 5])), sm)
    add("width_past", "score", *_cat(pre, ([1135 + 46], [635 + 5])), sm)
    add("equal_score", "score", [1000, 1010, 1024, 1040], [500, 514, 510, 540], Opt(max_gap=500, bw_long=400, inner=100))
    # ---- ties
    add("mirror", "tie", [1000, 1100, 1200], [600, 500, 700])                                 # nothing accepted
    add("mirror20", "tie", [1000, 1020, 1040], [600, 580, 620])                               # both accepted, one score: matters
    add("tie_improved", "tie", *_tie_improved())
    add("tie_matters", "tie", *_tie_matters())
    add("tie_far", "tie", *_tie_matters(clutter=330))                                         # the tied anchors 340 apart: one behind the 512-ring
    a, b = _tie_matters(), _tie_matters(13000, 8000)
    add("tie_twice", "tie", *_cat(a, b))                                                      # one stretch, a second tie after one that matters
    far = 30000
    add("tie_after_empty", "tie", *_cat(_line(50, 1000, 500), _shift(_tie_matters(), far + 2000, 0)))
    add("tie_at_third", "tie", *_cat(_line(50, 1000, 500), ([40000, 40020, 40040], [600, 580, 620])))
    add("tie_free_tie", "tie", *_cat(_tie_matters(), _shift(_line(80, 1000, 500), 40000), _shift(_tie_matters(), 80000)))
    for nr in (1024, 4096):
        for over in (0, 1):
            n_run = TCAP_OF[nr] + 1 + over - 3
            add(f"tree{nr}_{'over' if over else 'fits'}", "tie", *_cat(([1000, 1020, 1040], [600, 580, 620]), _line(n_run, 1100, 700, 1)))
    add("tree1024_no_tie", "tie", *_cat(([1000, 1020, 1040], [600, 581, 620]), _line(TCAP_OF[1024] - 1, 1100, 700, 1)))
    # ---- runs: stretches that lr_coop cuts apart
    blocks = [_noisy(rng, 64), _noisy(rng, 70), _tie_matters(), _noisy(rng, 200), _line(129, 1000, 500)]
    for m in (2, 3, 4, 5):
        parts = [_shift(blocks[j], 30000 * j, 0, hi=(2 if j >= 3 else 0)) for j in range(m)]      # x jumps beyond max_dist; the fourth starts another contig
        x, q = _cat(*parts)
        starts = np.cumsum([len(p[0]) for p in parts])[:-1].tolist()
        add(f"runs{m}_all", "runs", x, q, cuts=starts)
        if m >= 3: add(f"runs{m}_some", "runs", x, q, cuts=starts[1::2])
    # a run whose first anchor S shares its y with a later anchor A of the run: the key bound (q_i, 0) means anchor 0 of the WHOLE array, not of
    # the run; taken for a candidate, S would beat the collinear C on priority and hide it (C lies outside the inner window)
    xa, ya = 60000, 9000
    add("runs_key0", "runs", *_cat(_line(70, 1000, 500), ([xa - 150, xa - 100, xa, xa + 15], [ya, ya - 100, ya, ya + 15])), Opt(inner=30), cuts=[70])
    return T



@functools.lru_cache(maxsize=None)
def backtrack_cases():
    """(name, f, p, options): chaining state made by hand for lr_backtrack0 / lr_backtrack_wave"""
    B = []

    def chain(n, idx, f0=15, step=15, base_f=15):
        f = np.full(n, base_f, np.int32); p = np.full(n, -1, np.int32)
        for k, i in enumerate(idx):
            f[i] = f0 + step * k
            if k: p[i] = idx[k - 1]
        return f, p
    o = Opt(min_cnt=1, min_sc=20)
    B.append(("hops", *chain(3300, [0, 36, 100, 163, 228, 3228, 3229]), o))                   # predecessors 36, 64, 63, 65, 3000 and 1 back
    B.append(("ends", *chain(200, [0, 50, 120, 199], f0=25), o))                              # candidates at n - 1 and at 0: one chain between them
    f, p = chain(10, list(range(10)))
    f[:] = [0, 0, 64, 4, 20, 30, 40, 50, 60, 70]      # walking back from 9 the score falls by 60 at anchor 2 and recovers at anchor 1
    B.append(("drop_breaks", f.copy(), p.copy(), Opt(min_cnt=1, min_sc=65, max_drop=50)))
    B.append(("drop_goes_on", f.copy(), p.copy(), Opt(min_cnt=1, min_sc=65, max_drop=100)))
    f, p = chain(40, list(range(0, 20)))
    for k, i in enumerate(range(20, 30)):                                                     # a second chain that runs into the first at anchor 9
        f[i] = f[9] + 10 * (k + 1); p[i] = 9 if k == 0 else i - 1
    B.append(("joins_marked", f.copy(), p.copy(), o))
    B.append(("min_sc", f.copy(), p.copy(), Opt(min_cnt=1, min_sc=101)))                      # the second chain's own 100 points are one too few
    f, p = chain(30, [0, 1, 2, 3, 10, 11])
    p[10] = -1; f[10] = 45; f[11] = 60
    B.append(("min_cnt", f.copy(), p.copy(), Opt(min_cnt=3, min_sc=20)))
    B.append(("no_candidates", f.copy(), p.copy(), Opt(min_cnt=1, min_sc=1000)))
    f = np.full(30, 15, np.int32); p = np.full(30, -1, np.int32)
    for s in (0, 10, 20):
        for k in range(4): f[s + k] = 30 + 15 * k + s; p[s + k] = s + k - 1 if k else -1
    B.append(("cap_u_exact", f.copy(), p.copy(), Opt(min_cnt=2, min_sc=20, cap_u=3)))
    B.append(("cap_u_over", f.copy(), p.copy(), Opt(min_cnt=2, min_sc=20, cap_u=2)))
    return B


def sort_cases():
    """(name, k, v): distinct pairs for lr_sort"""
    rng = np.random.default_rng(77)
    S = []
    for n in (0, 1, 2, 63, 64, 65, 127, 128, 129, 4097, 5000):
        v = np.arange(n, dtype=np.uint64)
        S.append((f"asc{n}", np.arange(n, dtype=np.uint64) * np.uint64(3), v))
        S.append((f"desc{n}", (np.arange(n, dtype=np.uint64) * np.uint64(3))[::-1].copy(), v))
        S.append((f"rand{n}", rng.integers(0, 1 << 40, n).astype(np.uint64), v))
        S.append((f"equal_k{n}", rng.integers(0, 4, n).astype(np.uint64), rng.permutation(n).astype(np.uint64)))
        S.append((f"high_word{n}", rng.permutation(n).astype(np.uint64) << np.uint64(32) | np.uint64(7), rng.permutation(n).astype(np.uint64)))
    return S


# ---- the references, once per process ---------------------------------------------------------------------------------------------------
_REF = {}


def oracle_fill(oracle, c):
    """mmo_lchain_rmq_fill over the case: (f, p) as int32"""
    import ctypes as C
    L = oracle.lib()
    L.mmo_lchain_rmq_fill.argtypes = [C.c_int] * 5 + [C.c_float, C.c_float, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    o, n = c["o"], len(c["x"])
    a = np.zeros((n, 2), np.uint64); a[:, 0] = c["x"]; a[:, 1] = y_of(c)
    f = np.zeros(n, np.int32); p = np.zeros(n, np.int64); t = np.zeros(n, np.int32)
    L.mmo_lchain_rmq_fill(o["max_gap"], o["inner"], o["bw_long"], o["max_skip"], o["cap"], o["pen_gap"], o["pen_skip"], n, a.ctypes.data, f.ctypes.data, p.ctypes.data, t.ctypes.data)
    return f, p.astype(np.int32)


def reference(oracle, c):
    """(oracle f, oracle p, the model on its own, the model following the oracle through the ties that matter)"""
    from tests import long_join_ref as JR
    if c["name"] not in _REF:
        o = c["o"]
        f, p = oracle_fill(oracle, c)
        args = (c["x"], y_of(c), o["max_gap"], o["bw_long"], o["inner"], o["max_skip"], o["cap"], o["pen_gap"], o["pen_skip"])
        m = JR.join_model(*args)
        mf = JR.join_model(*args, follow=(f, p)) if m["matter"] else m
        _REF[c["name"]] = (f, p, m, mf)
    return _REF[c["name"]]


def oracle_backtrack(oracle, f, p, o):
    """mmo_backtrack_arrays with o.bw = max_drop: (u, v)"""
    import ctypes as C
    oo = oracle.preset("map-ont")
    oo.min_cnt, oo.min_chain_score, oo.bw = o["min_cnt"], o["min_sc"], o["max_drop"]
    f, p = np.ascontiguousarray(f, np.int32), np.ascontiguousarray(p, np.int64)
    n = len(f)
    u, v = np.zeros(n, np.uint64), np.zeros(n, np.int32)
    n_u, n_v = C.c_int32(0), C.c_int64(0)
    oracle.lib().mmo_backtrack_arrays(C.byref(oo), n, f.ctypes.data, p.ctypes.data, u.ctypes.data, v.ctypes.data, C.byref(n_u), C.byref(n_v))
    return u[:n_u.value].copy(), v[:n_v.value].copy()
