"""The chaining model (tests/chain_ref.py) against the oracle's arrays (mmo_chain_arrays / mmo_backtrack_arrays) on the case table of
tests/chain_cases.py, the known answers of tests/golden/chain_dp_kat.json, and whether the table reaches what it is meant to reach - from
the model's event report, on the CPU, so that a GPU visit is not spent on a table with a hole in it."""
import json
import os

import numpy as np
import pytest

from tests import chain_cases as K
from tests import chain_lanes as W
from tests import chain_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))


def _ints(a):
    return [int(v) for v in a]


@pytest.fixture(scope="module")
def by_name():
    return {c["name"]: c for c in K.table()}


@pytest.fixture(scope="module")
def models(oracle):
    return {c["name"]: K.model_case(oracle, c) for c in K.table()}


def test_the_presets_of_the_table_are_the_oracles(oracle):
    for name, o in K.PRESETS.items():
        p = oracle.preset(name)
        got = R.Opt(p.k, p.is_sr, p.min_cnt, p.min_chain_score, p.max_gap, p.max_gap_ref, p.max_frag_len, p.bw, p.max_chain_skip, p.max_chain_iter,
                    round(p.chain_gap_scale, 6), round(p.chain_skip_scale, 6))
        assert got == o, name


def test_the_model_equals_the_oracle_on_every_case(oracle, models):
    bad = []
    for c in K.table():
        f, p, chains = K.oracle_case(oracle, c)
        m = models[c["name"]]
        if _ints(f) != m.f or _ints(p) != m.p or chains != m.chains:
            bad.append(c["name"])
    assert not bad, bad


def test_the_model_backtrack_equals_the_oracle_on_the_handmade_states(oracle):
    for b in K.bt_table():
        chains, _, _ = R.backtrack(b["o"], _ints(b["f"]), _ints(b["p"]))
        assert oracle.backtrack_arrays(K.oracle_opts(oracle, b["o"]), b["f"], b["p"]) == chains, b["name"]


def test_known_answers(oracle, by_name):
    kat = json.load(open(os.path.join(HERE, "golden", "chain_dp_kat.json")))["cases"]
    assert len(kat) >= 20
    for e in kat:
        c = by_name[e["name"]]      # the table still holds the case the answer was written for
        assert _ints(c["x"]) == e["x"] and _ints(c["q"]) == e["q"] and c["qlen"] == e["qlen"] and c["o"]._asdict() == e["opt"], e["name"]
        f, p, chains = K.oracle_case(oracle, c)
        assert _ints(f) == e["f"] and _ints(p) == e["p"] and [list(ch) for ch in chains] == e["chains"], e["name"]
    # four of them by hand (sr: k = 21, pen_gap = 0.168; a chain with f = 21, 42, 63 lies behind the pair): 1 apart in q the link scores
    # 1 - int(0.67 + 1.16) = 0; at dd = bw it scores 10 - int(16.8 + 3.33) = -10 and is still taken, at bw + 1 it is not; two equal
    # predecessors, the later one wins
    ans = {e["name"]: e for e in kat}
    assert ans["edge_dq1"]["f"] == [21, 42, 63, 63] and ans["edge_dq1"]["p"] == [-1, 0, 1, 2] and ans["edge_dq1"]["chains"] == [[3, -1, 63, 4, 63]]
    assert ans["edge_dd_bw"]["f"] == [21, 42, 63, 53] and ans["edge_dd_bw"]["p"] == [-1, 0, 1, 2]
    assert ans["edge_dd_bw1"]["f"] == [21, 42, 63, 21] and ans["edge_dd_bw1"]["p"] == [-1, 0, 1, -1]
    assert ans["tie_dq_0"]["f"] == [21, 21, 42, 52] and ans["tie_dq_0"]["p"] == [-1, -1, 1, 2] and ans["tie_dq_0"]["chains"] == [[3, -1, 52, 3, 52]]


# ---- coverage ------------------------------------------------------------------------------------------------------------------------------
def test_sizes_sit_on_both_sides_of_every_border(by_name):
    single = {len(c["x"]) for c in K.table() if c["groups"] == 1}
    assert set(K.SIZES) <= single
    for border in (K.SMALL_CAP, 64, 128, K.RING_WIN, K.RING_CAP):
        assert {border - 1, border, border + 1} <= set(K.SIZES)
    assert all(len(c["x"]) <= 600 for c in K.table() if c["fam"] != "large")
    assert sorted(c["name"] for c in K.table() if c["fam"] == "large") == ["ring_wrap", "tile_bounds"]
    assert len({c["name"] for c in K.table()}) == len(K.table())


def test_score_edges(oracle, by_name, models):
    """each edge as a pair of anchors: which side of the comparison it is on, from the pair score itself"""
    def pair(name):      # the last anchor against the one before it
        c = by_name["edge_" + name]
        sc = R.Scorer(oracle.lib(), c["o"], c["qlen"])
        x, q = _ints(c["x"]), _ints(c["q"])
        i, j = len(x) - 1, len(x) - 2
        return sc(x[i], q[i], x[j], q[j]), (q[i] - q[j], (x[i] & 0xffffffff) - (x[j] & 0xffffffff)), sc
    for name, valid in (("dq0", False), ("dq1", True), ("dq_mdy_sr", True), ("dq_mdy1_sr", False), ("dq_mdy_long", True), ("dq_mdy1_long", False),
                        ("dr0", False), ("dr1", True), ("dd_bw", True), ("dd_bw1", False), ("dd_bw_q", True), ("dd_bw1_q", False), ("dg_k", True), ("dg_k1", True)):
        s, (dq, dr), sc = pair(name)
        assert (s != R.NONE) == valid, name
    # and the edge shows in f and p: on the valid side the last anchor links to the one before it, on the other side it does not - a kernel
    # with the comparison off by one gives other arrays on one of the two
    for inside, outside in (("dq1", "dq0"), ("dr1", "dr0"), ("dd_bw", "dd_bw1"), ("dd_bw_q", "dd_bw1_q"), ("dq_mdy_sr", "dq_mdy1_sr"),
                            ("dq_mdy_long", "dq_mdy1_long"), ("win_mdx", "win_mdx1")):
        a, b = models["edge_" + inside], models["edge_" + outside]
        n = len(a.p)
        assert a.p[-1] == n - 2 and b.p[-1] != n - 2 and a.f[-1] != b.f[-1] and a.f[-1] > by_name["edge_" + inside]["o"].k, (inside, outside)
        assert len(by_name["edge_" + inside]["x"]) <= 4      # small enough for every variant, the SmallStore's included
    assert pair("dq0")[1][0] == 0 and pair("dq1")[1][0] == 1 and pair("dr0")[1][1] == 0 and pair("dr1")[1][1] == 1
    assert models["edge_dq0"].p[-1] == models["edge_dr0"].p[-1] == 1      # past the invalid neighbour to the anchor behind it
    assert pair("dq_mdy_sr")[1][0] == pair("dq_mdy_sr")[2].mdy == 150 and pair("dq_mdy1_sr")[1][0] == 151      # is_sr: max_dist_y = qlen
    assert pair("dq_mdy_long")[1][0] == pair("dq_mdy_long")[2].mdy == 5000 < pair("dq_mdy_long")[2].mdx        # not is_sr: max_gap
    assert pair("dd_bw")[1] == (10, 110) and pair("dd_bw1")[1] == (10, 111) and pair("dd_bw_q")[1] == (110, 10) and pair("dd_bw1_q")[1] == (111, 10)
    assert by_name["edge_dd_bw"]["o"].bw == 100
    k = by_name["edge_dg_k"]["o"].k
    assert pair("dg_k")[1] == (k, k) and pair("dg_k1")[1] == (k + 1, k + 1)
    assert pair("dg_k")[0] == k and pair("dg_k1")[0] == k - 2      # a skip penalty of 0.105 a base starts beyond k: int(0.105 * 22) = 2
    # the window: max_dist_x away is in, one more is out (the pair itself would be valid: bw = max_dist_x)
    c = by_name["edge_win_mdx"]
    assert R.dists(c["o"], c["qlen"])[0] == 200 == int(c["x"][1] - c["x"][0]) and models["edge_win_mdx"].events[1].st == 0 and models["edge_win_mdx"].p[1] == 0
    assert int(by_name["edge_win_mdx1"]["x"][1] - by_name["edge_win_mdx1"]["x"][0]) == 201 and models["edge_win_mdx1"].events[1].st == 1
    assert pair("win_mdx1")[0] != R.NONE and models["edge_win_mdx1"].p[1] == -1
    assert models["edge_win_mdx_3"].events[2].st == 1
    # another strand or contig inside what would be the window
    for name in ("edge_group", "edge_strand", "groups_3x30", "groups_9x3"):
        c, m = by_name[name], models[name]
        x = _ints(c["x"])
        cut = [i for i in range(1, len(x)) if x[i] >> 32 != x[i - 1] >> 32]
        assert cut and all(m.events[i].st == i and (x[i] & 0xffffffff) - (x[i - 1] & 0xffffffff) <= R.dists(c["o"], c["qlen"])[0] for i in cut), name
    assert by_name["groups_9x3"]["groups"] > 8 and len(by_name["groups_9x3"]["x"]) <= K.SMALL_CAP      # more groups than SmallStore keeps in registers


def test_ties(by_name, models):
    chunks, subs = set(), set()
    for m_fill in K.FILLERS:
        for kind in ("dq", "dd"):
            m = models[f"tie_{kind}_{m_fill}"]
            i, j1, j2 = m_fill + 2, 0, m_fill + 1
            assert m.f[j1] == m.f[j2] and m.p[j1] == m.p[j2] == -1 and m.events[i].tie and m.p[i] == j2, (kind, m_fill)
            assert m.events[i].n_valid == 2 and m.events[i].brk is None
        chunks.add(((i - 1 - j1) // 64, (i - 1 - j2) // 64))
        subs.add(((i - 1 - j1) % 8, (i - 1 - j2) % 8))
    assert {(0, 0), (1, 0), (2, 0), (3, 0), (4, 0)} <= chunks                 # the two in one 64-chunk, and one to four chunks apart
    assert {(s, 0) for s in range(8)} <= subs | {(0, 0)} and (0, 0) in subs   # every sub-lane of the eight-lane split against sub-lane 0
    # equal f among the backtrack's candidates: visited by descending index
    b = {b["name"]: b for b in K.bt_table()}["top_3"]
    chains, _, _ = R.backtrack(b["o"], _ints(b["f"]), _ints(b["p"]))
    assert [c[0] for c in chains] == [5, 3, 1] and len({c[4] for c in chains}) == 1


def test_n_skip(models, by_name):
    brk = set()
    for s in K.SKIPS:
        m = models[f"skip_dense_{s}"]
        assert m.events[s + 1].brk is None and m.events[s + 1].n_valid == s + 1      # max_skip marked non-maxima and the maximum: no break
        assert all(e.brk == s + 1 for e in m.events[s + 2:]) and len(m.events) > s + 3
        brk.add(s + 1)
    for pos in K.SHIFTS:
        m = models[f"skip_shift_{pos}"]
        assert m.events[-1].brk == pos and m.events[-1].n_valid == 4 and by_name[f"skip_shift_{pos}"]["o"].max_skip == 2
        brk.add(pos)
    # scan lanes 1, 62, 63; lanes 0 and 1 of the second, third and fourth chunk with the count carried across; the fifth chunk (lane 0 of the
    # first chunk cannot break: nothing is marked before the first predecessor)
    assert {1, 62, 63, 64, 65, 127, 128, 129, 191, 192, 193, 256} <= brk
    ev = [(c["name"], e) for c in K.table() if len(c["x"]) <= 600 for e in models[c["name"]].events]
    assert sum(e.dec_at_zero for _, e in ev) >= 20                                          # a new maximum at n_skip = 0 after n_skip had been up
    assert sum(e.touch_zero >= 2 and e.scanned <= 64 for _, e in ev) >= 10                   # back to zero several times inside one chunk
    assert sum(e.touch_zero >= 3 for _, e in ev) >= 3
    assert any(e.brk is not None and 64 <= e.brk < 128 and e.touch_zero for _, e in ev)      # up, down to zero and a break in the second chunk


def test_max_ii(models):
    ev = [(i, e) for c in K.table() if len(c["x"]) <= 600 for i, e in enumerate(models[c["name"]].events)]
    assert sum(e.consulted and e.won for _, e in ev) >= 50 and sum(e.consulted and not e.won for _, e in ev) >= 50 and sum(e.far for _, e in ev) >= 20
    won = {i - e.max_ii for i, e in ev if e.won}
    assert {K.RING_WIN - 1, K.RING_WIN, K.RING_WIN + 1, K.RING_WIN + 2} <= won and max(won) > K.RING_CAP       # inside the ring window and beyond it
    lost = {i - e.max_ii for i, e in ev if e.consulted and not e.won}
    assert min(lost) < 64 and max(lost) > K.RING_CAP
    for gap in (20, 260):      # the best predecessor lies behind the break point: only the shortcut finds it
        m = models[f"maxii_{gap}"]
        e = m.events[-3]
        assert e.won and e.brk is not None and e.scanned < 12 and m.p[-3] == 29 and len(m.p) - 3 - 29 == gap + 13
    m = models["maxii_tie"]
    assert m.events[14].far and m.events[14].ii_tie and m.events[14].max_ii == 13 and m.f[12] == m.f[13] and m.events[18].consulted and not m.events[18].won


def test_long_scans_marks_and_max_iter(oracle, models, by_name):
    for m_fill in K.FILLERS:
        e = models[f"long_dq_{m_fill}"].events[-1]
        assert e.scanned == m_fill + 2 and e.brk is None and e.n_valid == 2 and models[f"long_dq_{m_fill}"].p[-1] == 1
    assert {63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257} <= set(K.FILLERS)      # the scan's last two steps on both sides of 64 .. 256
    # marks written by lanes past the break point: the scan breaks at position b, and a later position of the same 64-chunk holds a valid
    # predecessor whose own predecessor lies in the window - a wave marks it although the sequential scan never gets there
    def marks_past_break(name, i):
        c, m = by_name[name], models[name]
        e, x, q = m.events[i], _ints(c["x"]), _ints(c["q"])
        sc = R.Scorer(oracle.lib(), c["o"], c["qlen"])
        return [pos for pos in range(e.brk + 1, e.brk // 64 * 64 + 64)
                if i - 1 - pos >= e.st and sc(x[i], q[i], x[i - 1 - pos], q[i - 1 - pos]) != R.NONE and m.p[i - 1 - pos] >= e.st]
    assert marks_past_break("skip_dense_25", 32) == [27, 28, 29, 30] and marks_past_break("skip_dense_2", 9) and marks_past_break("skip_dense_64", 71)
    # marks in a previous chunk: skip_shift_127 breaks at position 127 on three marked anchors of the second chunk (positions 125 .. 127);
    # the first of them was marked from position 0, a chunk earlier
    m = models["skip_shift_127"]
    i = len(m.p) - 1
    assert m.events[i].brk == 127 and m.p[i - 1] == i - 1 - 125 and [m.p[i - 1 - pos] for pos in (125, 126)] == [i - 1 - 126, i - 1 - 127]
    # marks past 8192 decide breaks
    m = models["ring_wrap"]
    assert len(m.f) > K.RING_TBITS + 150 and sum(e.brk is not None for e in m.events[K.RING_TBITS + 8:]) > 100
    assert max(e.scanned for e in m.events[K.RING_TBITS:]) > K.RING_WIN and any(i - e.st > K.RING_CAP for i, e in enumerate(m.events[K.RING_TBITS:], K.RING_TBITS))
    for it in K.ITERS:
        m = models[f"iter_{it}"]
        assert by_name[f"iter_{it}"]["o"].max_iter == it
        assert not m.events[it].cut and m.events[it].st == 0 and m.p[it] == 0            # a window of exactly max_iter: anchor 0 is its last
        assert m.events[it + 1].cut and m.events[it + 1].st == 1 and m.p[it + 1] == -1   # max_iter + 1: cut off
        assert sum(e.cut for e in models[f"iter_tandem_{it}"].events) > 20


def _pf(c, m):
    return R.par_fill_model(c["o"], c["qlen"], _ints(c["x"]), _ints(c["q"]), m.events)


def test_clusters(models, by_name):
    ok = {n: _pf(by_name[n], models[n]) for n in by_name if by_name[n]["fam"] in ("clusters", "large", "groups")}
    assert ok["clus_ranks_128"][0] and len(set(_ints(by_name["clus_ranks_128"]["q"]))) == 128
    assert not ok["clus_ranks_129"][0] and len(set(_ints(by_name["clus_ranks_129"]["q"]))) == 129
    assert ok["clus_qlen_1024"][0] and not ok["clus_qlen_1025"][0] and _ints(by_name["clus_qlen_1024"]["q"]) == _ints(by_name["clus_qlen_1025"]["q"])
    for name, n_bad, applies in (("clus_dirty_64", 64, True), ("clus_dirty_65", 65, False)):
        m, o = models[name], by_name[name]["o"]
        assert sum(e.n_valid > o.max_skip or e.cut for e in m.events) == n_bad and ok[name][0] == applies, name
    assert ok["clus_dirty_64"][1] == {3} and sum(ok["clus_dirty_64"][2]) == 3
    starts = ok["clus_mixed"][2]
    sizes = np.diff([i for i, s in enumerate(starts) if s] + [len(starts)])
    assert sum(sizes == 1) >= 3 and max(sizes) == 26 and not ok["clus_mixed"][1]       # singletons; 26 anchors = max_skip + 1: still clean
    mixed = [n for n in ok if ok[n][0] and ok[n][1] and len(ok[n][1]) < sum(ok[n][2])]
    assert len(mixed) >= 6, mixed                                                        # clean and dirty clusters in one read
    # the tiled fill's borders
    applies, dirty, starts = ok["tile_bounds"]
    assert applies and not dirty
    where = [i for i, s in enumerate(starts) if s]
    assert K.PFT_T in where                                                              # a cluster starts exactly at 4096
    a = max(i for i in where if i <= 2 * K.PFT_T)
    assert 2 * K.PFT_T - K.PFT_H < a < 2 * K.PFT_T and where[where.index(a) + 1] > 2 * K.PFT_T + 100      # one spans 8192 from inside the halo
    a = max(i for i in where if i <= 3 * K.PFT_T)
    assert a < 3 * K.PFT_T - K.PFT_H and where[where.index(a) + 1] > 3 * K.PFT_T + 100                      # one spans 12288 from before the halo
    assert max(e.scanned for e in models["tile_bounds"].events) < K.PFT_H


def test_backtrack_edges():
    B = {b["name"]: b for b in K.bt_table()}
    def visits(name):
        b = B[name]
        return R.backtrack(b["o"], _ints(b["f"]), _ints(b["p"])) + (b["o"],)
    ch, _, v, o = visits("drop_bw")
    assert v[0][3] == o.bw and ch[0] == (4, -1, 300, 5, 300)                 # a drop of exactly bw does not end the walk
    ch, _, v, o = visits("drop_bw1")
    assert v[0][3] == o.bw + 1 and ch[0] == (4, 2, 200, 2, 300)              # one more does
    for name in ("taken", "taken_deep"):
        assert any(hit for _, _, hit, _, _, _ in visits(name)[2]), name
    assert [x[1] for x in visits("cnt_1")[2]] == [False] and visits("cnt_1")[2][0][5] == B["cnt_1"]["o"].min_cnt - 1
    assert visits("cnt_2")[0] == [(1, -1, 25, 2, 25)] and not visits("below_min_sc")[2]
    assert visits("sc_24_into_taken")[2][1][1:5:3] == (False, 24) and visits("sc_25_into_taken")[2][1][1:5:3] == (True, 25)
    assert len(visits("cnt_3_of_3")[0]) == 1 and visits("cnt_2_of_3")[0] == [] and visits("cnt_2_of_3")[2][0][5] == 2
    ch, _, v, _ = visits("first_rejected")
    assert not v[0][1] and v[0][0] == 2 and len(ch) == 1
    for m, over in ((K.TOPBT_MAX, False), (K.TOPBT_MAX + 1, True)):
        ch, _, v, _ = visits(f"top_{m}")
        assert v[0][1] and (sum(int(f) >= v[0][4] for f in B[f"top_{m}"]["f"]) > K.TOPBT_MAX) == over
    # a best point that stands still: the wrong comparison (>= for >) keeps one anchor more
    for name in ("plateau", "plateau_root"):
        b = B[name]
        assert R.backtrack(b["o"], _ints(b["f"]), _ints(b["p"]))[0] != R.backtrack(b["o"], _ints(b["f"]), _ints(b["p"]), late=True)[0], name
    assert max(len(b["f"]) for b in K.bt_table()) <= 600


def test_wrong_programmes_are_told_apart(oracle, models):
    """Three deliberate mistakes in the model - a scan that breaks one mark late, the smaller index on equal sums, the smaller index on equal f
    in the search for max_ii - change f or p on cases of every size class, so a variant making one of them cannot pass."""
    L = oracle.lib()
    hit = {"slack": set(), "low_tie": set(), "ii_low": set()}
    for c in K.table():
        n = len(c["x"])
        if n > 600:
            continue
        m = models[c["name"]]
        for knob, kw in (("slack", {"slack": 1}), ("low_tie", {"low_tie": True}), ("ii_low", {"ii_low": True})):
            f, p, _, _ = R.chain_dp(L, c["o"], c["qlen"], _ints(c["x"]), _ints(c["q"]), **kw)
            if f != m.f or p != m.p:
                hit[knob].add((n <= 32, n <= 64, n > 64, n > K.RING_CAP, c["name"]))
    for knob in ("slack", "low_tie"):
        for cls in range(4):
            assert sum(h[cls] for h in hit[knob]) >= 2, (knob, cls)
    assert {h[4] for h in hit["ii_low"]} >= {"maxii_tie"}


def test_broken_lane_schemes_are_told_apart(oracle, models):
    """The wave scan and the eight-lane combine, restated lane by lane (tests/chain_lanes.py), equal the oracle on every case they take; with
    the reflection term of n_skip dropped, with the break lane shut out of the tie ballot, with the combine keeping the smaller index on
    equal sums, they do not - on cases below and above 64 anchors each."""
    L = oracle.lib()
    hit = {"reflect": [], "tie": [], "combine": []}
    for c in K.table():
        n = len(c["x"])
        if n > 600:
            continue
        m = models[c["name"]]
        if c["groups"] == 1:
            assert W.wave_dp(L, c) == (m.f, m.p), c["name"]
            if W.wave_dp(L, c, no_reflect=True) != (m.f, m.p):
                hit["reflect"].append(n)
            if W.wave_dp(L, c, tie_lt=True) != (m.f, m.p):
                hit["tie"].append(n)
        applies, dirty, starts = _pf(c, m)
        if applies and max(i - e.st for i, e in enumerate(m.events)) < K.PFT_H:      # what the tiled fill must leave clean is compared
            clean = [i for a, b in zip([i for i, s in enumerate(starts) if s], [i for i, s in enumerate(starts) if s][1:] + [n]) if a not in dirty for i in range(a, b)]
            f, p = W.tiled8(L, c)
            assert [f[i] for i in clean] == [m.f[i] for i in clean] and [p[i] for i in clean] == [m.p[i] for i in clean], c["name"]
            f, p = W.tiled8(L, c, combine_lt=True)
            if [f[i] for i in clean] != [m.f[i] for i in clean] or [p[i] for i in clean] != [m.p[i] for i in clean]:
                hit["combine"].append(n)
    assert sum(n <= 64 for n in hit["reflect"]) >= 5 and sum(n > 64 for n in hit["reflect"]) >= 10 and sum(n > K.RING_CAP for n in hit["reflect"]) >= 3, hit["reflect"]
    assert sorted(hit["tie"])[:2] == [66, 67] and len(hit["tie"]) >= 4, hit["tie"]      # the maximum on lane 63 of a chunk that does not break: long_dq_63, iter_64, ...
    assert sum(n <= 64 for n in hit["combine"]) >= 5 and sum(n > 64 for n in hit["combine"]) >= 5, hit["combine"]


def test_applicability(capsys):
    """which cases a variant takes is decided in chain_cases.takes alone; no variant is left with less than half the cases its size allows"""
    T = K.table()
    for v in K.DP_VARIANTS:
        fits = [c for c in T if K.n_fits(v, len(c["x"]))]
        took = [c for c in fits if K.takes(v, len(c["x"]), c["qlen"], c["o"], c["groups"])]
        with capsys.disabled():
            print(f"\n  {v:9s} takes {len(took):3d} of {len(fits):3d} cases that fit it (table: {len(T)})", end="")
        assert 2 * len(took) >= len(fits) and len(took) >= 20, v
        assert not any(K.takes(v, len(c["x"]), c["qlen"], c["o"], c["groups"]) for c in T if not K.n_fits(v, len(c["x"])))
    for v in K.BT_VARIANTS:
        n_t = sum(K.bt_takes(v, len(c["x"])) for c in T) + sum(K.bt_takes(v, len(b["f"])) for b in K.bt_table())
        with capsys.disabled():
            print(f"\n  backtrack {v:9s} takes {n_t:3d} DP states", end="")
        assert n_t >= 60
    assert not K.takes("ring", 100, 1024, K.SRW._replace(max_iter=K.RING_TMAX_ITER + 1)) and K.takes("ring", 100, 1024, K.SRW._replace(max_iter=K.RING_TMAX_ITER))
    assert not K.takes("small", 32, 70000, K.SR) and not K.takes("small", 33, 150, K.SR) and not K.takes("mask", 65, 150, K.SR) and not K.takes("wave", 10, 150, K.SR, groups=2)
