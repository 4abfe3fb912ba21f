"""The case table of the long join (tests/long_join_cases.py) against the oracle and the plain model (tests/long_join_ref.py) alone: the model
equals mmo_lchain_rmq_fill on every case (through the ties that matter it follows the oracle's choice among the tied anchors and must find one
that explains it), and each family sits on both sides of the edge it is named for - so that tests/test_long_join_gpu.py, which runs the
device code over the same table, cannot pass because a path was never taken."""
import numpy as np
import pytest

from tests import long_join_cases as LC
from tests import long_join_ref as JR


@pytest.fixture(scope="module")
def ref(oracle):
    return {c["name"]: (c,) + LC.reference(oracle, c) for c in LC.join_cases()}


def _fam(ref, fam):
    return [v for v in ref.values() if v[0]["fam"] == fam]


def _declined(v, cap=None):
    c, f, p, m, mf = v
    return "".join("D" if JR.declines(mf, nr, tree, c["o"]["cap"]) else "." for nr, tree in JR.INSTANCES.values())


def test_sizes_and_names(ref):
    cases = LC.join_cases()
    assert len({c["name"] for c in cases}) == len(cases)
    assert sum(len(c["x"]) for c in cases) <= 70000 and max(len(c["x"]) for c in cases) <= 11000
    for c in cases:      # what sh_dbg_long_join asks of a case
        xl = (c["x"] & np.uint64(0xffffffff)).astype(np.int64)
        assert np.all(xl + c["q"].astype(np.int64) <= 2 ** 31 - 1) and np.all(xl < 2 ** 31), c["name"]


def test_model_equals_the_oracle_on_every_case(ref):
    for name, (c, f, p, m, mf) in ref.items():
        assert not mf["follow_fail"], name
        assert np.array_equal(mf["F"], f) and np.array_equal(mf["P"], p), name
        if not m["matter"]: assert np.array_equal(m["F"], f) and np.array_equal(m["P"], p), name
        # up to the first tie that matters the trajectory is the same whichever tied anchor is taken
        first = min([i for i, k in m["shared"] if k == JR.TIE_MATTERS], default=len(f))
        assert np.array_equal(m["F"][:first], f[:first]) and np.array_equal(m["P"][:first], p[:first]), name


def test_block_and_same_x_edges(ref):
    assert sorted(len(v[0]["x"]) for v in _fam(ref, "block")) == [1, 2, 63, 64, 65, 128, 129]
    for c, f, p, m, mf in _fam(ref, "block"):
        assert p.tolist() == list(range(-1, len(p) - 1)) and not m["shared"]
    pend = {v[0]["name"]: v[3]["pending_max"] for v in _fam(ref, "samex")}
    assert [pend[f"samex{g}"] for g in (1, 2, 64, 65, 191, 192)] == [1, 2, 64, 65, 191, 192]
    assert JR.samex(512) == JR.samex(1024) == JR.samex(4096) == 191
    assert _declined(ref["samex191"]) == "....." and _declined(ref["samex192"]) == "DDDDD"
    c, f, p, m, mf = ref["samex_at0"]
    assert c["q"][3] == c["q"][0] and m["BJ"][3] == 0 and m["I0"][3] == 3      # anchor 0 is scored although its y is q_i: the (q_i, 0) key bound


def _reach_step(c):
    return len(c["x"]) - 4      # _reach: the anchor that reaches back, before its tail of three


def test_ring_depth(ref):
    want = {"reach_new": (512, "new", 0, True), "reach_ring": (512, "ring", 0, True), "reach_old": (512, "old", 1, True),
            "reach_near447": (512, "old", 1, True), "reach_far448": (512, "old", 1, False), "reach_old65": (512, "old", 65, False),
            "reach_old_4096": (4096, "old", 1, True), "reach_near4031": (4096, "old", 1, True), "reach_far4032": (4096, "old", 1, False),
            "reach_old65_4096": (4096, "old", 65, False)}
    for name, (nr, place, n_old_min, near) in want.items():
        c, f, p, m, mf = ref[name]
        i = _reach_step(c)
        got = JR.ring_place(m, nr, i)
        assert p[i] == 79 and f[i] > f[79], name                          # it chains to the end of the high-scoring run
        assert got[0] == place and got[1] >= n_old_min and got[2] == near, (name, got)
        assert not m["shared"] and _declined(ref[name]) == ".....", name
    assert JR.ring_place(ref["reach_near447"][3], 512, _reach_step(ref["reach_near447"][0]))[2] and _reach_step(ref["reach_near447"][0]) - 79 == 447
    assert _reach_step(ref["reach_far448"][0]) - 79 == 448 and _reach_step(ref["reach_far4032"][0]) - 79 == 4032
    for name, nr in (("reach_pml", 512), ("reach_pml_4096", 4096)):      # blocks behind the ring that cannot hold the minimum
        c, f, p, m, mf = ref[name]
        i = _reach_step(c)
        got = JR.ring_place(m, nr, i)
        assert got[0] in ("new", "ring") and got[1] >= 1, (name, got)


def test_trim(ref):
    assert ref["dist_at"][3]["BJ"][1] == 0 and ref["dist_at"][2][1] == 0 and ref["dist_past"][3]["BJ"][1] == -1 and ref["dist_past"][2][1] == -1
    o = ref["dist_at"][0]["o"]
    assert int(ref["dist_at"][0]["x"][1] - ref["dist_at"][0]["x"][0]) == max(o["max_gap"], o["bw_long"]) == int(ref["dist_past"][0]["x"][1] - ref["dist_past"][0]["x"][0]) - 1
    st = ref["leave100"][3]["ST"]
    assert max(b - a for a, b in zip(st, st[1:])) > 64
    for name in ("strand", "contig"):
        c, f, p, m, mf = ref[name]
        assert m["starts"] == [40] and p[40] == -1 and abs((int(c["x"][40]) & 0xffffffff) - (int(c["x"][39]) & 0xffffffff)) < 20000 and (int(c["x"][40]) >> 32) != (int(c["x"][39]) >> 32)
    assert ref["gap_lt_bw"][0]["o"]["max_gap"] < ref["gap_lt_bw"][0]["o"]["bw_long"] and ref["gap_gt_bw"][0]["o"]["max_gap"] > ref["gap_gt_bw"][0]["o"]["bw_long"]
    i = _reach_step(ref["cap_ample"][0])
    assert ref["cap_ample"][2][i] == 79 and ref["cap_ample"][3]["lookback_max"] > 700
    assert ref["cap_trims"][2][i] != 79 and ref["cap_trims"][3]["lookback_max"] == 600 == ref["cap_trims"][0]["o"]["cap"]      # the cap trimmed the run away
    assert _declined(ref["cap_trims"]) == ".DDDD" and _declined(ref["cap_below_ring"]) == "DDDDD" and ref["cap_below_ring"][0]["o"]["cap"] == 511


def _leaving(c, m):
    """per step with anchors leaving the inner window: (how many, do they head the (y, index) list)"""
    out = []
    q = c["q"].astype(np.int64)
    for i in range(1, len(q)):
        a, b = m["ST_IN"][i - 1], min(m["ST_IN"][i], m["I0"][i])
        if b <= a: continue
        lst = sorted(range(a, m["I0"][i]), key=lambda j: (q[j], j))
        out.append((b - a, sorted(lst[:b - a]) == list(range(a, b))))
    return out


def test_inner_list(ref):
    c, f, p, m, mf = ref["desc130"]
    assert np.all(np.diff(c["q"].astype(np.int64)) < 0) and m["list_max"] >= 128 and set(p.tolist()) == {-1}      # every entry goes in at the head
    lv = _leaving(*ref["prefix"][0:1], ref["prefix"][3])
    assert lv and all(h and d <= 64 for d, h in lv)
    lv = _leaving(ref["compact"][0], ref["compact"][3])
    assert any(not h for d, h in lv) and any(d > 64 for d, h in lv)
    m = ref["compact"][3]
    assert m["ST_IN"][300] == 150 == ref["compact"][2][300] and m["BJ"][300] != 150 and m["ST_IN"][299] < 150 - 64      # the oldest anchor that stays is the predecessor, found by the inner scan alone
    lv = _leaving(ref["wrap"][0], ref["wrap"][3])
    assert all(h for d, h in lv) and sum(d for d, h in lv) > 4096                             # the list's head goes round every ring
    for nr in (512, 1024, 4096):
        a, b = ref[f"inner{nr}_{nr - 1}"], ref[f"inner{nr}_{nr}"]
        assert a[3]["inner_span_max"] == nr - 1 and b[3]["inner_span_max"] == nr
        k = [k for k, (r, t) in JR.INSTANCES.items() if r == nr]
        assert all(_declined(a)[j - 1] == "." and _declined(b)[j - 1] == "D" for j in k)
    assert not ref["inner0"][3]["inner_on"] and not ref["inner_neg"][3]["inner_on"] and ref["inner_big"][3]["inner_on"]
    assert ref["inner_big"][0]["o"]["inner"] > max(ref["inner_big"][0]["o"]["max_gap"], ref["inner_big"][0]["o"]["bw_long"])
    assert 0 < max(ref["scan1"][3]["scan_len"]) <= 64 and max(ref["scan3"][3]["scan_len"]) > 128
    assert any(b < 64 for _, b in ref["skip_first"][3]["skip_breaks"]) and any(b >= 64 for _, b in ref["skip_later"][3]["skip_breaks"])
    assert ref["skip0"][0]["o"]["max_skip"] == 0 and ref["skip0"][3]["skip_breaks"]


def test_scoring_edges(ref):
    c, f, p, m, mf = ref["q0"]
    assert c["q"][1] == 0 and m["BJ"][1] == 0 and m["scan_len"][1] == 0
    c, f, p, m, mf = ref["exact"]
    assert p.tolist() == list(range(-1, 19)) and max(m["scan_len"]) == 0                      # an exact predecessor ends the step
    assert ref["width_at"][2][10] == 9 and ref["width_past"][2][10] != 9
    assert ref["equal_score"][3]["equal_hits"]


def test_ties(ref):
    cl = lambda name: [k for _, k in ref[name][4]["shared"]]
    assert cl("mirror") == ["a"] and cl("mirror20") == ["m"] and ref["mirror"][3]["shared"][0][0] == 2
    assert "b" in cl("tie_improved") and "m" not in cl("tie_improved")
    assert cl("tie_matters") == ["m"]
    c, f, p, m, mf = ref["tie_far"]
    i = [i for i, k in m["shared"] if k == "m"][0]
    done = m["I0"][i] // 64
    ring_lo = max(done - JR.rblk(512), 0) * 64
    assert min(m["tied"][i]) < ring_lo <= max(m["tied"][i])                                   # one tied anchor behind the 512-ring, one inside
    assert cl("tie_twice").count("m") >= 2 and not ref["tie_twice"][3]["starts"]              # a second tie in the stretch of one that matters
    assert cl("tie_matters") and ref["tie_matters"][3]["starts"] == []                        # a tie in the first stretch
    c, f, p, m, mf = ref["tie_after_empty"]
    assert len(m["starts"]) == 1 and all(i > m["starts"][0] for i, _ in m["shared"]) and m["shared"]
    c, f, p, m, mf = ref["tie_at_third"]
    assert [i for i, _ in m["shared"]] == [m["starts"][0] + 2]                                # as early as a stretch can tie
    c, f, p, m, mf = ref["tie_free_tie"]
    s = m["starts"]
    assert len(s) == 2 and any(i < s[0] for i, _ in mf["shared"]) and any(i >= s[1] for i, _ in mf["shared"]) and not any(s[0] <= i < s[1] for i, _ in mf["shared"])
    for nr in (1024, 4096):
        assert ref[f"tree{nr}_fits"][4]["tree_need"] == JR.TCAP[nr] and ref[f"tree{nr}_over"][4]["tree_need"] == JR.TCAP[nr] + 1
        j = 4 if nr == 1024 else 5
        assert _declined(ref[f"tree{nr}_fits"])[j - 1] == "." and _declined(ref[f"tree{nr}_over"])[j - 1] == "D"
    c, f, p, m, mf = ref["tree1024_no_tie"]
    assert not m["shared"] and m["tree_need"] == 0 and m["lookback_max"] > JR.TCAP[1024] and _declined(ref["tree1024_no_tie"])[3] == "."


def test_runs(ref):
    n_str = set()
    for c, f, p, m, mf in _fam(ref, "runs"):
        assert set(c["cuts"]) <= set(m["starts"]) and c["cuts"]
        if c["name"] != "runs_key0": n_str.add(len(m["starts"]) + 1)
        if c["name"].endswith("_all"): assert c["cuts"] == m["starts"]
        elif c["name"].endswith("_some"): assert len(c["cuts"]) < len(m["starts"])
    assert n_str == {2, 3, 4, 5}
    c, f, p, m, mf = ref["runs_key0"]
    assert c["cuts"] == [70] and c["q"][70] == c["q"][72] and p[72] == 71 == m["BJ"][72] and m["scan_len"][72] == 0      # anchor 70 is no candidate at 72 although it starts the run
    c, f, p, m, mf = ref["runs5_all"]
    assert c["cuts"][0] % 64 == 0 and c["cuts"][1] % 64 != 0 and any(i > c["cuts"][1] for i, _ in mf["shared"])      # a tie in a later run


def test_backtrack_and_sort_cases(oracle):
    got = {name: LC.oracle_backtrack(oracle, f, p, o) for name, f, p, o in LC.backtrack_cases()}
    B = {name: (f, p, o) for name, f, p, o in LC.backtrack_cases()}
    u, v = got["hops"]
    assert len(u) == 1 and v.tolist() == [3229, 3228, 228, 163, 100, 36, 0]
    assert got["ends"][1].tolist() == [199, 120, 50, 0]
    assert got["drop_breaks"][1].tolist() == [9, 8, 7, 6, 5, 4] and got["drop_goes_on"][1].tolist() == [9, 8, 7, 6, 5, 4, 3, 2]
    u, v = got["joins_marked"]
    assert len(u) == 2 and 9 in v.tolist()[:(int(u[0]) & 0xffffffff)] and 9 not in v.tolist()[(int(u[0]) & 0xffffffff):]
    assert len(got["no_candidates"][0]) == 0 and len(got["min_sc"][0]) == 1 and int(B["min_sc"][0][29]) >= 101      # a candidate, and its chain rejected
    assert len(LC.oracle_backtrack(oracle, *B["min_cnt"][:2], LC.Opt(min_cnt=1, min_sc=20))[0]) > len(got["min_cnt"][0])
    assert len(LC.oracle_backtrack(oracle, *B["min_sc"][:2], LC.Opt(min_cnt=1, min_sc=20))[0]) > len(got["min_sc"][0])
    assert len(got["cap_u_exact"][0]) == 3 == B["cap_u_exact"][2]["cap_u"] == B["cap_u_over"][2]["cap_u"] + 1
    ns = set()
    for name, k, v in LC.sort_cases():
        assert len(set(zip(k.tolist(), v.tolist()))) == len(k), name
        ns.add(len(k))
    assert ns == {0, 1, 2, 63, 64, 65, 127, 128, 129, 4097, 5000}
