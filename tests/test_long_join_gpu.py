"""The long join of csrc/sh_long.h called directly (sh_dbg_long_join / sh_dbg_lr_sort, csrc/sh_dbg_long.hip) on the case table of
tests/long_join_cases.py: lr_rmq_fill in the five instances the product launches, lr_rmq_fill_tree, the runs of lr_coop cut by hand and by
lr_coop_fill itself, lr_sort and the two backtracks - against the oracle's mmo_lchain_rmq_fill / mmo_backtrack_arrays and, where an instance may
decline a case or leave a tie open, against what the plain model (tests/long_join_ref.py) says it must do.  Integers only: no tolerance, no case
left out.  The whole table runs in one call (and once more shuffled); the tests share its results.

The one-lane trees (variant 6) are slow by design: they get the cases of up to ONE_LANE_MAX anchors."""
import ctypes as C

import numpy as np
import pytest

from tests import long_join_cases as LC
from tests import long_join_ref as JR

pytestmark = pytest.mark.gpu
ONE_LANE_MAX = 3000
SH_ERR_BAD_ARG = 1


class LongCase(C.Structure):
    _fields_ = [("off", C.c_uint64), ("cut_off", C.c_uint64)] + [(n, C.c_int32) for n in
                ("n", "fill", "bt", "ring", "k", "max_gap", "bw_long", "max_skip", "rmq_inner_dist", "rmq_size_cap", "min_cnt", "min_sc", "coop_min",
                 "coop_run", "max_drop", "cap_u", "n_cut", "q_cap")] + [("pen_gap", C.c_float), ("pen_skip", C.c_float)]


class LongResult(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("ok", "n_tie", "n_u", "n_v", "best", "ovf", "n_z", "pad")] + [("guard", C.c_uint64)]


class SortCase(C.Structure):
    _fields_ = [("off", C.c_uint64), ("n", C.c_int32), ("pad", C.c_int32)]


class Batch:
    """cases for one call of sh_dbg_long_join"""

    def __init__(self):
        self.x, self.y, self.n_total, self.entries, self.cuts = [], [], 0, [], []

    def anchors(self, x, y):
        off = self.n_total
        self.x.append(np.asarray(x, np.uint64)); self.y.append(np.asarray(y, np.uint64)); self.n_total += len(x)
        return off

    def add(self, off, n, o, fill=0, bt=0, ring=0, q_cap=0, cuts=(), f_in=None, p_in=None, tag=None):
        self.entries.append(dict(off=off, n=n, o=o, fill=fill, bt=bt, ring=ring, q_cap=q_cap, cut_off=len(self.cuts), n_cut=len(cuts), f_in=f_in, p_in=p_in, tag=tag))
        self.cuts += [int(v) for v in cuts]
        return len(self.entries) - 1

    def call(self, order=None):
        from scrubby_amd import lib as S
        L = S.require_gpu()
        ent = self.entries if order is None else [self.entries[i] for i in order]
        x, y = np.concatenate(self.x), np.concatenate(self.y)
        arr = (LongCase * len(ent))()
        outs, tot = [], 0
        for c, e in zip(arr, ent):
            o = e["o"]
            c.off, c.cut_off, c.n, c.fill, c.bt, c.ring, c.n_cut, c.q_cap = e["off"], e["cut_off"], e["n"], e["fill"], e["bt"], e["ring"], e["n_cut"], e["q_cap"]
            c.k, c.max_gap, c.bw_long, c.max_skip, c.rmq_inner_dist, c.rmq_size_cap = o["k"], o["max_gap"], o["bw_long"], o["max_skip"], o["inner"], o["cap"]
            c.min_cnt, c.min_sc, c.coop_min, c.coop_run, c.max_drop, c.cap_u = o["min_cnt"], o["min_sc"], o["coop_min"], o["coop_run"], o["max_drop"], o["cap_u"]
            c.pen_gap, c.pen_skip = o["pen_gap"], o["pen_skip"]
            outs.append(tot); tot += e["n"]
        f_in, p_in = np.zeros(tot, np.int32), np.full(tot, -1, np.int32)
        for at, e in zip(outs, ent):
            if e["f_in"] is not None:
                f_in[at:at + e["n"]] = e["f_in"]; p_in[at:at + e["n"]] = e["p_in"]
        cuts = np.array(self.cuts + [0], np.int32)
        res = (LongResult * len(ent))()
        f, p, t, v = (np.zeros(tot, np.int32) for _ in range(4))
        u = np.zeros(tot, np.uint64)
        rc = L.sh_dbg_long_join(0, x.ctypes.data, y.ctypes.data, len(x), C.cast(arr, C.c_void_p), len(ent), f_in.ctypes.data, p_in.ctypes.data, cuts.ctypes.data,
                                C.cast(res, C.c_void_p), f.ctypes.data, p.ctypes.data, t.ctypes.data, u.ctypes.data, v.ctypes.data)
        return rc, ent, outs, res, f, p, t, u, v

    def run(self, order=None):
        from scrubby_amd import lib as S
        rc, ent, outs, res, f, p, t, u, v = self.call(order)
        S.check(rc)
        out = [None] * len(ent)
        for k, (at, e, r) in enumerate(zip(outs, ent, res)):
            n = e["n"]
            d = {"ok": int(r.ok), "n_tie": int(r.n_tie), "n_u": int(r.n_u), "n_v": int(r.n_v), "best": int(r.best), "ovf": int(r.ovf), "n_z": int(r.n_z), "guard": int(r.guard),
                 "f": f[at:at + n].copy(), "p": p[at:at + n].copy(), "t": t[at:at + n].copy(), "u": u[at:at + n].copy(), "v": v[at:at + n].copy()}
            out[k if order is None else order[k]] = d
        return out


def _same(a, b):
    """two results of one case: everything a block hands back (f / p only where the fill did not decline, the chains only where there are any)"""
    if any(a[k] != b[k] for k in ("ok", "n_tie", "n_u", "n_v", "best", "ovf", "n_z")): return False
    if a["ok"] and not (np.array_equal(a["f"], b["f"]) and np.array_equal(a["p"], b["p"])): return False
    return np.array_equal(a["u"][:a["n_u"]], b["u"][:b["n_u"]]) and np.array_equal(a["v"][:a["n_v"]], b["v"][:b["n_v"]])


# ---- the whole table, once ------------------------------------------------------------------------------------------------------------------
COOP_RUNS = (2, 100)


@pytest.fixture(scope="module")
def table(oracle):
    """one call over every case x variant, and the same entries shuffled in a second call"""
    B = Batch()
    idx = {}
    for c in LC.join_cases():
        n, o = len(c["x"]), c["o"]
        off = B.anchors(c["x"], LC.y_of(c))
        for fill in (1, 2, 3, 4, 5):
            idx[(c["name"], fill)] = B.add(off, n, o, fill=fill, bt=2)
        if n <= ONE_LANE_MAX:
            idx[(c["name"], 6)] = B.add(off, n, o, fill=6, bt=1)
        if c["fam"] == "runs":
            for ring in (1024, 4096):
                idx[(c["name"], 7, ring)] = B.add(off, n, o, fill=7, ring=ring, cuts=c["cuts"], bt=2)
                for q_cap in (0, 64):
                    for cr in COOP_RUNS:
                        idx[(c["name"], 8, ring, q_cap, cr)] = B.add(off, n, LC.Opt(**{**o, "coop_run": cr}), fill=8, ring=ring, q_cap=q_cap, bt=2)
    res = B.run()
    rng = np.random.default_rng(3)
    order = [int(v) for v in rng.permutation(len(B.entries))]
    res2 = B.run(order)
    return {"idx": idx, "res": res, "res2": res2, "entries": B.entries}


def _cases():
    return LC.join_cases()


def test_ring_instances_decline_what_the_model_says_they_must(oracle, table):
    bad = []
    for c in _cases():
        f, p, m, mf = LC.reference(oracle, c)
        for fill, (nr, tree) in JR.INSTANCES.items():
            r = table["res"][table["idx"][(c["name"], fill)]]
            if r["ok"] != (0 if JR.declines(mf, nr, tree, c["o"]["cap"]) else 1): bad.append((c["name"], fill, r["ok"]))
    assert not bad, bad


def test_plain_instances_report_the_ties_that_matter_and_equal_the_oracle_elsewhere(oracle, table):
    bad = []
    for c in _cases():
        f, p, m, mf = LC.reference(oracle, c)
        for fill in (1, 2, 3):
            r = table["res"][table["idx"][(c["name"], fill)]]
            if not r["ok"]: continue
            if m["matter"] and not r["n_tie"] > 0: bad.append((c["name"], fill, "a tie that matters went unreported"))
            if not m["matter"] and r["n_tie"] != 0: bad.append((c["name"], fill, "n_tie", r["n_tie"]))
            if r["n_tie"] == 0 and not (np.array_equal(r["f"], f) and np.array_equal(r["p"], p)):
                d = np.nonzero((r["f"] != f) | (r["p"] != p))[0]
                bad.append((c["name"], fill, "f / p differ first at", int(d[0]), int(r["f"][d[0]]), int(f[d[0]]), int(r["p"][d[0]]), int(p[d[0]])))
    assert not bad, bad


def test_tree_instances_equal_the_oracle_and_count_the_shared_minima(oracle, table):
    bad = []
    for c in _cases():
        f, p, m, mf = LC.reference(oracle, c)
        for fill in (4, 5):
            r = table["res"][table["idx"][(c["name"], fill)]]
            if not r["ok"]: continue
            if not (np.array_equal(r["f"], f) and np.array_equal(r["p"], p)):
                d = np.nonzero((r["f"] != f) | (r["p"] != p))[0]
                bad.append((c["name"], fill, "f / p differ first at", int(d[0]), int(r["f"][d[0]]), int(f[d[0]]), int(r["p"][d[0]]), int(p[d[0]])))
            if r["n_tie"] != len(mf["shared"]): bad.append((c["name"], fill, "n_tie", r["n_tie"], len(mf["shared"])))
    assert not bad, bad


def test_one_lane_trees_equal_the_oracle(oracle, table):
    bad, n_run = [], 0
    for c in _cases():
        if (c["name"], 6) not in table["idx"]: continue
        f, p, m, mf = LC.reference(oracle, c)
        r = table["res"][table["idx"][(c["name"], 6)]]
        n_run += 1
        if not (r["ok"] == 1 and np.array_equal(r["f"], f) and np.array_equal(r["p"], p)): bad.append(c["name"])
    assert not bad and n_run >= 60, (bad, n_run)


def test_runs_equal_the_uncut_join(oracle, table):
    bad = []
    for c in _cases():
        if c["fam"] != "runs": continue
        for ring, whole in ((1024, 4), (4096, 5)):
            w = table["res"][table["idx"][(c["name"], whole)]]
            assert w["ok"] == 1
            keys = [(c["name"], 7, ring)] + [(c["name"], 8, ring, q_cap, cr) for q_cap in (0, 64) for cr in COOP_RUNS]
            for k in keys:
                r = table["res"][table["idx"][k]]
                if not (r["ok"] == 1 and r["n_tie"] == w["n_tie"] and np.array_equal(r["f"], w["f"]) and np.array_equal(r["p"], w["p"])): bad.append(k)
    assert not bad, bad


def _check_backtrack(oracle, r1, r2, f, p, o, name, bad):
    u, v = LC.oracle_backtrack(oracle, f, p, o)
    ovf = len(u) > o["cap_u"]
    for which, r in (("lane0", r1), ("wave", r2)):
        if r["ovf"] != int(ovf): bad.append((name, which, "ovf", r["ovf"], len(u), o["cap_u"]))
        if ovf: continue
        best = int((u >> np.uint64(32)).max()) if len(u) else 0
        if not (r["n_u"] == len(u) and r["n_v"] == len(v) and r["best"] == best and np.array_equal(r["u"][:len(u)], u) and np.array_equal(r["v"][:len(v)], v)):
            bad.append((name, which, r["n_u"], len(u), r["n_v"], len(v), r["best"], best))
    if not np.array_equal(r1["t"], r2["t"]): bad.append((name, "the two backtracks leave different marks"))


def test_backtracks_equal_the_oracle(oracle, table):
    B = Batch()
    todo = []
    for name, f, p, o in LC.backtrack_cases():
        n = len(f)
        off = B.anchors(np.arange(n, dtype=np.uint64) + np.uint64(1000), np.full(n, (o["k"] << 32) | 100, np.uint64))
        todo.append((name, f, p, o, B.add(off, n, o, fill=0, bt=1, f_in=f, p_in=p), B.add(off, n, o, fill=0, bt=2, f_in=f, p_in=p)))
    for c in LC.join_cases():      # and over the oracle's own f / p
        if c["name"] not in ("runs5_all", "gap_lt_bw", "skip_later", "reach_old65", "tie_free_tie", "wrap"): continue
        f, p, m, mf = LC.reference(oracle, c)
        n = len(f)
        off = B.anchors(c["x"], LC.y_of(c))
        for o in (c["o"], LC.Opt(**{**c["o"], "min_cnt": 1, "min_sc": 16, "max_drop": 40})):
            todo.append((c["name"], f, p, o, B.add(off, n, o, fill=0, bt=1, f_in=f, p_in=p), B.add(off, n, o, fill=0, bt=2, f_in=f, p_in=p)))
    res = B.run()
    bad = []
    for name, f, p, o, i1, i2 in todo:
        _check_backtrack(oracle, res[i1], res[i2], f, p, o, name, bad)
    assert all(r["guard"] == 0 for r in res)
    # behind the fills of the table: the chains of every join that equals the oracle's
    for c in _cases():
        f, p, m, mf = LC.reference(oracle, c)
        a, b = table["res"][table["idx"][(c["name"], 5)]], table["res"][table["idx"].get((c["name"], 6), table["idx"][(c["name"], 5)])]
        if a["ok"] and b["ok"]: _check_backtrack(oracle, b, a, f, p, c["o"], c["name"] + " (filled)", bad)
    assert not bad, bad


def test_order_of_the_cases_does_not_matter(table):
    bad = [i for i, (a, b) in enumerate(zip(table["res"], table["res2"])) if not _same(a, b)]
    assert not bad, [(table["entries"][i]["off"], table["entries"][i]["fill"]) for i in bad[:10]]


def test_no_guard_byte_changes(table):
    bad = [(i, r["guard"]) for res in (table["res"], table["res2"]) for i, r in enumerate(res) if r["guard"] != 0]
    assert not bad, bad[:10]


def test_bad_cases_are_refused_before_any_launch():
    o = LC.Opt()
    x, y = np.array([1000, 1020, 50000], np.uint64), np.array([500, 520, 700], np.uint64) | np.uint64(LC.K << 32)

    def rc(x, y, **kw):
        B = Batch()
        B.add(B.anchors(x, y), kw.pop("n", len(x)), kw.pop("o", o), **kw)
        return B.call()[0]
    assert rc(x, y, fill=1) == 0
    assert rc(x, y, fill=1, n=4) == SH_ERR_BAD_ARG                                            # outside the arrays
    assert rc(x, y, fill=1, n=0) == SH_ERR_BAD_ARG
    assert rc(x[::-1].copy(), y, fill=1) == SH_ERR_BAD_ARG                                    # x not ascending
    assert rc(x, y ^ np.uint64(1 << 32), fill=1) == SH_ERR_BAD_ARG                            # a q_span other than k
    assert rc(np.array([1 << 30, (1 << 31) - 5], np.uint64), np.array([10, 20], np.uint64) | np.uint64(LC.K << 32), fill=1) == SH_ERR_BAD_ARG      # x + y beyond int32
    assert rc(x, y, fill=7, ring=1024, cuts=[2]) == 0
    assert rc(x, y, fill=7, ring=1024, cuts=[1]) == SH_ERR_BAD_ARG                            # no stretch start
    assert rc(x, y, fill=7, ring=512, cuts=[2]) == SH_ERR_BAD_ARG
    assert rc(x, y, fill=9) == SH_ERR_BAD_ARG and rc(x, y, fill=1, bt=3) == SH_ERR_BAD_ARG    # variants not listed
    assert rc(x, y, fill=0, f_in=[15, 30, 15], p_in=[-1, 1, -1]) == SH_ERR_BAD_ARG            # a predecessor that is not earlier


def test_lr_sort_sorts_distinct_pairs():
    from scrubby_amd import lib as S
    L = S.require_gpu()
    cases = LC.sort_cases()
    k = np.concatenate([c[1] for c in cases] + [np.zeros(1, np.uint64)]); v = np.concatenate([c[2] for c in cases] + [np.zeros(1, np.uint64)])
    arr = (SortCase * len(cases))()
    at = 0
    for a, c in zip(arr, cases):
        a.off, a.n = at, len(c[1]); at += len(c[1])
    ok, ov, oi = np.zeros(len(k), np.uint64), np.zeros(len(k), np.uint64), np.zeros(len(k), np.uint32)
    S.check(L.sh_dbg_lr_sort(0, k.ctypes.data, v.ctypes.data, C.cast(arr, C.c_void_p), len(cases), ok.ctypes.data, ov.ctypes.data, oi.ctypes.data))
    bad = []
    for a, c in zip(arr, cases):
        s = np.lexsort((c[2], c[1]))
        sl = slice(a.off, a.off + a.n)
        if not (np.array_equal(ok[sl], c[1][s]) and np.array_equal(ov[sl], c[2][s]) and np.array_equal(oi[sl], s.astype(np.uint32))): bad.append(c[0])
    assert not bad, bad
