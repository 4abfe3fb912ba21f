"""The case table of the region stage (tests/regs_cases.py) on the CPU: every case is what it says it is, both sides of every edge are there,
the oracle (mma_align_read_rows / mma_chain_post) and the plain model (tests/regs_ref.py) agree on every bookkeeping row, and the hand-computed
tables of tests/golden/regs_kat.json come out as written on both.  Integers only."""
import json
import os

import pytest

from tests import regs_cases as RC
from tests import regs_ref as M

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def tables():
    return RC.table_cases()


@pytest.fixture(scope="module")
def reads():
    return RC.read_cases()


@pytest.fixture(scope="module")
def read_answers(oracle, reads):
    W, cases = reads
    return {c["name"]: RC.oracle_read(oracle, W, c) for c in cases}


def model_table(t, in_place=True):
    p = t["par"]
    return M.chain_post(t["tab"], p["mask_level"], p["pri_ratio"], p["min_diff"], p["best_n"], p["min_strand_sc"], in_place)


def rows_of_model(regs):
    return [(r["orig"], r["parent"], r["subsc"], r["n_sub"], r["strand_retained"]) for r in regs]


def rows_of_oracle(book):
    return [(int(r[0]), int(r[1]), int(r[10]), int(r[11]), int(r[12])) for r in book]


def test_the_oracle_and_the_model_agree_on_every_table(oracle, tables):
    assert len(tables) >= 40
    bad = [t["name"] for t in tables if rows_of_oracle(RC.oracle_table(oracle, t)) != rows_of_model(model_table(t))]
    assert not bad, bad


def test_the_tables_are_what_they_are_meant_to_be(oracle, tables):
    n_checked = 0
    for t in tables:
        e = t["expect"]
        got_o, got_m = rows_of_oracle(RC.oracle_table(oracle, t)), rows_of_model(model_table(t))
        if "parent" in e:      # as mm_set_parent names it, before anything is dropped
            regs = M.set_parent([dict(x) for x in t["tab"]], t["par"]["mask_level"])
            assert {i: regs[i]["parent"] for i in e["parent"]} == e["parent"], t["name"]
            for i, p in e["parent"].items():      # and on the oracle, for the rows that are kept with their parent
                at = {r[0]: j for j, r in enumerate(got_o)}
                if i in at and p in at:
                    assert got_o[at[i]][1] == at[p], t["name"]
        for got in (got_o, got_m):
            if "kept" in e:
                assert [r[0] for r in got] == e["kept"], t["name"]
            if "strand" in e:
                assert [r[0] for r in got if r[4]] == e["strand"], t["name"]
            for f, col in (("subsc", 2), ("n_sub", 3)):
                if f in e:
                    assert {r[0]: r[col] for r in got if r[0] in e[f]} == e[f], t["name"]
        if "kept_plain" in e:      # the reading without the aliasing
            assert [r[0] for r in rows_of_model(model_table(t, in_place=False))] == e["kept_plain"], t["name"]
        n_checked += bool(e)
    assert n_checked >= 35


def test_the_aliasing_case_separates_the_two_readings(tables):
    by = {t["name"]: t for t in tables}
    a, b = by["sub:alias:changes"], by["sub:alias:harmless"]
    assert rows_of_model(model_table(a)) != rows_of_model(model_table(a, in_place=False))
    assert rows_of_model(model_table(b)) == rows_of_model(model_table(b, in_place=False))


def test_both_sides_of_every_edge_are_in_the_table(tables, reads):
    have = {(c["edge"], c["side"]) for c in tables + reads[1]}
    for edge in ("mask_level, uncovered part non-zero", "mask_level, nothing uncovered", "mask_level, inexact quotients", "score against parent * 0.5", "score against parent * 0.8"):
        assert {(edge, s) for s in ("above", "at", "below")} <= have, edge
    want = [("score + 2 k against the parent", "at"), ("score + 2 k against the parent", "below"), ("nested regions", "inner is later"), ("nested regions", "outer is later"),
            ("regions that only touch", "-"), ("covered by two primaries, each at the level alone", "-"), ("coverage intervals out of order", "-"), ("coverage intervals out of order", "five"),
            ("secondary with the parent's coordinates", "-"), ("aliasing of r[p]", "changes the outcome"), ("aliasing of r[p]", "no drop in front"),
            ("cnt against the parent's", "equal"), ("cnt against the parent's", "above"), ("cnt against the parent's", "below"), ("inv regions are always kept", "-"),
            ("number of regions", "1"), ("number of regions", "2"), ("number of regions", "300 primaries"), ("sync_regs after drops", "-"),
            ("hash order", "both strands"), ("hash order", "tandem bit"), ("hash order", "equal z and x: discovery order"),
            ("split tail", "min_cnt anchors"), ("split tail", "min_cnt - 1 anchors")]
    want += [("eligible secondaries around best_n", f"{n} of 3") for n in (2, 3, 4)]
    want += [("strand branch", s) for s in ("taken", "best_n reached", "score at min_strand_sc", "same strand", "other contig", "rs == parent's re", "re == parent's rs")]
    want += [("number of chains", f"{n}, {how}") for n in (1, 2, 63, 64, 65, 127, 128, 129) for how in ("distinct scores", "hash order")]
    want += [("reg_cap", f"{n} chains") for n in (69, 70, 71)]
    want += [("split", f"{n} chains, the split region {w}") for n in (64, 65) for w in ("first", "middle", "last")] + [("split", "1 chains, the split region alone")]
    want += [("split slot", f"{n} regions kept") for n in (63, 64, 69, 70)]
    want += [("query length", f"{q} with max_read_len {m}") for q, m in ((320, 321), (321, 321), (416, 400), (417, 400))]
    missing = [w for w in want if w not in have]
    assert not missing, missing
    # every table case that can be written as chains goes to the short form as well
    assert {"table:" + t["name"] for t in tables if not t["long_only"]} <= {c["name"] for c in reads[1]}


def predicted_overflow(case, n_aligned, split_at):
    """the code align_read_wave must give a read up with, from the sizes alone (csrc/sh_align.h): 2 more chains than reg_cap; 4 a query in
    scratch (longer than AL_Q) beyond qcap = (max(max_read_len, 32) + 31) & ~15; 6 a split when the region arrays are full (AL_R in LDS, reg_cap
    in scratch).  split_at: how many regions there are when the first split comes, or None."""
    n_u = len(case["chains"])
    if n_u > case["reg_cap"]:
        return 2
    if case["qlen"] > RC.AL_Q and case["qlen"] > ((max(case["max_read_len"], 32) + 31) & ~15):
        return 4
    if split_at is not None and split_at + 1 > (case["reg_cap"] if n_u > RC.AL_R else RC.AL_R):
        return 6
    return 0


def test_the_reads_are_what_they_are_meant_to_be(reads, read_answers):
    W, cases = reads
    assert len(cases) >= 75
    by = {c["name"]: c for c in cases}
    for c in cases:
        e = c["expect"]
        (n_aligned, n_regs, dp_max, sig), book, keep = read_answers[c["name"]]
        assert n_aligned == len(book) and n_regs == len(keep), c["name"]
        if "n_u" in e:
            assert len(c["chains"]) == e["n_u"], c["name"]
        if "split" in e:      # a split adds a region behind the one that z-dropped; here both halves survive
            assert n_regs == n_aligned + (1 if e["split"] else 0), c["name"]
        if e.get("all_kept"):
            assert n_aligned == len(c["chains"]) and n_regs == n_aligned + 1, c["name"]
        if "survive" in e:
            assert n_regs > 0
        split = e.get("split") or e.get("all_kept")
        assert predicted_overflow(c, n_aligned, n_aligned if split else None) == e.get("overflow", 0), c["name"]
        # the anchors are what the device entry insists on: ascending, inside the read and the contig, one contig and strand per chain
        for ch in c["chains"]:
            assert all(a < b for a, b in zip(ch["x"], ch["x"][1:])) and all(a < b for a, b in zip(ch["q"], ch["q"][1:])), c["name"]
            assert RC.K - 1 <= ch["q"][0] and ch["q"][-1] < c["qlen"] and len({x >> 32 for x in ch["x"]}) == 1, c["name"]
            rid = ch["x"][0] >> 32 & 0x7fffffff
            assert RC.K - 1 <= (ch["x"][0] & 0xffffffff) and (ch["x"][-1] & 0xffffffff) < RC.CONTIGS[rid], c["name"]
    # the region arrays are in LDS up to AL_R chains and in scratch beyond: both, with and without a split
    assert {len(c["chains"]) > RC.AL_R for c in cases if c["expect"].get("split")} == {True, False}
    # where the split region stands among the kept ones
    for n in (64, 65):
        first, mid, last = (read_answers[f"split:{n}:{w}"][1] for w in ("first", "middle", "last"))
        zd = lambda c: max(range(len(c["chains"])), key=lambda i: len(c["chains"][i]["x"]))      # the chain across the block has the most anchors
        at = [[ch for ch, _ in b].index(zd(by[f"split:{n}:{w}"])) for b, w in ((first, "first"), (mid, "middle"), (last, "last"))]
        assert at[0] == 0 and 0 < at[1] < len(mid) - 1 and at[2] == len(last) - 1, at
    # the tandem bit changes the order of otherwise equal chains; equal z and x falls back on the discovery order
    assert [ch for ch, _ in read_answers["order:tandem"][1]] != [ch for ch, _ in read_answers["order:tandem-off"][1]]
    c = by["order:same-anchor"]
    assert c["chains"][read_answers["order:same-anchor"][1][0][0]]["key"] == c["expect"]["first_key"]
    strands = [c["x"][0] >> 63 for c in by["order:strands"]["chains"]]
    order = [strands[ch] for ch, _ in read_answers["order:strands"][1]]
    assert order != sorted(order) and order != sorted(order, reverse=True)      # the hash mixes the strands


def test_the_oracle_and_the_model_agree_on_every_read(reads, read_answers):
    W, cases = reads
    bad = [c["name"] for c in cases if read_answers[c["name"]][1] != RC.model_book(c)]
    assert not bad, bad
    # and the aliasing shows in the short form as it does in the table
    by = {c["name"]: c for c in cases}
    assert RC.model_book(by["table:sub:alias:changes"]) != RC.model_book(by["table:sub:alias:changes"], in_place=False)


def test_a_table_as_chains_gives_the_table_back(reads, read_answers, tables):
    """regions written as chains come back in the table's order with the table's parents (scores are distinct, so the hash does not reorder)"""
    W, cases = reads
    by = {c["name"]: c for c in cases}
    for t in tables:
        if t["long_only"]:
            continue
        c = by["table:" + t["name"]]
        key = lambda ch: (tuple(ch["x"]), tuple(ch["q"]), ch["score"])      # a chain of the case, found again by its anchors and score
        rows = {key(RC.region_chain(x, RC.AL_Q)): i for i, x in enumerate(t["tab"])}
        assert len(rows) == len(t["tab"])
        got = [(rows[key(c["chains"][ch])], rows[key(c["chains"][p])]) for ch, p in read_answers[c["name"]][1]]
        kept = rows_of_model(model_table(t))
        want = [(r[0], kept[r[1]][0]) for r in kept]
        assert got == want, t["name"]


def test_known_answers(oracle):
    kat = json.load(open(os.path.join(HERE, "golden", "regs_kat.json")))["cases"]
    assert len(kat) >= 8
    for c in kat:
        p = c["par"]
        tab = [dict(zip(RC.TAB, row)) for row in c["tab"]]
        want = [tuple(r) for r in c["rows"]]
        assert rows_of_model(M.chain_post(tab, p["mask_level"], p["pri_ratio"], p["min_diff"], p["best_n"], p["min_strand_sc"])) == want, c["name"]
        assert rows_of_oracle(oracle.chain_post(p["mask_level"], p["pri_ratio"], p["min_diff"], p["best_n"], p["min_strand_sc"], c["tab"])) == want, c["name"]


def test_the_hashes_of_the_model_are_the_oracle_s(oracle):
    """mmo_hash64 with a full mask is the 64-bit mix the region order uses"""
    for key in (0, 1, 0x8000000100000419, (1 << 64) - 1, 21 << 32 | 40):
        assert M.hash64(key) == oracle.lib().mmo_hash64(key, (1 << 64) - 1)
