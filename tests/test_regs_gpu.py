"""The region stage on the device, called directly (sh_dbg_regs_short / sh_dbg_regs_long, csrc/sh_dbg_align.hip) on the case table of
tests/regs_cases.py: align_read_wave over hand-made chains in its three modes and both LDS instances, and lr_set_parent0 / lr_select_sub0 /
lr_sync_regs0 over hand-made regions - against the oracle's rows (mma_align_read_rows, mma_chain_post), the plain model (tests/regs_ref.py) and
the hand-computed tables of tests/golden/regs_kat.json.  Integers only: there is no tolerance anywhere.

The short entry takes one parameter set and one scratch size per call, so the table goes through it in one launch per (parameters, reg_cap,
max_read_len) it holds - a handful - each with every case in all three modes."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests import regs_cases as RC
from tests import regs_ref as M
from tests.test_regs_cases_cpu import model_table, predicted_overflow, rows_of_model, rows_of_oracle

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

REC = np.dtype([("next", "<u4"), ("cnt", "<u4"), ("score", "<i4"), ("key_f", "<u4"), ("key_i", "<u4"), ("yfl", "<u4"), ("off", "<u8"), ("z", "<u8")])
OUT = np.dtype([("n_aligned", "<i4"), ("n_regs", "<i4"), ("dp_max", "<i4"), ("sig", "<u4"), ("overflow", "<u4"), ("done", "<i4"), ("n_book", "<u4"), ("n_keep", "<u4"),
                ("guard", "<u4"), ("pad", "<u4")])
LCASE = np.dtype([("off", "<u8"), ("n", "<i4"), ("min_diff", "<i4"), ("best_n", "<i4"), ("min_strand_sc", "<i4"), ("mask_level", "<f4"), ("pri_ratio", "<f4")])
ROW_CAP = 160
FULL, FLAG, TOP = 0, 1, 2


class Params(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("k", "min_cnt", "min_sc", "max_gap", "bw", "bw_long", "a", "b", "q", "e", "q2", "e2", "sc_ambi", "zdrop", "zdrop_inv", "end_bonus", "min_dp_max", "best_n")] + \
               [(n, C.c_float) for n in ("pri_ratio", "mask_level", "max_clip_ratio")] + [("lemma", C.c_int32), ("unc_max", C.c_int32)]


def params(oracle, par):
    o, p = RC.oracle_opts(oracle, par), Params()
    for f, _ in Params._fields_:
        setattr(p, f, getattr(o, {"min_sc": "min_chain_score"}.get(f, f), 0))
    return p


def pack(entries, seed):
    """entries: (case, mode).  The reads, anchors and chain records of one call; a read's records are linked in a shuffled order."""
    bases, offsets, cx, cq, recs, head, modes, base = [], [0], [], [], [], [], [], []
    for c, mode in entries:
        bases.append(np.ascontiguousarray(c["seq"], np.uint8)); offsets.append(offsets[-1] + c["qlen"])
        keys = RC.chain_keys(c)
        b = len(recs)
        base.append(b)
        for ch, z in zip(c["chains"], keys):
            recs.append((0xffffffff, len(ch["x"]), ch["score"], ch["key"][0], ch["key"][1], ch["yfl"], len(cx), z))
            cx += ch["x"]; cq += ch["q"]
        order = RC.link_order(c, seed)
        for a, nxt in zip(order, list(order[1:]) + [None]):
            recs[b + a] = (0xffffffff if nxt is None else b + int(nxt),) + recs[b + a][1:]
        head.append(b + int(order[0])); modes.append(mode)
    return dict(bases=np.concatenate(bases), offsets=np.array(offsets, np.uint64), cx=np.array(cx, np.uint64), cq=np.array(cq, np.uint32), recs=np.array(recs, REC),
                head=np.array(head, np.uint32), mode=np.array(modes, np.int32), base=base)


def call_short(W, p, par, reg_cap, max_read_len):
    from scrubby_amd import lib as S
    L = S.require_gpu()
    n = len(p["head"])
    out, book, keep = np.zeros(n, OUT), np.zeros((n, ROW_CAP, 2), np.uint32), np.zeros((n, ROW_CAP, 8), np.int32)
    S.check(L.sh_dbg_regs_short(0, W["packed"].ctypes.data, W["cstart"].ctypes.data, len(W["cstart"]) - 1, p["bases"].ctypes.data, p["offsets"].ctypes.data, n,
                                p["cx"].ctypes.data, p["cq"].ctypes.data, len(p["cx"]), p["recs"].ctypes.data, len(p["recs"]), p["head"].ctypes.data, C.byref(par),
                                reg_cap, max_read_len, p["mode"].ctypes.data, ROW_CAP, out.ctypes.data, book.ctypes.data, keep.ctypes.data))
    return out, book, keep


def run_short(oracle, W, cases, seed, modes=(FULL, FLAG, TOP)):
    """every case in every mode; one call per (parameters, reg_cap, max_read_len).  -> {(name, mode): (out, [(chain, parent's chain)], [keep rows])}"""
    groups = {}
    for c in cases:
        groups.setdefault((tuple(sorted(c["par"].items())), c["reg_cap"], c["max_read_len"]), []).append(c)
    res = {}
    for (par, reg_cap, mrl), cs in groups.items():
        entries = [(c, m) for c in cs for m in modes]
        p = pack(entries, seed)
        out, book, keep = call_short(W, p, params(oracle, dict(par)), reg_cap, mrl)
        for i, (c, m) in enumerate(entries):
            nb, nk = int(out[i]["n_book"]), int(out[i]["n_keep"])
            assert nb <= ROW_CAP and nk <= ROW_CAP, c["name"]
            b = p["base"][i]
            res[c["name"], m] = (out[i], [(int(x) - b, int(y) - b) for x, y in book[i, :nb]], [tuple(int(v) for v in r) for r in keep[i, :nk]])
    return res, len(groups)


@pytest.fixture(scope="module")
def reads():
    return RC.read_cases()


@pytest.fixture(scope="module")
def want(oracle, reads):
    W, cases = reads
    return {c["name"]: RC.oracle_read(oracle, W, c) for c in cases}


@pytest.fixture(scope="module")
def device(oracle, reads):
    W, cases = reads
    res, n_calls = run_short(oracle, W, cases, 1)
    assert n_calls <= 12
    return res


def expected_overflow(c, want, top=False):
    (n_aligned, _, _, _), _, _ = want[c["name"]]
    split = c["expect"].get("split") or c["expect"].get("all_kept")
    if top:      # one chain in a 16-region array: only the query can be too long
        return 4 if predicted_overflow(dict(c, chains=c["chains"][:1]), 1, None) == 4 else 0
    return predicted_overflow(c, n_aligned, n_aligned if split else None)


def test_the_bookkeeping_rows_are_the_oracle_s_and_the_model_s(reads, device, want):
    W, cases = reads
    bad, n = [], 0
    for c in cases:
        out, book, _ = device[c["name"], FULL]
        if expected_overflow(c, want) in (2, 4) and not out["done"]:
            continue      # given up before or right after the bookkeeping: test_overflow_codes looks at these
        n += 1
        if book != want[c["name"]][1] or book != RC.model_book(c):
            bad.append((c["name"], book[:6], want[c["name"]][1][:6]))
    assert not bad, (len(bad), bad[:5])
    assert n >= len(cases) - 2


def test_the_surviving_regions_are_the_oracle_s(reads, device, want):
    W, cases = reads
    bad = []
    for c in cases:
        out, _, keep = device[c["name"], FULL]
        if expected_overflow(c, want):
            continue
        res, _, wkeep = want[c["name"]]
        got = (int(out["n_aligned"]), int(out["n_regs"]), int(out["dp_max"]), int(out["sig"]))
        if not out["done"] or got != res or keep != wkeep:
            bad.append((c["name"], int(out["done"]), int(out["overflow"]), got, res, [i for i, (a, b) in enumerate(zip(keep, wkeep)) if a != b][:3]))
    assert not bad, (len(bad), bad[:5])


def test_overflow_codes_are_the_predicted_ones_and_no_guard_band_is_touched(reads, device, want):
    W, cases = reads
    seen = set()
    for c in cases:
        for mode in (FULL, FLAG, TOP):
            out = device[c["name"], mode][0]
            assert out["guard"] == 0, (c["name"], mode)
            exp = expected_overflow(c, want, top=mode == TOP)
            if mode == FLAG and exp == 6:
                continue      # flag_only stops at the first survivor, which may come before the split
            assert (int(out["overflow"]), int(out["done"])) == (exp, 0 if exp else 1), (c["name"], mode, int(out["overflow"]), int(out["done"]), exp)
            if mode == FULL:
                seen.add(exp)
            if exp in (2, 4):      # given up before any region was aligned: no survivor rows
                assert out["n_keep"] == 0, (c["name"], mode)
    assert seen == {0, 2, 4, 6}      # 3 cannot be reached as the code stands (see mm_set_parent's loop in csrc/sh_align.h) and 5 needs a window beyond tcap


def top_is_tied(c):
    """two chains share the largest key: the product does not take the top form then (ChainSink::tie), and which of them it would align depends on the list order"""
    keys = RC.chain_keys(c)
    return keys.count(max(keys)) > 1


def test_the_modes_agree(reads, device, want):
    W, cases = reads
    n_top = 0
    for c in cases:
        full, flag, top = (device[c["name"], m] for m in (FULL, FLAG, TOP))
        if full[0]["done"] and flag[0]["done"]:
            assert (flag[0]["n_regs"] > 0) == (full[0]["n_regs"] > 0), c["name"]
        if top[0]["done"] and top[0]["n_regs"] > 0 and full[0]["done"] and not top_is_tied(c):      # a decision: the region it found is the first survivor of the full run
            assert top[2][0] == full[2][0], c["name"]
            n_top += 1
    assert n_top >= 60


def test_the_top_form_is_the_oracle_on_the_top_chain_alone(oracle, reads, device):
    W, cases = reads
    for c in cases:
        out, book, keep = device[c["name"], TOP]
        if not out["done"] or top_is_tied(c):
            continue
        res, _, wkeep = RC.oracle_top(oracle, W, c)
        assert (out["n_regs"] > 0) == (res[1] > 0), c["name"]
        if wkeep:
            assert keep[0] == wkeep[0], c["name"]


def test_a_reshuffled_link_order_gives_the_same_rows(oracle, reads, device):
    W, cases = reads
    again, _ = run_short(oracle, W, cases, 2, modes=(FULL,))
    differs = sum(list(RC.link_order(c, 1)) != list(RC.link_order(c, 2)) for c in cases)
    assert differs >= 50
    bad = [c["name"] for c in cases if again[c["name"], FULL][1:] != device[c["name"], FULL][1:] or again[c["name"], FULL][0].tobytes() != device[c["name"], FULL][0].tobytes()]
    assert not bad, bad


# ---- the long form -------------------------------------------------------------------------------------------------------------------
def run_long(tables):
    from scrubby_amd import lib as S
    L = S.require_gpu()
    tab = np.concatenate([RC.table_rows(t["tab"]) for t in tables])
    cases = np.zeros(len(tables), LCASE)
    at = 0
    for i, t in enumerate(tables):
        p = t["par"]
        cases[i] = (at, len(t["tab"]), p["min_diff"], p["best_n"], p["min_strand_sc"], p["mask_level"], p["pri_ratio"])
        at += len(t["tab"])
    n_kept, rows = np.zeros(len(tables), np.int32), np.zeros((len(tab), 6), np.int32)
    S.check(L.sh_dbg_regs_long(0, tab.ctypes.data, len(tab), cases.ctypes.data, len(tables), n_kept.ctypes.data, rows.ctypes.data))
    out = []
    for c, k in zip(cases, n_kept):
        r = rows[int(c["off"]):int(c["off"]) + int(k)]
        assert [int(x) for x in r[:, 1]] == list(range(int(k)))      # id = the place after mm_sync_regs (or from set_parent when nothing left)
        out.append([(int(x[0]), int(x[2]), int(x[3]), int(x[4]), int(x[5])) for x in r])
    return out


def kat_tables():
    kat = json.load(open(os.path.join(HERE, "golden", "regs_kat.json")))["cases"]
    return [dict(name="kat:" + c["name"], tab=[dict(zip(RC.TAB, row)) for row in c["tab"]], par=c["par"], rows=[tuple(r) for r in c["rows"]]) for c in kat]


def test_the_long_form_is_the_oracle_s_and_the_model_s(oracle):
    tables = RC.table_cases()
    got = run_long(tables)
    bad = [t["name"] for t, g in zip(tables, got) if g != rows_of_oracle(RC.oracle_table(oracle, t)) or g != rows_of_model(model_table(t))]
    assert not bad, bad
    by = {t["name"]: g for t, g in zip(tables, got)}
    assert [r[0] for r in by["sub:alias:changes"]] == [0, 2, 3, 4] and len(by["long:n300"]) == 300


def test_known_answers_on_the_device(oracle, reads):
    """the written answers on both entries: the long form's rows whole; the short form's kept regions and their parents (the tables as chains)"""
    kat = kat_tables()
    assert len(kat) >= 8
    for t, g in zip(kat, run_long(kat)):
        assert g == t["rows"], t["name"]
    W, _ = reads
    cases = []
    for t in kat:
        par = dict(RC.SR, **{k: v for k, v in t["par"].items() if k in RC.SR})
        c = RC._r(t["name"], "kat", "-", RC.cut(W, RC.AL_Q), [RC.region_chain(x, RC.AL_Q) for x in t["tab"]], **par)
        assert t["par"]["min_diff"] == 2 * RC.K and t["par"]["min_strand_sc"] == int(par["max_gap"] * 0.8)
        cases.append(c)
    res, _ = run_short(oracle, W, cases, 3, modes=(FULL,))
    for t, c in zip(kat, cases):
        key = lambda ch: (tuple(ch["x"]), tuple(ch["q"]), ch["score"])
        row = {key(RC.region_chain(x, RC.AL_Q)): i for i, x in enumerate(t["tab"])}
        out, book, _ = res[c["name"], FULL]
        got = [(row[key(c["chains"][a])], row[key(c["chains"][b])]) for a, b in book]
        assert out["done"] and got == [(r[0], t["rows"][r[1]][0]) for r in t["rows"]], t["name"]


# ---- what the entries refuse -------------------------------------------------------------------------------------------------------------
def test_the_entries_refuse_what_the_product_never_hands_over(oracle, reads):
    from scrubby_amd import lib as S
    W, cases = reads
    by = {c["name"]: c for c in cases}
    c = by["n_u:2:distinct"]
    par = params(oracle, c["par"])
    good = pack([(c, FULL)], 1)
    out, _, _ = call_short(W, good, par, 256, RC.AL_Q)
    assert out[0]["done"] == 1

    def broken(f):
        p = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in good.items()}
        f(p)
        return p

    def bump(arr, i, d):
        def f(p):
            p[arr][i] = int(p[arr][i]) + d
        return f

    def set_rec(i, field, v):
        def f(p):
            p["recs"][field][i] = v
        return f

    h = int(good["head"][0])
    bads = {
        "a list that does not end": set_rec(int(good["recs"]["next"][h]), "next", h),
        "a list that leaves the table": set_rec(h, "next", 7),
        "anchors not ascending in q": bump("cq", 1, -40),      # the chain's anchors are 40 apart: equal is not ascending
        "anchors not ascending in x": bump("cx", 1, -40),
        "an anchor on the other strand": bump("cx", 1, 1 << 63),
        "an anchor on another contig": bump("cx", 1, 1 << 32),
        "an anchor beyond the read": bump("cq", 1, 400),
        "an anchor beyond the contig": lambda p: (bump("cx", 0, 6000)(p), bump("cx", 1, 6000)(p)),
        "an anchor whose k bases start before the read": lambda p: (bump("cq", 0, -5)(p), bump("cx", 0, -5)(p)),
        "a z that is not the chain's key": set_rec(0, "z", 5),
        "a record without anchors": set_rec(0, "cnt", 0),
        "a mode that does not exist": lambda p: p["mode"].__setitem__(0, 3),
    }
    for what, f in bads.items():
        with pytest.raises(S.ScrubbyHipError):
            call_short(W, broken(f), par, 256, RC.AL_Q)
            pytest.fail(what + " was not refused")
    for reg_cap, mrl in ((0, 320), (256, 0)):
        with pytest.raises(S.ScrubbyHipError):
            call_short(W, good, par, reg_cap, mrl)
    # the long form: n within the scratch, a region that is empty on the query, a case outside the table
    one = dict(RC.table_cases()[0])
    for tab in ([RC.reg(1000 - j, 0, 100) for j in range(4097)], [RC.reg(1000, 50, 50)]):
        with pytest.raises(S.ScrubbyHipError):
            run_long([dict(one, tab=tab)])
    assert len(run_long([dict(one, tab=[RC.reg(5000 - j, 0, 100) for j in range(4096)])])[0]) >= 1      # 4096 fit
