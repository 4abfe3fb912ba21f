"""The case table of the region stage: what lies between "a read's chains" and "a region survives mm_filter_regs" (mm_gen_regs' order,
mm_set_parent, mm_select_sub, mm_sync_regs, the split / insert steps of mm_align_skeleton).  Deterministic; shared by
tests/test_regs_cases_cpu.py (oracle and model, no GPU) and tests/test_regs_gpu.py (the device entries sh_dbg_regs_short / sh_dbg_regs_long).

Two kinds of case:
  table cases  - a list of regions in mm_gen_regs' order (score, cnt, qs, qe, rs, re, rev, rid, inv) with the parameters of chain_post.  They go
                 to the long form as they are and, where every region can be written as a chain (no inv; room for its anchors), to the short
                 form as chains whose records carry those scores.
  read cases   - a read cut from a small random reference with hand-made chains of exact k-mer matches (so that alignment succeeds where
                 wanted; substitutions where a region must z-drop), for the edges of the short form alone: the number of chains around AL_R, the
                 rank loop's blocks and reg_cap, the hash order, splits, the query length around AL_Q and the scratch.
Every case says what it is there for (`edge`, `side`) and, where the answer is derivable on paper, what must come out (`expect`)."""
import numpy as np

from tests import regs_ref as M

K = 21                      # preset sr
AL_Q, AL_R = 320, 64        # csrc/sh_align.h
R0 = 1000                   # where reads are cut from contig 0
CONTIGS = (6000, 3000)
TAB = ("score", "cnt", "qs", "qe", "rs", "re", "rev", "rid", "inv")
SR = dict(mask_level=0.5, pri_ratio=0.5, best_n=20, max_gap=100)      # preset sr; min_diff = 2 k, min_strand_sc = int(max_gap * 0.8)


def world():
    """two random contigs: codes 0..3 per contig, the 4-bit packing the device and the oracle read (low nibble = even position) and the starts"""
    rng = np.random.RandomState(20260421)
    seqs = [rng.randint(0, 4, n).astype(np.uint8) for n in CONTIGS]
    allc = np.concatenate(seqs)
    if len(allc) & 1:
        allc = np.append(allc, np.uint8(0))
    packed = (allc[0::2] | allc[1::2] << 4).astype(np.uint8)
    cstart = np.concatenate([[0], np.cumsum(CONTIGS)]).astype(np.uint64)
    return dict(seqs=seqs, packed=packed, cstart=cstart)


def cut(W, qlen, r0=R0, rid=0, subs=()):
    """a forward read: qlen bases of contig rid from r0, as ASCII; subs: positions whose base is replaced by another one"""
    codes = W["seqs"][rid][r0:r0 + qlen].copy()
    for p in subs:
        codes[p] = (codes[p] + 1) & 3
    return np.frombuffer(b"ACGT", np.uint8)[codes]


# ---- table cases --------------------------------------------------------------------------------------------------------------------
def reg(score, qs, qe, cnt=3, rev=0, rid=0, rs=None, re=None, inv=0):
    """a region; on the forward strand of contig 0 it lies on the read's own diagonal unless rs / re say otherwise"""
    if rs is None:
        rs, re = R0 + qs, R0 + qe
    return dict(score=score, cnt=cnt, qs=qs, qe=qe, rs=rs, re=re, rev=rev, rid=rid, inv=inv)


def _t(name, edge, side, tab, expect=None, long_only=False, **par):
    p = dict(SR, min_diff=2 * K)
    p["min_strand_sc"] = int(p["max_gap"] * 0.8)
    p.update(par)
    return dict(name=name, edge=edge, side=side, tab=tab, par=p, expect=expect or {}, long_only=long_only, qlen=AL_Q)


def table_cases():
    """expect: parent = {row: row of its parent as mm_set_parent names it}, kept = rows select_sub keeps, in order"""
    c = []
    P = lambda: reg(1000, 0, 100)
    # -- set_parent around mask_level.  One primary [0, 100) and one later region of 100 bases [s, s + 100): ol = 100 - s of min = 100, the
    #    uncovered part s of max = 100: (100 - 2 s) / 100 > 0.5 <=> s < 25.  0.75 and 0.25 are exact in binary: s = 25 is exactly AT the level.
    for side, s, par in (("above", 24, 0), ("at", 25, 1), ("below", 26, 1)):
        c.append(_t(f"mask:uncov:{side}", "mask_level, uncovered part non-zero", side, [P(), reg(900, s, s + 100)], dict(parent={0: 0, 1: par}, kept=[0, 1])))
    # -- the same with nothing uncovered: two primaries [0, 100) [100, 200) cover the third, [s, 150); ol with the first is 100 - s of min = 100
    #    (s >= 50: min = 150 - s).  s = 50: 50 / 100 each, at the level, a primary; s = 49: 51 / 100 above; s = 51: first 49 / 99 below - second 50 / 99 above
    for side, s, par in (("above", 49, 0), ("at", 50, 2), ("below", 51, 1)):
        c.append(_t(f"mask:covered:{side}", "mask_level, nothing uncovered", side, [P(), reg(950, 100, 200), reg(900, s, 150)], dict(parent={2: par})))
    # -- float quotients that are not exact: 42 / 60 - 18 / 90 is 0.5 on paper; float32 decides (no paper answer: oracle = model = device)
    for side, s in (("above", 47), ("at", 48), ("below", 49)):
        c.append(_t(f"mask:inexact:{side}", "mask_level, inexact quotients", side, [reg(1000, 0, 90), reg(900, s, s + 60)]))
    c.append(_t("mask:two-together", "covered by two primaries, each at the level alone", "-", [P(), reg(950, 100, 200), reg(900, 60, 140)], dict(parent={2: 2})))
    # -- three covering intervals met out of order: the primaries are [200, 300) [0, 100) [100, 200) in score order, the fourth region [50, 250) is
    #    covered whole once the intervals are sorted (uncov 0): 50 / 100 at the level for the first two, 100 / 100 for the third.  Unsorted, the walk
    #    would count 150 uncovered bases and 1 - 150 / 200 = 0.25 would make it a primary.
    c.append(_t("mask:cov-sort", "coverage intervals out of order", "-", [reg(1000, 200, 300), reg(950, 0, 100), reg(900, 100, 200), reg(800, 50, 250)], dict(parent={3: 2})))
    # five of them: [30, 300) holds four primaries whole (60 / 60 each) and nothing of it is uncovered, so the first primary is its parent;
    # unsorted, 210 bases would count as uncovered and 1 - 210 / 270 = 0.22 would make it a primary
    c.append(_t("mask:cov-sort5", "coverage intervals out of order", "five", [reg(1000, 240, 300), reg(990, 60, 120), reg(980, 180, 240), reg(970, 0, 60), reg(960, 120, 180), reg(800, 30, 300)],
                dict(parent={5: 0})))
    c.append(_t("mask:nested:inner-later", "nested regions", "inner is later", [reg(1000, 0, 200), reg(900, 50, 100)], dict(parent={1: 0})))
    c.append(_t("mask:nested:outer-later", "nested regions", "outer is later", [reg(1000, 50, 100), reg(900, 0, 200)], dict(parent={1: 1})))      # 50 / 50 - 150 / 200 = 0.25
    c.append(_t("mask:touch", "regions that only touch", "-", [P(), reg(900, 100, 200)], dict(parent={1: 1})))
    # -- select_sub.  A secondary [10, 90) of the primary [0, 100) with score p: kept when s >= p * pri_ratio (float32) or s + 2 k >= p
    for ratio, p, s_at in ((0.5, 1000, 500), (0.8, 1000, 800)):      # 1000 * 0.8f = 800.0000119.. rounds to 800.0f: 800 is kept in float32, dropped in double
        for side, s, kept in (("above", s_at + 1, [0, 1]), ("at", s_at, [0, 1]), ("below", s_at - 1, [0])):
            c.append(_t(f"sub:ratio{ratio}:{side}", f"score against parent * {ratio}", side, [reg(p, 0, 100), reg(s, 10, 90)], dict(parent={1: 0}, kept=kept), pri_ratio=ratio))
    for side, s, kept in (("at", 200 - 2 * K, [0, 1]), ("below", 200 - 2 * K - 1, [0])):
        c.append(_t(f"sub:min_diff:{side}", "score + 2 k against the parent", side, [reg(200, 0, 100), reg(s, 10, 90)], dict(kept=kept), pri_ratio=0.9))
    for n2 in (2, 3, 4):      # best_n = 3
        c.append(_t(f"sub:best_n:{n2}", "eligible secondaries around best_n", f"{n2} of 3", [P()] + [reg(900 - j, 5 + j, 95) for j in range(n2)],
                    dict(kept=list(range(1 + min(n2, 3)))), best_n=3))
    # a secondary with its parent's coordinates is dropped and NOT counted: with best_n = 1 the next one is still kept
    c.append(_t("sub:same-coords", "secondary with the parent's coordinates", "-", [P(), reg(900, 0, 100), reg(800, 10, 90)], dict(kept=[0, 2]), best_n=1))
    # pri_ratio 0 switches select_sub off: even a hopeless secondary stays
    c.append(_t("sub:off", "select_sub switched off", "-", [P(), reg(10, 10, 90)], dict(parent={1: 0}, kept=[0, 1]), pri_ratio=0.0))
    # -- the strand branch: score below the ratio and min_diff, above min_strand_sc = 80, other strand, same contig, overlapping on the reference
    sp = lambda: reg(1000, 0, 300)
    ss = lambda score=90, rev=1, rid=0, rs=R0 + 120, re=R0 + 220: reg(score, 100, 200, rev=rev, rid=rid, rs=rs, re=re)
    c.append(_t("sub:strand:taken", "strand branch", "taken", [sp(), ss()], dict(kept=[0, 1], strand=[1])))
    c.append(_t("sub:strand:best_n", "strand branch", "best_n reached", [sp(), reg(900, 10, 290), ss()], dict(kept=[0, 1]), best_n=1))
    c.append(_t("sub:strand:score", "strand branch", "score at min_strand_sc", [sp(), ss(score=80)], dict(kept=[0])))
    c.append(_t("sub:strand:same-strand", "strand branch", "same strand", [sp(), ss(rev=0)], dict(kept=[0])))
    c.append(_t("sub:strand:contig", "strand branch", "other contig", [sp(), ss(rid=1, rs=120, re=220)], dict(kept=[0])))
    c.append(_t("sub:strand:right-of", "strand branch", "rs == parent's re", [sp(), ss(rs=R0 + 300, re=R0 + 400)], dict(kept=[0])))
    c.append(_t("sub:strand:left-of", "strand branch", "re == parent's rs", [sp(), ss(rs=R0 - 100, re=R0)], dict(kept=[0])))
    # -- the aliasing of the in-place compaction.  Row 1 (child of 0) is dropped, so primary 2 moves to slot 1 and its child 3, kept, lands in
    #    slot 2 - the place index "2" still names.  Row 4, another child of 2, is then compared with row 3 (score 200: 120 >= 100, kept), not with
    #    its parent (score 300: 120 < 150 and 120 + 42 < 300, dropped).
    alias = [reg(1000, 0, 100), reg(400, 10, 90), reg(300, 200, 300), reg(200, 210, 290), reg(120, 215, 285)]
    c.append(_t("sub:alias:changes", "aliasing of r[p]", "changes the outcome", alias, dict(parent={1: 0, 3: 2, 4: 2}, kept=[0, 2, 3, 4], kept_plain=[0, 2, 3])))
    # the same without the drop in front: nothing moved when row 3 is reached... row 3 is kept in slot 3, slot 2 stays the parent
    c.append(_t("sub:alias:harmless", "aliasing of r[p]", "no drop in front", [reg(1000, 0, 100), reg(600, 10, 90), reg(300, 200, 300), reg(200, 210, 290), reg(120, 215, 285)],
                dict(kept=[0, 1, 2, 3], kept_plain=[0, 1, 2, 3])))
    # -- long form only
    for side, cnt in (("equal", 5), ("above", 6), ("below", 4)):      # n_sub counts a secondary with at least as many anchors as its parent
        c.append(_t(f"long:n_sub:{side}", "cnt against the parent's", side, [reg(1000, 0, 100, cnt=5), reg(900, 10, 90, cnt=cnt), reg(800, 20, 80, cnt=cnt)],
                    dict(subsc={0: 900}, n_sub={0: 0 if cnt < 5 else 2}), long_only=True))
    c.append(_t("long:inv", "inv regions are always kept", "-", [P(), reg(10, 10, 90, inv=1), reg(9, 20, 80)], dict(kept=[0, 1]), long_only=True))
    c.append(_t("long:n1", "number of regions", "1", [P()], dict(kept=[0]), long_only=True))
    c.append(_t("long:n2", "number of regions", "2", [P(), reg(999, 100, 200)], dict(kept=[0, 1]), long_only=True))
    c.append(_t("long:n300", "number of regions", "300 primaries", [reg(5000 - j, 30 * j, 30 * j + 30, rs=30 * j, re=30 * j + 30) for j in range(300)], dict(kept=list(range(300))), long_only=True))
    # drops in front of many children: ids and parents after mm_sync_regs
    many = [reg(2000, 0, 100), reg(1900, 200, 300)]
    for j in range(40):
        many.append(reg(1200 - 25 * j, 5 + (j & 1) * 200, 95 + (j & 1) * 200))
    c.append(_t("long:sync", "sync_regs after drops", "-", many, long_only=True))
    names = [x["name"] for x in c]
    assert len(set(names)) == len(names)
    return c


def table_rows(tab):
    return np.array([[t[f] for f in TAB] for t in tab], np.int32)


# ---- chains ------------------------------------------------------------------------------------------------------------------------
def chain(anchors, score, rev=0, rid=0, yfl=0, key=None):
    """anchors: (reference position of the last base, query position of the last base on the chain's strand)"""
    xs = [rev << 63 | rid << 32 | x for x, _ in anchors]
    return dict(x=xs, q=[q for _, q in anchors], score=score, yfl=yfl, key=key)


def diag_chain(qpos, score, r0=R0, **kw):
    """exact matches of a forward read cut at r0: anchors on its diagonal at the given query positions"""
    return chain([(r0 + q, q) for q in qpos], score, **kw)


def region_chain(t, qlen):
    """a table region as a chain: first and last anchor give its coordinates, the others are spread between them"""
    n = t["cnt"]
    assert not t["inv"] and t["qe"] - t["qs"] >= K + n - 1 and t["re"] - t["rs"] >= K + n - 1 and n >= 2
    qa, qb = (qlen - t["qe"] + K - 1, qlen - t["qs"] - 1) if t["rev"] else (t["qs"] + K - 1, t["qe"] - 1)
    xa, xb = t["rs"] + K - 1, t["re"] - 1
    return chain([(xa + (xb - xa) * j // (n - 1), qa + (qb - qa) * j // (n - 1)) for j in range(n)], t["score"], rev=t["rev"], rid=t["rid"])


def _r(name, edge, side, seq, chains, expect=None, reg_cap=256, max_read_len=AL_Q, **par):
    p = dict(SR)
    p.update(par)
    # u[] order: by the first anchor's x; chains that share it: the later discovery (smaller key) stands later
    for i, ch in enumerate(chains):
        if ch["key"] is None:
            ch["key"] = (ch["score"], i)
    chains = sorted(chains, key=lambda ch: (ch["x"][0], [-ch["key"][0], -ch["key"][1]]))
    return dict(name=name, edge=edge, side=side, seq=seq, qlen=len(seq), chains=chains, par=p, expect=expect or {}, reg_cap=reg_cap, max_read_len=max_read_len)


def stack(n, equal, q0=K - 1, span=40):
    """n chains of two anchors on the read's diagonal, each one base further right: scores all different, or score and cnt all equal"""
    return [diag_chain([q0 + j, q0 + j + span], 300 if equal else 600 - j) for j in range(n)]


ZD_LEN, ZD_BLOCK = 400, range(180, 220)      # a read whose middle 40 bases are all substituted: a chain across them z-drops (40 mismatches of 8 against zdrop 100)


def zd_chain(score, n_tail=16):
    """16 anchors left of the block, n_tail right of it, all on the read's diagonal"""
    return diag_chain(list(range(20, 180, 10)) + list(range(240, 240 + 10 * n_tail, 10)), score)


def read_cases():
    W = world()
    c = []
    plain = cut(W, AL_Q)
    # -- the number of chains: AL_R (LDS -> scratch), the blocks of the rank loop
    for n in (1, 2, 63, 64, 65, 127, 128, 129):
        for equal in (False, True):
            c.append(_r(f"n_u:{n}:{'equal' if equal else 'distinct'}", "number of chains", f"{n}, {'hash order' if equal else 'distinct scores'}", plain, stack(n, equal), dict(n_u=n)))
    # -- reg_cap: one below, at, one above (overflow 2, nothing written)
    for n, ovf in ((69, 0), (70, 0), (71, 2)):
        c.append(_r(f"reg_cap:{n}of70", "reg_cap", f"{n} chains", plain, stack(n, False), dict(n_u=n, overflow=ovf), reg_cap=70))
    # -- the hash order: equal (score, cnt), different first anchors, both strands, a tandem flag
    rc_read = cut(W, AL_Q)      # reverse-strand anchors need not match for the order
    fw = [diag_chain([30 + 7 * j, 90 + 7 * j], 200) for j in range(6)]
    rv = [chain([(R0 + 40 + 5 * j, 35 + 5 * j), (R0 + 110 + 5 * j, 105 + 5 * j)], 200, rev=1) for j in range(6)]
    c.append(_r("order:strands", "hash order", "both strands", rc_read, fw + rv, dict(n_u=12)))
    td = [diag_chain([30 + 7 * j, 90 + 7 * j], 200, yfl=(1 << 10) if j & 1 else 0) for j in range(6)]      # yfl = MM_SEED_TANDEM >> 32
    c.append(_r("order:tandem", "hash order", "tandem bit", rc_read, td, dict(n_u=6)))
    c.append(_r("order:tandem-off", "hash order", "the same without the bit", rc_read, [diag_chain([30 + 7 * j, 90 + 7 * j], 200) for j in range(6)], dict(n_u=6)))
    # two chains with the SAME first anchor, score and cnt: equal z, equal x - the later discovery (smaller key) first
    same = [diag_chain([40, 80], 200, key=(200, 7)), diag_chain([40, 90], 200, key=(200, 3)), diag_chain([40, 100], 200, key=(199, 9))]
    c.append(_r("order:same-anchor", "hash order", "equal z and x: discovery order", rc_read, same, dict(n_u=3, first_key=(199, 9))))
    # -- query length: codes in LDS / in scratch, and the scratch's own limit (max_read_len 400: qcap 416)
    for qlen, mrl, ovf in ((AL_Q, AL_Q + 1, 0), (AL_Q + 1, AL_Q + 1, 0), (416, 400, 0), (417, 400, 4)):
        c.append(_r(f"qlen:{qlen}of{mrl}", "query length", f"{qlen} with max_read_len {mrl}", cut(W, qlen), [diag_chain([30, 60, 90, 200, 300], 150), diag_chain([40, 70], 60)],
                    dict(overflow=ovf, survive=not ovf), max_read_len=mrl))
    # -- splits
    zd = cut(W, ZD_LEN, subs=ZD_BLOCK)
    fill = lambda n: stack(n, False, q0=22, span=25)      # left of the block: [2 + j, 48 + j), j <= 128
    for n, where in ((1, "alone"), (64, "first"), (64, "middle"), (64, "last"), (65, "first"), (65, "middle"), (65, "last"), (130, "middle")):
        score = {"alone": 900, "first": 900, "middle": 600 - 10, "last": 100}[where]
        c.append(_r(f"split:{n}:{where}", "split", f"{n} chains, the split region {where}", zd, [zd_chain(score)] + fill(n - 1), dict(n_u=n, split=True), max_read_len=ZD_LEN))
    c.append(_r("split:tail:min_cnt", "split tail", "min_cnt anchors", zd, [zd_chain(900, n_tail=2)], dict(split=True), max_read_len=ZD_LEN))
    c.append(_r("split:tail:min_cnt-1", "split tail", "min_cnt - 1 anchors", zd, [zd_chain(900, n_tail=1)], dict(split=False), max_read_len=ZD_LEN))
    # a split that needs one slot more than the region arrays have (overflow 6): every chain kept (best_n 100), in LDS (64 of 64) and in scratch (70 of 70)
    for n, cap, ovf in ((63, 256, 0), (64, 256, 6), (69, 70, 0), (70, 70, 6)):
        c.append(_r(f"split:slot:{n}of{min(cap, 64) if n <= 64 else cap}", "split slot", f"{n} regions kept", zd, [zd_chain(900)] + [diag_chain([22 + j // 2, 62 + j // 2 + (j & 1)], 890 - j) for j in range(n - 1)],
                    dict(n_u=n, overflow=ovf, all_kept=True), reg_cap=cap, max_read_len=ZD_LEN, best_n=100))
    # -- the table cases whose regions can be chains
    for t in table_cases():
        if not t["long_only"]:
            par = {k: v for k, v in t["par"].items() if k in ("mask_level", "pri_ratio", "best_n", "max_gap")}
            c.append(_r("table:" + t["name"], t["edge"], t["side"], plain, [region_chain(x, AL_Q) for x in t["tab"]], dict(table=t["name"]), **par))
    names = [x["name"] for x in c]
    assert len(set(names)) == len(names)
    return W, c


# ---- a read case as arrays ---------------------------------------------------------------------------------------------------------------
def chain_keys(case):
    rh = M.read_hash(case["qlen"])
    return [M.chain_key(ch["x"][0], (ch["yfl"] << 32) | (K << 32) | ch["q"][0], ch["score"], len(ch["x"]), rh) for ch in case["chains"]]


def oracle_inputs(case):
    """u[] and the anchors (x, y) in chain order, as mma_align_read_rows takes them"""
    u = np.array([ch["score"] << 32 | len(ch["x"]) for ch in case["chains"]], np.uint64)
    ax = np.array([x for ch in case["chains"] for x in ch["x"]], np.uint64)
    ay = np.array([(K << 32 | q) | ((ch["yfl"] << 32) if j == 0 else 0) for ch in case["chains"] for j, q in enumerate(ch["q"])], np.uint64)
    return u, ax, ay


def model_book(case, in_place=True):
    """the model's bookkeeping of a read case: (chain, chain of its parent) per region select_sub keeps, chains by their index in u[]"""
    order = M.gen_order(chain_keys(case))
    regs = []
    for ci in order:
        ch = case["chains"][ci]
        regs.append(dict(M.anchor_coords(ch["x"], ch["q"], K, case["qlen"]), score=ch["score"], cnt=len(ch["x"]), inv=0, chain=ci))
    M.set_parent(regs, case["par"]["mask_level"])
    named = {r["id"]: r["chain"] for r in regs}
    for r in regs:
        r["parent_chain"] = named[r["parent"]]
    kept = M.select_sub(regs, case["par"]["pri_ratio"], 2 * K, case["par"]["best_n"], int(case["par"]["max_gap"] * 0.8), in_place)
    return [(r["chain"], r["parent_chain"]) for r in kept]


def link_order(case, seed):
    """a permutation of the chains: the order the device's linked list names them in"""
    return np.random.RandomState(seed * 7919 + len(case["chains"])).permutation(len(case["chains"]))


# ---- the oracle's answers (O: the oracle module) ------------------------------------------------------------------------------------------
def oracle_opts(O, par):
    o = O.preset("sr")
    o.flags |= O.F_CIGAR
    o.mask_level, o.pri_ratio, o.best_n, o.max_gap = par["mask_level"], par["pri_ratio"], par["best_n"], par["max_gap"]
    return o


def oracle_read(O, W, case):
    """(n_aligned, n_regs, dp_max, sig), [(chain, chain of the parent)], keep rows - of the whole stage, and of the top chain alone"""
    u, ax, ay = oracle_inputs(case)
    res, book, keep = O.align_read_rows(oracle_opts(O, case["par"]), W["packed"], W["cstart"], case["seq"], u, ax, ay)
    pairs = [(int(r[0]), int(book[r[1]][0]) if r[1] >= 0 else -1) for r in book]
    return res, pairs, [tuple(int(v) for v in r) for r in keep]


def oracle_top(O, W, case):
    """the same for the chain with the largest key alone (what the top_z form aligns)"""
    top = M.gen_order(chain_keys(case))[0]
    one = dict(case, chains=[case["chains"][top]])
    return oracle_read(O, W, one)


def oracle_table(O, t):
    p = t["par"]
    return O.chain_post(p["mask_level"], p["pri_ratio"], p["min_diff"], p["best_n"], p["min_strand_sc"], table_rows(t["tab"]))
