"""A second case table of k_local_cluster: the edges of a window that GROWS (tests/lc_cases.py walks the first round's; the model is
tests/lc_model.py, unchanged).  The kernel searches a seed's occurrence list once and then extends the answer at its two ends
(scrubby_amd/csrc/sh_lc_search.h): what the later rounds admit, on either side, through more than one group of eight, up to the cap and up
to K's size, and what they must not admit, is what these families walk.

A small seeded reference of three contigs built with lc_cases.Builder, reads of 150 bases, each forward and reverse-complemented.  As in
lc_cases every family is a sweep and the model says where each read landed; tests/test_lc_cases_grow_cpu.py asks that both sides of every
edge occur.  A locus is a unit v of 110 random bases of its own (planted once, so that its seeds are singletons unless a family plants
pieces of it again) with unique flanks; a `rung` is a 31-base piece of v that holds ONE seed of the read whatever stands beside it, a
`slab` the 70 bases of v the read holds, with all their seeds.

Families (Read.family):
  above     slabs 500 above the locus, 1 to 5 of them, the read's flank on the high side: three growths upward are taken, the fourth
            gives WINDOW (lc_cases' ladder only goes below)
  both      slabs 500 apart on both sides of one locus, nb below and na above: both ends of every list move in one round; rounds are
            max(nb, na) + 1, so (3, 3) is taken and (4, 1), (1, 4) give WINDOW
  tandem    below the locus a rung the first round finds, below it a tandem of 9 to 20 copies of the rung on the OTHER strand and, beyond
            the tandem, one forward copy: the second round's step down crosses more than one group of eight entries that do not count,
            without the cap, and takes the copy behind them (19 copies are the most that leave it inside the window)
  cumcap    rungs in two tandems: nine copies the first round finds (ten with the locus), and four to eight the second round admits:
            16 in-window occurrences reached cumulatively are taken, 17 give WINDOW in round 2, no round adding more than 16
  k2nd      one slab the first round finds, four to six more that only the second round admits, the last of them cut short base by
            base: K of 64 anchors is taken, 65 give K_SIZE, and K grows past 40 only in the second round
  contig    the locus on contig 1 with a rung 600 below (above) it; a further copy at the END of contig 0 (the START of contig 2) whose
            position lies numerically inside the grown window, 500 .. 700 below (above) the rung: the list's neighbour entry on the other
            contig is never in K"""
import numpy as np

from tests import lc_cases as T_
from tests import lc_model as M

K, W, QLEN, MDX = T_.K, T_.W, T_.QLEN, T_.MDX
CONTIG_LEN = (220_000, 340_000, 220_000)
TAIL_AT = 170_000                       # contig 2: the 40-copy unit that puts every read on the repeat list
GUARD = 800                             # between two loci: each allocates every copy it plants, and a window ends max_dist_x past the last of them
TABLE_SEED = 0x6A0E1
Read, rc = T_.Read, T_.rc


class Builder(T_.Builder):
    """lc_cases.Builder over a smaller reference"""

    def __init__(self, O, seed):
        self.O = O
        self.rng = np.random.default_rng(seed)
        self.ref = [T_.ACGT[self.rng.integers(0, 4, n)].copy() for n in CONTIG_LEN]
        self.cur = [GUARD, 12_000, 12_000]      # the first bases of contigs 1 and 2 belong to the contig family
        self.reads = []
        self.n_sweep = 0

    def alloc(self, c, size, guard=GUARD):
        at = self.cur[c]
        self.cur[c] += size + guard
        assert self.cur[c] < (160_000, 190_000, 160_000)[c], "the family area of a contig is full"
        return at

    def locus(self, c, below, above):
        """a unit of its own with `below` / `above` bases of room -> (v, a0): v planted at a0"""
        v = self.unit(110)
        at = self.alloc(c, below + 200 + above)
        self.plant(c, at + below + 40, v)
        return v, at + below + 40

    def rung_locus(self, c, below, above, at=None):
        """a locus whose unit has a 31-base piece that holds ONE seed of the read in any context (strand bit 0) -> (v, a0, rung, e_in_rung)"""
        found = None
        while found is None:
            v = self.unit(110)
            for e0, strand in self.minimizers(v[:70]):
                for s in range(0, W):
                    rs = e0 - K + 1 - s
                    if strand == 0 and rs >= 0 and (K - 1 + s, 0) in self.minimizers(v[rs:rs + 31]):
                        found = (v[rs:rs + 31], K - 1 + s)
        a0 = (self.alloc(c, below + 200 + above) if at is None else at) + below + 40
        self.plant(c, a0, v)
        return v, a0, found[0], found[1]

    def low_read(self, c, a0, p40):
        """the read with its unique flank on the LOW side of the unit, and the position of its lowest singleton"""
        read = p40 + self.cut(c, a0 - 40, 110)
        singles = [e for e, _ in self.minimizers(read) if 40 <= e - K + 1 < 80]
        return read, (a0 - 40 + (min(singles) - 40) if singles else a0)

    def high_read(self, c, a0, p40):
        """... on the HIGH side, and the position of its highest singleton"""
        read = self.cut(c, a0 + 40, 110) + p40
        singles = [e for e, _ in self.minimizers(read) if 70 <= e < 110]      # k-mers that end in the flank: past its end the read leaves the reference
        return read, (a0 + 40 + max(singles) if singles else a0 + 110)


def build(O, seed=TABLE_SEED):
    B = Builder(O, seed)
    r40 = B.unit(100)
    for i in range(40):
        B.plant(2, TAIL_AT + i * 1000, r40, rev=i % 3 == 1)
    p40 = r40[30:70]

    # ---- above: the read holds the last 70 bases of v and 40 unique bases behind it; slabs of those 70 bases 500, 1000, ... above
    for c in (0, 1):
        for n in range(1, 6):
            v, a0 = B.locus(c, 0, 500 * n + 200)
            for i in range(1, n + 1):
                B.plant(c, a0 + 40 + 500 * i, v[40:])
            sw = B.sweep()
            for sh in (40, 32):
                B.add(B.cut(c, a0 + sh, 110) + p40, "above", sw, n)

    # ---- both: the read holds v whole (90 bases here) and 10 unique bases on either side
    for i, (nb, na) in enumerate(((1, 1), (2, 1), (1, 2), (2, 2), (3, 3), (3, 1), (1, 3), (4, 1), (1, 4), (0, 2), (2, 0), (3, 2), (4, 4), (0, 3), (0, 4))):
        c = i % 2
        v, a0 = B.locus(c, 500 * nb + 100, 500 * na + 200)
        for j in range(1, nb + 1):
            B.plant(c, a0 + 10 - 500 * j, v[10:100])
        for j in range(1, na + 1):
            B.plant(c, a0 + 10 + 500 * j, v[10:100])
        B.add(p40 + B.cut(c, a0 - 10, 110), "both", B.sweep(), nb * 10 + na)

    # ---- tandem: [forward copy][n copies on the other strand][rung 600 below the read's lowest singleton] ... locus
    for i, n in enumerate(range(9, 21)):
        c = i % 2
        v, a0, rung, e = B.rung_locus(c, 1500, 0)
        read, lo_s = B.low_read(c, a0, p40)
        top = lo_s - 600 - e                      # the rung the first round finds: its seed at lo_s - 600
        B.plant(c, top, rung)
        B.plant(c, top - 31 * n, rc(rung) * n)
        B.plant(c, top - 31 * (n + 1), rung)
        B.add(read, "tandem", B.sweep(), n)

    # ---- cumcap: nine copies within the first window, m2 more below it
    for i, m2 in enumerate((4, 5, 6, 7, 8, 6, 7)):
        c = i % 2
        v, a0, rung, e = B.rung_locus(c, 1500, 0)
        read, lo_s = B.low_read(c, a0, p40)
        B.plant(c, lo_s - 600, rung * 9)
        B.plant(c, lo_s - 700 - 31 * m2, rung * m2)
        B.add(read, "cumcap", B.sweep(), 10 + m2)

    # ---- k2nd: slabs of the 70 bases the read holds: one 600 below, `full` more 75 apart from 730 below on (all of them below the first
    # window, all of them inside the second), then one cut short
    for full in (4, 5, 6):
        for i, cut in enumerate(range(22, 71, 4)):
            c = i % 2
            v, a0 = B.locus(c, 1500, 0)
            B.plant(c, a0 - 600, v[:70])
            for j in range(full):
                B.plant(c, a0 - 730 - 75 * j, v[:70])
            B.plant(c, a0 - 730 - 75 * full, v[:cut])
            B.add(p40 + B.cut(c, a0 - 40, 110), "k2nd", B.sweep(), full * 100 + cut)

    # ---- contig: loci of contig 1 at fixed places - near its start, and as far in as contig 0 is long
    for i, d in enumerate(range(500, 701, 25)):
        # the START of contig 2: locus, a rung 600 above its highest singleton, the copy on contig 2 numerically d above the rung
        v, a0, rung, e = B.rung_locus(1, 0, 0, at=2_000 + 1_000 * i)
        read, hi_s = B.high_read(1, a0, p40)
        found = None
        for e0, strand in B.minimizers(v[40:]):      # a rung among the 70 bases THIS read holds
            for s in range(0, W):
                rs = 40 + e0 - K + 1 - s
                if rs >= 40 and rs + 31 <= 110 and (K - 1 + s, strand) in B.minimizers(v[rs:rs + 31]):
                    found = (v[rs:rs + 31], K - 1 + s)
        if found:
            rung, e = found
            B.plant(1, hi_s + 600 - e, rung)
            B.plant(2, hi_s + 600 + d - e, rung)
            B.add(read, "contig", B.sweep(), d)
        # the END of contig 0: the mirror image
        v, a0, rung, e = B.rung_locus(1, 0, 0, at=CONTIG_LEN[0] - 11_000 + 1_000 * i)
        read, lo_s = B.low_read(1, a0, p40)
        B.plant(1, lo_s - 600 - e, rung)
        B.plant(0, lo_s - 600 - d - e, rung)
        B.add(read, "contig", B.sweep(), -d)
    return B


class Cases:
    """the table, laid out like lc_cases.Cases (one context)"""

    def __init__(self, O):
        B = build(O)
        self.contigs = [B.ref]
        self.reads = B.reads
        self.opts = [O.preset("sr")]
        self.cidx = [O.Index.build(c, W, K) for c in self.contigs]
        self.table = [M.Table(*ix.dump()) for ix in self.cidx]
        self.model = [M.decide(O, self.opts[0], self.table[0], self.contigs[0], r.seq) for r in self.reads]
        bases, offs = T_.batch([r.seq for r in self.reads])
        self.flag = self.cidx[0].classify(self.opts[0], bases, offs, threads=8, want_trace=False)[0]

    def of(self, ctx):
        return list(range(len(self.reads))) if ctx == 0 else []

    def outcome(self, i):
        return self.model[i].outcome


_CASES = None


def cases(O):
    global _CASES
    if _CASES is None:
        _CASES = Cases(O)
    return _CASES


def foreign_in_window(O, T, i):
    """of read i: the occurrences of its searched seeds on ANOTHER contig than K's whose position lies inside the final window, as
    (list length, index in the list, index of the list's first entry on K's contig)"""
    m, d = T.model[i], T.model[i].detail
    out = []
    if "rid" not in d:
        return out
    _, seeds = M.seeds_of(O, T.opts[0], T.table[0], T.reads[i].seq)
    for lst, y in seeds:
        if 2 <= len(lst) <= T.opts[0].mid_occ:
            ctg, pos = (lst >> np.uint64(32)).astype(np.int64), ((lst & np.uint64(M.U32)) >> np.uint64(1)).astype(np.int64)
            own = np.where(ctg == d["rid"])[0]
            for j in np.where((ctg != d["rid"]) & (pos >= d["wlo"]) & (pos <= d["whi"]))[0]:
                out.append((len(lst), int(j), int(own[0]) if len(own) else -1, int(own[-1]) if len(own) else -1))
    return out


def missing_edges(O, T, rc_):
    """the edges of the module's docstring that do NOT occur on both sides among the reads of orientation rc_"""
    idx = [i for i, r in enumerate(T.reads) if r.rc == rc_]
    rows = [(T.reads[i], T.model[i], T.model[i].detail) for i in idx]
    fam = lambda f: [(r, m, d) for r, m, d in rows if r.family == f]
    tried = lambda m: m.outcome in (M.K_SIZE, M.MARGIN, M.LEMMA, M.DECIDED, M.DECIDED_FILTERED, M.SCORE_TIE)
    want = {}
    for n in (2, 3, 4):
        want[f"above: {n - 1} slabs take {n} rounds"] = any(m.rounds == n and tried(m) and r.step == n - 1 for r, m, d in fam("above"))
    want["above: a fourth growth gives WINDOW"] = any(m.outcome == M.WINDOW and d["window"] == "rounds" and r.step >= 4 for r, m, d in fam("above"))
    want["above: K holds the slabs"] = all(d["n_k"] > (r.step + 1) * 5 for r, m, d in fam("above") if tried(m))
    by = {r.step: (m, d) for r, m, d in fam("both")}
    for nb, na in ((1, 1), (2, 1), (1, 2), (2, 2), (3, 3), (3, 1), (1, 3), (0, 2), (2, 0), (3, 2), (0, 3)):
        want[f"both: {nb} below and {na} above take {max(nb, na) + 1} rounds"] = nb * 10 + na in by and by[nb * 10 + na][0].rounds == max(nb, na) + 1 and tried(by[nb * 10 + na][0])
    for nb, na in ((4, 1), (1, 4), (4, 4), (0, 4)):
        want[f"both: {nb} below and {na} above give WINDOW"] = nb * 10 + na in by and by[nb * 10 + na][0].outcome == M.WINDOW and by[nb * 10 + na][1]["window"] == "rounds"
    want["both: K holds both sides"] = any(m.K and max(a[0] & M.U32 for a in m.K) - min(a[0] & M.U32 for a in m.K) >= 900 for r, m, d in fam("both") if r.step == 11)
    ta = {r.step: (m, d) for r, m, d in fam("tandem")}
    # K: the locus' anchors, the rung, and the forward copy beyond the tandem: one of K's lowest anchors lies 31 (n + 1) below the rung's (a rung
    # may hold a second seed of the read; at 20 copies the forward copy's seed is 651 below the rung's, and only such a second seed is inside)
    xs = lambda m: sorted(a[0] & M.U32 for a in m.K)
    beyond = lambda n: n in ta and tried(ta[n][0]) and ta[n][0].rounds >= 3 and any(x + 31 * (n + 1) in xs(ta[n][0]) for x in xs(ta[n][0])[:3])
    for n in range(9, 20):
        want[f"tandem: the copy beyond {n} entries of the other strand is taken"] = beyond(n)
    want["tandem: 20 entries"] = 20 in ta and tried(ta[20][0])
    want["tandem: the cap is not met"] = all(d["cap"] <= 3 for m, d in ta.values())
    for i in idx:      # the tandem's copies are in the searched list: n + 3 entries
        if T.reads[i].family == "tandem":
            want[f"tandem: a list of {T.reads[i].step} + 3"] = T.reads[i].step + 3 in [len(lst) for lst, y in M.seeds_of(O, T.opts[0], T.table[0], T.reads[i].seq)[1]]
    cu = fam("cumcap")
    for n in (15, 16):
        want[f"cumcap: {n} in-window occurrences over two rounds are taken"] = any(d.get("cap") == n and tried(m) and m.rounds == 3 for r, m, d in cu)
    for n in (17, 18):
        want[f"cumcap: {n} give WINDOW in round 2"] = any(d.get("cap") == n and m.outcome == M.WINDOW and d["window"] == "cap" and m.rounds == 2 for r, m, d in cu)
    k2 = fam("k2nd")
    want["k2nd: K of fewer than 64 anchors is taken"] = sum(d.get("n_k", 99) < 64 and m.outcome != M.K_SIZE and m.rounds == 3 for r, m, d in k2) >= 5
    for n in (64,):
        want[f"k2nd: K of {n} anchors after the second round is taken"] = any(d.get("n_k") == n and m.outcome != M.K_SIZE and m.rounds == 3 for r, m, d in k2)
    for n in (65,):
        want[f"k2nd: K of {n} gives K_SIZE"] = any(d.get("n_k") == n and m.outcome == M.K_SIZE and m.rounds == 3 for r, m, d in k2)
    want["k2nd: no seed near the cap"] = all(d["cap"] <= 10 for r, m, d in k2)
    for name, sign in (("the end of contig 0", -1), ("the start of contig 2", 1)):
        hit = []
        for i in idx:
            r, m = T.reads[i], T.model[i]
            if r.family == "contig" and r.step * sign > 0 and tried(m) and m.rounds >= 2:
                f = foreign_in_window(O, T, i)
                # ... and next to the list's entries on K's contig: the neighbour the search remembers
                hit += [x for x in f if (x[1] == x[2] - 1 if sign < 0 else x[1] == x[3] + 1)]
        want[f"contig: a copy at {name} inside the grown window, next to K's entries in the list"] = len(hit) >= 3
    want["contig: only one contig in K"] = all(len({a[0] >> 32 for a in m.K}) <= 1 for r, m, d in fam("contig"))
    return [name for name, ok in want.items() if not ok]
