"""The reference and the case table of k_local_cluster (the model is tests/lc_model.py).

One seeded reference of three contigs of random bases with exact copies of named random units planted into it, and a second small one whose
index is read with mid_occ = 12.  Reads of 150 bases unless a family says otherwise, glued from unique reference sequence and pieces of units.
Minimizers move with their neighbours, so no construction hits its target by arithmetic alone: every family is a SWEEP - a junction, a distance
or a copy number moved one step at a time - the whole sweep stays in the table, and the model says where each read of it landed.
tests/test_lc_cases_cpu.py then asks that both sides of every edge occur.  Every read comes forward and reverse-complemented.

Families (Read.family), and the premise of the kernel each walks across:
  list      units planted L times, > 3 max_dist_x apart, ascending over all three contigs and on both strands; the read touches copy t:
            the 8-ary lower bound must find exactly that copy, for t at the ends and around every first-round step boundary
  nowin     a repeated seed whose copies all lie below the window, above it, or on other contigs
  ladder    copies of a unit 600 bases apart below the locus, 1 to 5 rungs: 3 growths of the window are taken, the 4th gives WINDOW
  edge      four 31-base rungs that hold ONE seed of the read, 600 apart, the first moved base by base across the window's lower edge:
            on the edge (>= the lower key) the window grows four times, one base below it nothing is found; lists of 5 and of 13 occurrences
            (the second with the rung on the edge at a step boundary of the 8-ary search)
  cap       a tandem of period 31 to 38 beside the locus, 14 to 19 copies: 16 in-window occurrences of a seed are taken, 17 give WINDOW
  ksize     tandems again, K of 60 to 70 anchors in one cluster: 64 are taken, 65 give K_SIZE
  apart     two unique pieces of one contig and strand, their outermost singletons moved across 4 max_dist_x base by base; both orders of a
            long and a short piece, so that K's second cluster wins in one of them
  chimera   j = 21 .. 149 unique bases and the rest from a 40-copy unit far away, as they are (co-diagonal: the fast path) and with one base
            inserted (two diagonals: the general path): the margin over U_out changes sign along the sweep.  Also with the rest from another
            contig or the other strand (singletons elsewhere count as outside K), at base 0 of a contig and at a contig's end
  margin    the same two pieces, their lengths and the unit's phase chosen so that the margin is -3 .. 3, one read of each; and with 32
            bases from 1000 further on between them: a second cluster in K, the general path with a chain_lemma that passes
  span      21 .. 63 unique bases and 32 of the 40-copy unit (one seed, U_out = k): K of two to five co-diagonal anchors that out-score U_out,
            its span on either side of k
  fast      a unique piece with substitutions: bases outside the k-mers on either side of ext_unc_max, and every second base of a stretch
            substituted, the stretch growing until the middle check fails
  nseed     reads of 1 to 3 and of 59 to 69 minimizers (qlen 30 .. 90 and 380 .. 511)
  nosingle  reads glued from the inside of two planted units
  high      second reference: a unit planted mid_occ + 1 = 13 times, reads of 250 and 251 bases: (int)(qlen / 500 + .499) is 0, then 1"""
from collections import namedtuple

import numpy as np

from tests import lc_model as M

K, W = 21, 11
QLEN, MDX = 150, 650                    # sr at 150 bases: max(800 - 150, 100)
CONTIG_LEN = (1_300_000, 1_200_000, 1_200_000)
FAMILY_END, GRID_AT, GRID_SLOT, TAIL_AT = 640_000, 650_000, 200, 1_110_000
GUARD = 4500                            # between two loci: more than the widest window a read can reach (4 + 2 max_dist_x)
LIST_L = (2, 7, 8, 9, 10, 63, 64, 65, 72, 73, 511, 512, 513)
HIGH_MID_OCC, HIGH_MAX_OCC = 12, 40
TABLE_SEED = 0x10CA1E
ACGT = np.frombuffer(b"ACGT", np.uint8)
COMP = bytes.maketrans(b"ACGT", b"TGCA")

Read = namedtuple("Read", "seq ctx family sweep step rc")


def rc(s):
    return bytes(s).translate(COMP)[::-1]


def subst(b):
    return b"CGTA"[b"ACGT".index(bytes([b]))]


class Builder:
    def __init__(self, O, seed):
        self.O = O
        self.rng = np.random.default_rng(seed)
        self.ref = [ACGT[self.rng.integers(0, 4, n)].copy() for n in CONTIG_LEN]
        self.cur = [GUARD, GUARD, GUARD]
        self.reads = []
        self.n_sweep = 0

    def unit(self, n=None):
        return ACGT[self.rng.integers(0, 4, n or int(self.rng.integers(90, 121)))].tobytes()

    def alloc(self, c, size, guard=GUARD):
        at = self.cur[c]
        self.cur[c] += size + guard
        assert self.cur[c] < FAMILY_END, "the family area of a contig is full"
        return at

    def plant(self, c, at, seq, rev=False):
        seq = rc(seq) if rev else bytes(seq)
        assert 0 <= at and at + len(seq) <= len(self.ref[c])
        self.ref[c][at:at + len(seq)] = np.frombuffer(seq, np.uint8)

    def cut(self, c, at, n):
        assert 0 <= at and at + n <= len(self.ref[c])
        return self.ref[c][at:at + n].tobytes()

    def sweep(self):
        self.n_sweep += 1
        return self.n_sweep

    def add(self, seq, family, sweep, step, ctx=0):
        for r in (0, 1):
            self.reads.append(Read(rc(seq) if r else bytes(seq), ctx, family, sweep, step, r))

    def minimizers(self, seq):
        """(end position, strand) of the minimizers of seq sketched alone: minimizers of seq in ANY context"""
        x, y = self.O.sketch(bytes(seq), W, K)
        return [(int(v & 0xffffffff) >> 1, int(v) & 1) for v in y]


def first_round_pivots(n):
    """the indices the first 8-ary round of the lower bound loads in a list of n > 8 entries"""
    step = (n + 7) >> 3
    return [(j + 1) * step - 1 for j in range(7) if (j + 1) * step - 1 < n]


def build_main(O, seed=TABLE_SEED):
    B = Builder(O, seed)
    rng = B.rng
    # ---- the 40-copy units, far from every locus: the tail of contig 2, both strands; r40 puts short lists' reads on the repeat list
    r40, ch40 = B.unit(100), B.unit(140)
    for i in range(40):
        B.plant(2, TAIL_AT + i * 2000, r40, rev=i % 3 == 1)
        B.plant(2, TAIL_AT + i * 2000 + 1000, ch40, rev=i % 3 == 2)
    p40 = r40[30:70]

    # ---- list: the grid.  Copy i of unit u in slot i * len(LIST_L) + u, slots running through the three contigs in ascending order
    per = (TAIL_AT - GRID_AT) // GRID_SLOT
    slot = lambda g: (g // per, GRID_AT + (g % per) * GRID_SLOT)
    assert 513 * len(LIST_L) <= 3 * per and len(LIST_L) * GRID_SLOT > 3 * MDX
    units = {L: B.unit() for L in LIST_L}
    for u, L in enumerate(LIST_L):
        for i in range(L):
            c, at = slot(i * len(LIST_L) + u)
            B.plant(c, at, units[L], rev=(i * 7 + u) % 3 == 0)
    list_reads = []      # filled in once every family has planted: the reads are cut from the reference
    for u, L in enumerate(LIST_L):
        ts = {0, 1, L - 2, L - 1}
        if L > 8:
            for ix in first_round_pivots(L):
                ts |= {ix - 1, ix, ix + 1}
        sw = B.sweep()
        for t in sorted(x for x in ts if 0 <= x < L):
            list_reads.append((sw, L, t, slot(t * len(LIST_L) + u), (t * 7 + u) % 3 == 0))

    # ---- nowin
    z = B.unit()
    for kind in ("below", "above", "elsewhere"):
        at = B.alloc(0, 16000)
        locus = at + (12000 if kind == "below" else 0)
        for i in range(3):
            if kind == "elsewhere":
                B.plant(1 + i % 2, B.alloc(1 + i % 2, 200), z, rev=i == 2)
            else:
                B.plant(0, at + (0 if kind == "below" else 6000) + i * 2500, z)
        sw = B.sweep()
        for f in range(50, 72, 2):
            B.add(p40 + B.cut(0, locus, f) + z[20:20 + 110 - f], "nowin", sw, f)
        z = B.unit()

    # ---- ladder: rungs below the locus, the read's flank on the low side of the unit so that a rung 600 below is always within 650 of it
    for c in (0, 1):
        for n in range(1, 6):
            v = B.unit()
            at = B.alloc(c, 600 * n + 400)
            a0 = at + 600 * n + 100
            for i in range(n + 1):
                B.plant(c, a0 - 600 * i, v)
            sw = B.sweep()
            for cutlen in (100, 105, 110):
                B.add(p40 + B.cut(c, a0 - 40, cutlen) + p40[:110 - cutlen], "ladder", sw, n)

    # ---- edge: a unit of its own per locus, so that the seed's list holds this locus alone (5 entries) or eight far pieces more (13)
    for c, far in ((0, 0), (1, 0), (0, 8), (1, 8), (0, 0), (1, 8)):
        sw = B.sweep()
        for delta in range(-3, 4):
            found = None
            while found is None:
                v = B.unit(110)
                for e0, strand in B.minimizers(v[:70]):      # strand bit 0: the occurrence word can equal the window's lower key
                    for s in range(0, W):
                        rs = e0 - K + 1 - s
                        if strand == 0 and rs >= 0 and (K - 1 + s, 0) in B.minimizers(v[rs:rs + 31]):
                            found = (v[rs:rs + 31], K - 1 + s)
            rung, e_in_rung = found
            at = B.alloc(c, 3200)
            a0 = at + 2900
            B.plant(c, a0, v)
            read = p40 + B.cut(c, a0 - 40, 110)
            # the lowest singleton the read will have: its lowest minimizer that starts in the 40 flank bases
            singles = [e for e, _ in B.minimizers(read) if 40 <= e - K + 1 < 80]
            lo_s = a0 - 40 + (min(singles) - 40) if singles else a0
            for i in range(4):
                B.plant(c, lo_s - MDX + delta - 600 * i - e_in_rung, rung)
            for i in range(far):      # a list of 13: four rungs, the unit, eight pieces on a later contig - the rung on the edge at index 3, a step boundary
                B.plant(2, B.alloc(2, 40, guard=60), rung)
            B.add(read, "edge", sw, delta)

    # ---- cap and ksize: tandems beside the locus
    for c, p in ((0, 31), (0, 35), (1, 38)):
        sw = B.sweep()
        for n in range(14, 20):
            t = B.unit(p)
            at = B.alloc(c, 900)
            B.plant(c, at + 120, t * n)
            B.add(B.cut(c, at + 120 - (QLEN - p - 10), QLEN), "cap", sw, n)
    for c, p, n in ((0, 31, 15), (1, 33, 16), (0, 36, 13), (1, 38, 16), (0, 34, 14), (1, 32, 12), (0, 37, 11), (1, 35, 15), (0, 33, 10), (1, 36, 16)):
        t = B.unit(p)
        at = B.alloc(c, 900)
        B.plant(c, at + 160, t * n)
        sw = B.sweep()
        # more of the tandem in the read: more seeds, each with n occurrences (below p + k bases of it: no k-mer twice); a shorter read: fewer
        # singletons.  Kept where the read's own sketch promises a K of about 64: n anchors per minimizer in the tandem, one per minimizer before it
        for part in range(31, p + K - 1):
            for g in (0, 6, 12, 18):
                read = B.cut(c, at + 160 - (QLEN - part) + g, QLEN - g)
                e = [x for x, _ in B.minimizers(read)]
                if 58 <= sum(n if x - K + 1 >= QLEN - g - part else 1 for x in e) <= 72:
                    B.add(read, "ksize", sw, part * 100 + g)

    # ---- apart: piece B slides along the reference; of the places tried, one is kept for every distance hi - lo = 4 MDX + d the read's
    # own sketch promises (the singletons are the minimizers that lie inside one piece)
    for c, (la, lb) in ((0, (45, 65)), (1, (65, 45)), (0, (55, 55)), (1, (50, 60)), (0, (60, 50)), (1, (55, 55))):
        at = B.alloc(c, 3200)
        sw = B.sweep()
        seen = set()
        for a_s in range(at, at + 30):
            for bs in range(at + 2560, at + 2640):
                e = [x for x, _ in B.minimizers(p40 + B.cut(c, a_s, la) + B.cut(c, bs, lb))]
                ea, eb = [x for x in e if 40 <= x - K + 1 and x < 40 + la], [x for x in e if 40 + la <= x - K + 1]
                if ea and eb:
                    d = (bs + eb[-1] - 40 - la) - (a_s + ea[0] - 40) - 4 * MDX
                    if -6 <= d <= 6 and d not in seen:
                        seen.add(d)
                        B.add(p40 + B.cut(c, a_s, la) + B.cut(c, bs, lb), "apart", sw, d)

    # ---- chimera
    def chimera(c, at, sw, js, rest, family="chimera", insert=False, from_end=False, qlen=QLEN):
        for j in js:
            piece = B.cut(c, at - j, j) if from_end else B.cut(c, at, j)
            if insert and j > 30:      # behind the first whole window where the piece is long: one anchor or two before it, the long run after it
                ins = 32 if j >= 70 else j // 2
                piece = piece[:ins] + bytes([subst(piece[ins])]) + piece[ins:j - 1]
            B.add(piece + rest[:(qlen or j + len(rest)) - j], family, sw, j)

    for c in (0, 1, 0):
        at = B.alloc(c, 200)
        chimera(c, at, B.sweep(), range(21, 150), ch40)
        chimera(c, at, B.sweep(), range(31, 150), ch40, insert=True)
    for c in (1, 2, 0, 1):      # the general path again where its margin changes sign
        chimera(c, B.alloc(c, 200), B.sweep(), range(60, 110), ch40, insert=True)
    for c in (0, 1, 2, 0, 1, 2, 0, 1):      # short unique pieces with ONE seed of the 40-copy unit behind them: U_out = k, the span of K decides.
        at, sw, seen = B.alloc(c, 200), B.sweep(), set()      # Start and length both move; one read is kept per span its own sketch promises
        for st in range(0, 12):
            for j in range(24, 62):
                e = [x for x, _ in B.minimizers(B.cut(c, at + st, j) + ch40[50:82]) if x < j]
                if e and e[-1] - e[0] not in seen and (e[-1] - e[0] < 6 or K - 4 <= e[-1] - e[0] <= K + 3):
                    seen.add(e[-1] - e[0])
                    B.add(B.cut(c, at + st, j) + ch40[50:82], "span", sw, e[-1] - e[0])
    # the margin aimed at: the unique piece's length and the unit's phase both move, and of the reads whose own sketch promises a margin of
    # -3 .. 3 (what the piece's minimizers span plus k, less what the unit's minimizers cover) one is kept per locus and value.  As it is
    # (the fast path), and with 32 bases from 1000 further on between the two (a second cluster in K: the general path)
    for c, second in ((0, False), (1, False), (2, False), (0, False), (0, True), (1, True), (2, True), (1, True)):
        at, sw, seen = B.alloc(c, 1300), B.sweep(), set()
        mid = B.cut(c, at + 1000, 32) if second else b""
        for ph in range(0, 24, 3):
            for j in range(50, 104):
                read = B.cut(c, at, j) + mid + ch40[ph:ph + QLEN - j - len(mid)]
                e = [x for x, _ in B.minimizers(read)]
                ea, eu = [x for x in e if x < j], [x for x in e if x - K + 1 >= j + len(mid)]
                if len(ea) >= 2 and eu:
                    cover = sum(min(K, b - a) for a, b in zip([eu[0] - K] + eu, eu))
                    mg = ea[-1] - ea[0] + K - cover
                    if -3 <= mg <= 3 and mg not in seen:
                        seen.add(mg)
                        B.add(read, "margin", sw, mg)
    at, other = B.alloc(0, 200), B.alloc(1, 200)
    chimera(0, at, B.sweep(), range(21, 150, 3), B.cut(1, other, 140))                  # the rest from another contig
    chimera(0, at, B.sweep(), range(21, 150, 3), rc(B.cut(0, B.alloc(0, 200), 140)))    # ... from the other strand of this one
    chimera(1, 0, B.sweep(), range(21, 150, 2), ch40)                                   # the locus at base 0 of a contig: the window clamps
    chimera(0, CONTIG_LEN[0], B.sweep(), range(21, 150, 2), ch40, from_end=True)        # ... and ends at a contig's last base

    # ---- fast
    for c in (0, 1):
        at = B.alloc(c, 200)
        base = B.cut(c, at, 110)
        sw = B.sweep()
        for d in range(0, 26):      # two substitutions d apart: the gap between the k-mers left and right of them grows with d
            r = bytearray(base)
            r[40], r[40 + d] = subst(r[40]), subst(r[40 + d])
            B.add(p40 + bytes(r), "fast", sw, d)
        sw = B.sweep()
        for n in range(16, 50, 2):      # every second base of n substituted: -8 and +2 in turn, the drop passes zdrop = 100 near n = 34
            r = bytearray(base)
            for i in range(35, 35 + n, 2):
                r[i] = subst(r[i])
            B.add(p40 + bytes(r), "fast", sw, 100 + n)

    for c in (0, 1, 2, 1):      # the bases outside the k-mers aimed at: one read per locus and promised value of 8 .. 17
        at, sw, seen = B.alloc(c, 200), B.sweep(), set()
        base = B.cut(c, at, 110)
        for s0 in range(34, 50):
            for d in range(0, 26):
                r = bytearray(base)
                r[s0], r[s0 + d] = subst(r[s0]), subst(r[s0 + d])
                e = [x for x, _ in B.minimizers(p40 + bytes(r)) if x - K + 1 >= 40 and not (x - K + 1 <= 40 + s0 <= x or x - K + 1 <= 40 + s0 + d <= x)]
                unc = sum(max(b - a - K, 0) for a, b in zip(e, e[1:]))
                if 8 <= unc <= 17 and unc not in seen:
                    seen.add(unc)
                    B.add(p40 + bytes(r), "fast", sw, 200 + unc)

    # ---- nseed
    sw = B.sweep()
    for m in range(30, 62, 2):
        B.add(r40[20:20 + m], "nseed", sw, m)
    sw = B.sweep()
    for a in range(0, 110, 5):      # 31 and 32 bases hold one whole window: one seed, now and then two
        B.add(ch40[a:a + 31 + a % 2], "nseed", sw, a)
    at = B.alloc(0, 500)
    sw = B.sweep()
    for u in range(21, 50, 2):
        B.add(p40 + B.cut(0, at, u), "nseed", sw, u)
    for c in (0, 1, 2):
        at = B.alloc(c, 600)
        sw = B.sweep()
        for n in range(380, 512):
            if 59 <= len(B.minimizers(p40 + B.cut(c, at, n - 40))) <= 69:
                B.add(p40 + B.cut(c, at, n - 40), "nseed", sw, n)

    # ---- nosingle
    sw = B.sweep()
    for i, (la, lb) in enumerate(((63, 64), (64, 65), (65, 72), (72, 73), (511, 512), (512, 513), (513, 63), (73, 511))):
        B.add(units[la][5:85] + units[lb][5:75], "nosingle", sw, i)

    # ---- list, cut now that nothing is planted any more
    for sw, L, t, (c, at), rev in list_reads:
        B.add(p40 + B.cut(c, at - 55, 110), "list", sw, t)
    return B


def build_high(O, seed=TABLE_SEED + 1):
    """the second reference: one contig, a unit planted 13 times (one copy per locus, the loci far apart), reads of 250 and 251 bases"""
    rng = np.random.default_rng(seed)
    ref = ACGT[rng.integers(0, 4, 300_000)].copy()
    h = ACGT[rng.integers(0, 4, 60)].tobytes()
    reads = []
    for i in range(HIGH_MID_OCC + 1):
        at = 10_000 + i * 20_000
        ref[at:at + 60] = np.frombuffer(h, np.uint8)
    for i in range(HIGH_MID_OCC + 1):
        at = 10_000 + i * 20_000
        for n in (250, 251):
            seq = ref[at - 90 - 3 * i:at - 90 - 3 * i + n].tobytes()
            for r in (0, 1):
                reads.append(Read(rc(seq) if r else seq, 1, "high", 1000, n, r))
    return [ref], reads


class Cases:
    """the table: reads, per context the contigs and the oracle's options and index, per read the model's Result and the oracle's flag"""

    def __init__(self, O):
        B = build_main(O)
        high_ref, high_reads = build_high(O)
        self.contigs = [B.ref, high_ref]
        self.reads = B.reads + high_reads
        self.opts = [O.preset("sr"), O.preset("sr")]
        self.opts[1].mid_occ, self.opts[1].max_occ, self.opts[1].q_occ_frac = HIGH_MID_OCC, HIGH_MAX_OCC, 0.0
        self.cidx = [O.Index.build(c, W, K) for c in self.contigs]
        self.table = [M.Table(*ix.dump()) for ix in self.cidx]
        self.model = [M.decide(O, self.opts[r.ctx], self.table[r.ctx], self.contigs[r.ctx], r.seq) for r in self.reads]
        self.flag = np.zeros(len(self.reads), np.uint8)
        for ctx in (0, 1):
            sel = [i for i, r in enumerate(self.reads) if r.ctx == ctx]
            bases, offs = batch([self.reads[i].seq for i in sel])
            self.flag[sel] = self.cidx[ctx].classify(self.opts[ctx], bases, offs, threads=8, want_trace=False)[0]

    def of(self, ctx):
        return [i for i, r in enumerate(self.reads) if r.ctx == ctx]

    def outcome(self, i):
        return self.model[i].outcome


def batch(seqs):
    bases = np.frombuffer(b"".join(seqs), np.uint8)
    offs = np.zeros(len(seqs) + 1, np.uint64)
    offs[1:] = np.cumsum([len(s) for s in seqs])
    return bases, offs


_CASES = None


def cases(O):
    global _CASES
    if _CASES is None:
        _CASES = Cases(O)
    return _CASES


def missing_edges(T, rc_):
    """the edges of the module's docstring that do NOT occur on both sides among the reads of orientation rc_ (0 forward, 1 reverse-complemented)"""
    rows = [(r, m, m.detail) for r, m in zip(T.reads, T.model) if r.rc == rc_]
    fam = lambda f: [(r, m, d) for r, m, d in rows if r.family == f]
    tried = lambda m: m.outcome in (M.K_SIZE, M.MARGIN, M.LEMMA, M.DECIDED, M.DECIDED_FILTERED, M.SCORE_TIE)
    k, mdx, zdrop = K, MDX, T.opts[0].zdrop
    want = {}
    # list: the unit's anchors of the adjacent copy are in K (all of K lies within the read's 110 reference bases), they decide the read, and
    # the singletons alone would not
    want["list: K is the adjacent copy, and decides"] = all(
        m.outcome == M.DECIDED and d["n_k"] > d["n_single_in"] and max(a[0] for a in m.K) - min(a[0] for a in m.K) < 110 for r, m, d in fam("list"))
    want["list: without the unit's anchors the read is not decided"] = sum(d["single_cov"] <= m.u_out for r, m, d in fam("list")) >= 0.9 * len(fam("list"))
    want["list: every L and every t"] = len({(r.sweep, r.step) for r, m, d in fam("list")}) == sum(
        len({t for t in {0, 1, L - 2, L - 1} | ({i + e for i in first_round_pivots(L) for e in (-1, 0, 1)} if L > 8 else set()) if 0 <= t < L}) for L in LIST_L)
    want["nowin: K holds the singletons only"] = len(fam("nowin")) >= 30 and all(tried(m) and d["n_k"] == d["n_single_in"] for r, m, d in fam("nowin"))
    want["ladder: three growths are taken"] = any(m.rounds == 4 and tried(m) for r, m, d in fam("ladder"))
    want["ladder: a fourth gives WINDOW"] = any(m.outcome == M.WINDOW and d["window"] == "rounds" for r, m, d in fam("ladder"))
    for n in (15, 16):
        want[f"cap: {n} in-window occurrences are taken"] = any(d.get("cap") == n and tried(m) for r, m, d in fam("cap"))
    for n in (17, 18):
        want[f"cap: {n} give WINDOW"] = any(d.get("cap") == n and m.outcome == M.WINDOW and d["window"] == "cap" for r, m, d in fam("cap"))
    for n in (63, 64):
        want[f"ksize: K of {n} anchors in one cluster is taken"] = any(d.get("n_k") == n and d.get("clusters") == [n] and m.outcome != M.K_SIZE for r, m, d in fam("ksize"))
    want["ksize: K of 65 anchors gives K_SIZE"] = any(d.get("n_k") == 65 and m.outcome == M.K_SIZE for r, m, d in fam("ksize"))
    want["apart: 4 max_dist_x is taken, two clusters in K"] = any(d.get("apart") == 4 * mdx and tried(m) and len(d["clusters"]) == 2 for r, m, d in fam("apart"))
    want["apart: one base more gives APART"] = any(d.get("apart") == 4 * mdx + 1 and m.outcome == M.APART for r, m, d in fam("apart"))
    want["apart: the second cluster wins"] = any(d.get("best_base", 0) > 0 for r, m, d in fam("apart"))
    want["apart: the first cluster wins"] = any(d.get("best_base") == 0 and len(d["clusters"]) == 2 for r, m, d in fam("apart"))
    ch = fam("chimera") + fam("margin")
    want["chimera, fast path: margin 0 gives MARGIN"] = any(d.get("codiagonal") and d["margin"] == 0 and m.outcome == M.MARGIN for r, m, d in ch)
    want["chimera, fast path: margin 1 decides"] = any(m.fast and d["margin"] == 1 and m.outcome == M.DECIDED for r, m, d in ch)
    want["chimera, general path: margin 0 gives MARGIN"] = any(not d.get("codiagonal", True) and d.get("margin_general") == 0 and m.outcome == M.MARGIN for r, m, d in ch)
    want["chimera, general path: margin 1 decides"] = any(not d.get("codiagonal", True) and d.get("margin_general") == 1 and m.outcome == M.DECIDED for r, m, d in ch)
    # ... and along one sweep of j: no margin at one j, decided at the next
    by = {(r.sweep, r.step): (m, d) for r, m, d in fam("chimera")}
    for path, general in (("fast", False), ("general", True)):
        want[f"chimera, {path} path: MARGIN and DECIDED at neighbouring j"] = any(
            m.outcome == M.MARGIN and (sw, j + e) in by and by[(sw, j + e)][0].outcome == M.DECIDED and ("n_chain" in by[(sw, j + e)][1]) == general
            for (sw, j), (m, d) in by.items() for e in (-1, 1))

    want["chimera: singletons elsewhere, tried"] = any(d.get("n_single_out", 0) > 0 and tried(m) for r, m, d in ch)
    want["chimera: the window clamps at base 0"] = any(d.get("wlo") == 0 and m.outcome == M.DECIDED for r, m, d in ch)
    want["chimera: the window passes a contig's end"] = any(d.get("whi", 0) >= CONTIG_LEN[d["rid"]] and tried(m) for r, m, d in ch if "rid" in d)
    want["chimera: a locus on the second contig"] = any(d.get("rid") == 1 and m.outcome == M.DECIDED for r, m, d in ch)
    fa = fam("fast")
    want["fast: at most ext_unc_max bases outside the k-mers"] = any(m.fast and d["unc"] == zdrop // T.opts[0].b and d["code"] == 1 for r, m, d in fa + ch)
    want["fast: one more takes the middle check"] = any(m.fast and d["unc"] == zdrop // T.opts[0].b + 1 and d["code"] == 2 and m.outcome == M.DECIDED for r, m, d in fa + ch)
    want["fast: the middle check passes just below zdrop"] = any(d.get("code") == 2 and zdrop - 8 < d["mid_drop"] <= zdrop and m.outcome == M.DECIDED for r, m, d in fa)
    want["fast: the middle check fails just above zdrop"] = any(d.get("code") == 2 and zdrop < d["mid_drop"] <= zdrop + 8 and m.outcome == M.LEMMA for r, m, d in fa)
    sp = fam("span")
    want["span: k - 1 declines although the margin is there"] = any(d.get("codiagonal") and d["span"] == k - 1 and d["margin"] > 0 and m.outcome == M.LEMMA for r, m, d in sp)
    want["span: k decides"] = any(d.get("codiagonal") and d["span"] == k and m.outcome == M.DECIDED for r, m, d in sp)
    ns = [(r, m, d) for r, m, d in rows if m.outcome != M.NOT_LISTED]
    for n, out in ((1, True), (2, False), (3, False), (63, False), (64, False), (65, True)):
        want[f"nseed: {n} seeds"] = any(d["n_seed"] == n and (m.outcome == M.N_SEED) == out for r, m, d in ns)
    want["nosingle"] = len(fam("nosingle")) >= 8 and all(m.outcome == M.NO_SINGLETON for r, m, d in fam("nosingle"))
    want["high: 250 bases decide with seeds filtered"] = sum(m.outcome == M.DECIDED_FILTERED and len(r.seq) == 250 for r, m, d in fam("high")) >= 8
    want["high: 251 bases give HIGH_SEED"] = sum(m.outcome == M.HIGH_SEED and len(r.seq) == 251 for r, m, d in fam("high")) >= 8
    # edge: an occurrence ON the window's lower key in the first round makes the window grow to WINDOW; the same construction one base lower does not
    by = {(r.sweep, r.step): (m, d) for r, m, d in fam("edge")}
    for name, sel in (("a list of at most 8", lambda n, i: n <= 8), ("a step boundary of a longer list", lambda n, i: n > 8 and i in first_round_pivots(n))):
        want[f"edge: on the lower key, {name}"] = any(
            m.outcome == M.WINDOW and any(rnd == 1 and sel(n, i) for rnd, n, i in d["on_lower_key"]) and (sw, st - 1) in by and tried(by[(sw, st - 1)][0])
            for (sw, st), (m, d) in by.items())
    return [name for name, ok in want.items() if not ok]
