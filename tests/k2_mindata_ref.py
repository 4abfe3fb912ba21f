"""kraken2 --report-minimizer-data restated in Python over the unchanged oracle (in the manner of tests/chain_ref.py).

Neither kraken2's source nor a binary is at hand; the rules are recalled from classify.cc, reports.cc and hyperloglogplus.cc and
written down in DESIGN.md §7 "Minimizer data".  PARITY UNPINNED (oracle/k2_oracle.h).

Per unit the model walks oracle.k2_scan of each mate with kraken2's last_minimizer rule (a minimizer is looked up when it differs
from the last one looked up in this mate; an ambiguous span changes nothing, so a run resumed after it is not looked up again),
drops a minimizer whose hash is below min_acceptable_hash, looks the others up with K2Table.get and emits one (taxon, minimizer)
event per lookup that returns a taxon.  Masked bases (--minimum-base-quality) are 'x' before the scan.  With --quick the scan
stops at the lookup that brings the hit groups to the threshold: the events are the first min_hit_groups ones.

The model is accepted for an input only if, for every unit, its events number the oracle's hit_groups and its lookups the
oracle's n_probes (K2Table.classify_pair): `events` asserts that.
"""
import math

import numpy as np

P = 12
M = 1 << P
Q = 64 - P
MASK64 = (1 << 64) - 1


def fmix64(k):
    k ^= k >> 33; k = (k * 0xff51afd7ed558ccd) & MASK64
    k ^= k >> 33; k = (k * 0xc4ceb9fe1a85ec53) & MASK64
    k ^= k >> 33
    return k


def register_of(minimizer):
    """(index, rank) of a minimizer: the hash's top 12 bits; leading zeros of the other 52 + 1, 53 when they are all zero"""
    h = fmix64(int(minimizer))
    w = (h << P) & MASK64
    return h >> (64 - P), (64 - w.bit_length()) + 1 if w else Q + 1


def registers(minimizers):
    r = np.zeros(M, dtype=np.uint8)
    for m in minimizers:
        i, k = register_of(m)
        if k > r[i]:
            r[i] = k
    return r


def registers_np(values):
    """the same over a uint64 array, vectorised (the estimator tests insert millions of values)"""
    k = np.asarray(values, dtype=np.uint64).copy()
    k ^= k >> np.uint64(33); k *= np.uint64(0xff51afd7ed558ccd)
    k ^= k >> np.uint64(33); k *= np.uint64(0xc4ceb9fe1a85ec53)
    k ^= k >> np.uint64(33)
    idx = (k >> np.uint64(64 - P)).astype(np.int64)
    w = k << np.uint64(P)
    # leading zeros of w by binary search on the shifts
    lz = np.zeros(len(w), dtype=np.int64)
    x = w.copy()
    for s in (32, 16, 8, 4, 2, 1):
        top0 = (x >> np.uint64(64 - s)) == 0
        lz += np.where(top0, s, 0)
        x = np.where(top0, x << np.uint64(s), x)
    rank = np.where(w == 0, Q + 1, lz + 1).astype(np.uint8)
    r = np.zeros(M, dtype=np.uint8)
    np.maximum.at(r, idx, rank)
    return r


def _sigma(x):
    if x == 1.0:
        return math.inf
    y, z = 1.0, x
    while True:
        x *= x
        zp = z
        z += x * y
        y += y
        if zp == z:
            return z


def _tau(x):
    if x == 0.0 or x == 1.0:
        return 0.0
    y, z = 1.0, 1.0 - x
    while True:
        x = math.sqrt(x)
        zp = z
        y *= 0.5
        z -= (1.0 - x) * (1.0 - x) * y
        if zp == z:
            return z / 3.0


def estimate(regs):
    """Ertl's improved raw estimator over 4096 registers, in doubles"""
    C = np.bincount(np.asarray(regs, dtype=np.int64), minlength=Q + 2)
    assert len(C) == Q + 2, "a register above 53"
    m = float(M)
    z = m * _tau(1.0 - float(C[Q + 1]) / m)
    for k in range(Q, 0, -1):
        z = 0.5 * (z + float(C[k]))
    z += m * _sigma(float(C[0]) / m)
    d = 2.0 * math.log(2.0) * z
    return math.inf if d == 0.0 else m * m / d


def rounded(e):
    """the estimate as the report prints it"""
    return int(math.floor(e + 0.5))


class Model:
    def __init__(self, oracle, table, opts):
        self.O, self.t, self.o = oracle, table, opts
        self.cache = {}

    def _lookup(self, m):
        r = self.cache.get(m)
        if r is None:
            if self.o.min_acceptable_hash and fmix64(m) < self.o.min_acceptable_hash:
                r = (0, 0)
            else:
                r = (1, self.t.get(m))
            self.cache[m] = r
        return r

    def unit(self, mates):
        """(events, lookups) of one unit without --quick"""
        events, lookups = [], 0
        for seq in mates:
            mins, amb = self.O.k2_scan(seq, self.o)
            last = None
            for m, a in zip(mins.tolist(), amb.tolist()):
                if a or m == last:
                    continue
                last = m
                probed, taxon = self._lookup(m)
                lookups += probed
                if taxon:
                    events.append((taxon, m))
        return events, lookups

    def events(self, bases, offsets, paired, quick=False, min_hit_groups=None):
        """every event of a batch, per unit; asserts the acceptance condition against the oracle for every unit"""
        bases = np.asarray(bases, dtype=np.uint8)
        off = [int(x) for x in offsets]
        n_rec = len(off) - 1
        mhg = self.o.min_hit_groups if min_hit_groups is None else min_hit_groups
        out = []
        for u in range(n_rec // 2 if paired else n_rec):
            recs = (2 * u, 2 * u + 1) if paired else (u,)
            mates = [bases[off[r]: off[r + 1]].tobytes() for r in recs]
            ev, lookups = self.unit(mates)
            r = self.t.classify_pair(self.o, mates[0], mates[1] if paired else None)
            assert len(ev) == r["hit_groups"] and lookups == r["n_probes"], (u, len(ev), lookups, r)
            out.append(ev[:mhg] if quick and len(ev) >= mhg else ev)
        return out


class Expected:
    """what the accumulator must hold after the events of some units: n_minimizers, the distinct sets, and from them the
    registers, the clade values and the estimates"""

    def __init__(self, parent):
        self.parent = [int(p) for p in parent]
        self.n = len(self.parent)
        self.count = np.zeros(self.n, dtype=np.uint64)
        self.sets = [set() for _ in range(self.n)]

    def add(self, unit_events, times=1):
        for ev in unit_events:
            for taxon, m in ev:
                self.count[taxon] += times
                self.sets[taxon].add(m)
        return self

    def regs(self, t):
        return registers(self.sets[t])

    def subtree(self, t):
        return [x for x in range(1, self.n) if self._under(x, t)]

    def _under(self, x, t):
        while x > t:
            x = self.parent[x]
        return x == t

    def clade_count(self):
        c = self.count.copy()
        for i in range(self.n - 1, 1, -1):
            c[self.parent[i]] += c[i]
        return c

    def clade_sets(self):
        s = [set(x) for x in self.sets]
        for i in range(self.n - 1, 1, -1):
            s[self.parent[i]] |= s[i]
        return s

    def clade_regs(self):
        """registers of every clade: the element-wise maximum over the subtree"""
        r = np.zeros((self.n, M), dtype=np.uint8)
        for t in range(1, self.n):
            if self.sets[t]:
                r[t] = registers(self.sets[t])
        for i in range(self.n - 1, 1, -1):
            np.maximum(r[self.parent[i]], r[i], out=r[self.parent[i]])
        return r


def report_text(nodes_parent, first_child, child_count, names, ranks, externals, direct, clade_min, clade_distinct, total_units):
    """the 8-column report: the layout of sh_k2_write_report (depth-first, children by clade reads descending, ties by id, rank
    codes with a depth suffix, two spaces of indentation per level) with the two minimizer columns after "direct reads\""""
    n = len(nodes_parent)
    clade = [int(x) for x in direct]
    for i in range(n - 1, 1, -1):
        clade[nodes_parent[i]] += clade[i]
    letters = {"superkingdom": "D", "kingdom": "K", "phylum": "P", "class": "C", "order": "O", "family": "F", "genus": "G", "species": "S"}
    total = float(total_units) if total_units else 1.0
    lines = []
    unclassified = total_units - clade[1]
    if unclassified:
        lines.append("%6.2f\t%d\t%d\t0\t0\tU\t0\tunclassified" % (100.0 * unclassified / total, unclassified, unclassified))
    stack = [(1, "R", 0, 0)] if clade[1] else []
    while stack:
        t, code, cd, depth = stack.pop()
        letter = letters.get(ranks[t])
        if t != 1:
            if letter:
                code, cd = letter, 0
            else:
                cd += 1
        rc = code + (str(cd) if cd else "")
        lines.append("%6.2f\t%d\t%d\t%d\t%d\t%s\t%d\t%s%s" % (100.0 * clade[t] / total, clade[t], int(direct[t]), int(clade_min[t]), int(clade_distinct[t]), rc,
                                                          externals[t], "  " * depth, names[t]))
        kids = [c for c in range(first_child[t], first_child[t] + child_count[t]) if clade[c]]
        kids.sort(key=lambda c: (-clade[c], c))
        for c in reversed(kids):
            stack.append((c, code, cd, depth + 1))
    return "".join(l + "\n" for l in lines)
