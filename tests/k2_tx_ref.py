"""Translated search over a protein database, longhand in plain Python: the model the kernels are tested against.

Written from the rules as DESIGN.md §7 "Translated search" states them (recalled from Kraken 2's aa_translate.cc, mmscanner.cc
and classify.cc: PARITY UNPINNED), not from the kernels.  No state machine, no rolling state: a frame is a list of residues,
an l-mer is re-read from its l characters, a minimizer is the minimum over a slice.

  translate(seq, quals, min_qual)   the six frames of one record, as strings of residues
  aa_code(ch)                       the reduced 15-letter alphabet (None = ambiguous)
  scan_aa(residues, k, l, ...)      one entry per k-mer of a frame: the minimizer, or None for an ambiguous k-mer
  Table                             hash.k2d's cells: get, set (LCA on a key already there)
  classify(table, mates, ...)       one unit: (call, total_kmers, hit_groups)
"""
import math

MASK64 = (1 << 64) - 1
TOGGLE = 0xe37e28c4271b5a2d
K_AA, L_AA = 15, 12

# the standard code, indexed by 16 * b0 + 4 * b1 + b2 with A=0, C=1, G=2, T=3
CODE_TABLE = "KNKNTTTTRSRSIIMIQHQHPPPPRRRRLLLLEDEDAAAAGGGGVVVV*Y*YSSSS*CWCLFLF"
NT = {"A": 0, "C": 1, "G": 2, "T": 3, "a": 0, "c": 1, "g": 2, "t": 3}

# ResolveTree's threshold is ceil(confidence * (total_kmers + S)): Kraken 2 counts its frame-border markers in taxa.size() (5 for a
# read, 11 for a pair) and then subtracts 2 for a read, and 4 + 1 for a pair
S_READ, S_PAIR = 3, 6

AA_GROUPS = [("*UO", 0), ("A", 1), ("NQS", 2), ("C", 3), ("DE", 4), ("F", 5), ("G", 6), ("H", 7), ("IL", 8), ("K", 9), ("P", 10),
             ("R", 11), ("MV", 12), ("T", 13), ("W", 14), ("Y", 15)]
AA_CODE = {}
for letters, code in AA_GROUPS:
    for ch in letters:
        AA_CODE[ch] = code
        AA_CODE[ch.lower()] = code


def fmix64(k):
    k ^= k >> 33
    k = (k * 0xff51afd7ed558ccd) & MASK64
    k ^= k >> 33
    k = (k * 0xc4ceb9fe1a85ec53) & MASK64
    k ^= k >> 33
    return k


def aa_code(ch):
    """scanner code 0..15 of a residue character, None for every other byte (X included)"""
    return AA_CODE.get(ch)


def masked(q, min_qual):
    """--minimum-base-quality: a Phred+33 byte below the threshold; 0xFF never"""
    return q != 0xff and q - 33 < min_qual


def translate(seq, quals=None, min_qual=0):
    """six strings: forward frames 0, 1, 2, reverse frames 3, 4, 5.  seq: str; quals: bytes-like or None"""
    n = len(seq)
    if n < 3:
        return [""] * 6
    n_f = [0, 0, 0]
    for i in range(2, n):
        n_f[i % 3] += 1
    frames = [[None] * n_f[f % 3] for f in range(6)]
    for i in range(2, n):
        codon = seq[i - 2:i + 1]
        f, j = i % 3, (i - 2) // 3
        ok = all(c in NT for c in codon)
        if ok and quals is not None and min_qual > 0:
            ok = not any(masked(quals[p], min_qual) for p in (i - 2, i - 1, i))
        if ok:
            b = [NT[c] for c in codon]
            fwd = CODE_TABLE[16 * b[0] + 4 * b[1] + b[2]]
            r = [3 - b[2], 3 - b[1], 3 - b[0]]              # the reverse complement of the codon
            rev = CODE_TABLE[16 * r[0] + 4 * r[1] + r[2]]
        else:
            fwd = rev = "X"
        frames[f][j] = fwd
        frames[3 + f][n_f[f] - 1 - j] = rev
    return ["".join(fr) for fr in frames]


def frames_layout(seqs, quals=None, min_qual=0, as_letters=False):
    """what sh_k2_translate_* writes for a batch of records: (bytearray of 2 * n_bases + 8, mask of the bytes that are defined)"""
    n_bases = sum(len(s) for s in seqs)
    out, defined = bytearray(2 * n_bases + 8), bytearray(2 * n_bases + 8)
    at = 0
    for r, s in enumerate(seqs):
        q = None if quals is None else quals[r]
        p = 2 * at
        for fr in translate(s, q, min_qual):
            for ch in fr:
                if as_letters:
                    out[p] = ord(ch)
                else:
                    c = aa_code(ch)
                    out[p] = 0x80 if c is None else c
                defined[p] = 1
                p += 1
        at += len(s)
    return out, defined


def scan_aa(residues, k=K_AA, l=L_AA, spaced=0, toggle=TOGGLE):
    """one entry per k-mer of a frame (or of a library protein), in order: its minimizer, or None when the k-mer is ambiguous.
    An ambiguous character restarts the l-mer and the window: a k-mer's minimizer is the minimum over the l-mers that lie inside
    the k-mer and behind the last ambiguous character (none there: the k-mer is ambiguous)."""
    codes = [aa_code(ch) for ch in residues]
    out = []
    for e in range(k - 1, len(codes)):          # the k-mer ends at character e
        if codes[e] is None:
            out.append(None)
            continue
        first = e - k + 1
        for p in range(e, first - 1, -1):
            if codes[p] is None:
                first = p + 1
                break
        cands = []
        for s in range(first, e - l + 2):       # l-mers [s, s + l) inside [first, e]
            v = 0
            for c in codes[s:s + l]:
                v = v << 4 | c
            if spaced:
                v &= spaced
            cands.append(v ^ toggle)
        out.append(min(cands) ^ toggle if cands else None)
    return out


class Table:
    """the compact hash table of hash.k2d over a taxonomy given by its parent list (breadth-first ids, 0 = no taxon, 1 = root)"""

    def __init__(self, capacity, value_bits, parent):
        self.capacity, self.value_bits, self.parent = capacity, value_bits, list(parent)
        self.cells = [0] * capacity

    def lca(self, a, b):
        if a == 0 or b == 0:
            return a or b
        while a != b:
            if a > b:
                a = self.parent[a]
            else:
                b = self.parent[b]
        return a

    def is_ancestor(self, a, b):                # a is an ancestor of b, or b itself
        if a == 0 or b == 0:
            return False
        while b > a:
            b = self.parent[b]
        return a == b

    def set(self, key, taxon):
        h = fmix64(key)
        ck = h >> (32 + self.value_bits)
        i = h % self.capacity
        for _ in range(self.capacity):
            c = self.cells[i]
            if c == 0:
                self.cells[i] = ck << self.value_bits | taxon
                return
            if c >> self.value_bits == ck:
                self.cells[i] = ck << self.value_bits | self.lca(c & ((1 << self.value_bits) - 1), taxon)
                return
            i = (i + 1) % self.capacity
        raise RuntimeError("table full")

    def get(self, key):
        h = fmix64(key)
        ck = h >> (32 + self.value_bits)
        i = h % self.capacity
        for _ in range(self.capacity):
            c = self.cells[i]
            if c == 0:
                return 0
            if c >> self.value_bits == ck:
                return c & ((1 << self.value_bits) - 1)
            i = (i + 1) % self.capacity
        return 0

    def size(self):
        return sum(1 for c in self.cells if c)

    def add_protein(self, residues, taxon, k=K_AA, l=L_AA, spaced=0, toggle=TOGGLE):
        """the library side: every minimizer of the protein under `taxon`; returns the distinct keys it set"""
        keys = []
        for m in scan_aa(residues, k, l, spaced, toggle):
            if m is not None and m not in keys:
                keys.append(m)
                self.set(m, taxon)
        return keys


def classify(table, mates, confidence=0.0, min_hit_groups=2, k=K_AA, l=L_AA, spaced=0, toggle=TOGGLE, quals=None, min_qual=0):
    """one unit, mates = one or two nucleotide strings: (call, total_kmers, hit_groups).
    Frames 0..5 of mate 1, then of mate 2; last_minimizer is forgotten at the start of every frame; hit groups and taxon counts
    pool over all frames and both mates; an ambiguous k-mer counts in total_kmers and is never looked up."""
    counts, total, groups = {}, 0, 0
    for mi, seq in enumerate(mates):
        q = None if quals is None else quals[mi]
        for frame in translate(seq, q, min_qual):
            last_min, last_tax = None, 0
            for m in scan_aa(frame, k, l, spaced, toggle):
                total += 1
                if m is None:
                    continue
                if m != last_min:
                    last_tax = table.get(m)
                    last_min = m
                    if last_tax:
                        groups += 1
                if last_tax:
                    counts[last_tax] = counts.get(last_tax, 0) + 1
    s = S_PAIR if len(mates) == 2 else S_READ
    required = math.ceil(confidence * (total + s))
    best, best_score = 0, 0
    for t in sorted(counts):
        score = sum(c for t2, c in counts.items() if table.is_ancestor(t2, t))
        if score > best_score:
            best, best_score = t, score
        elif score == best_score:
            best = table.lca(best, t)
    score = counts.get(best, 0)
    while best and score < required:
        score = sum(c for t2, c in counts.items() if table.is_ancestor(best, t2))
        if score >= required:
            break
        best = table.parent[best]
    if best and groups < min_hit_groups:
        best = 0
    return best, total, groups


def n_taxa(table, mates, **kw):
    """distinct taxa a unit's k-mers count for (more than the kernel's in-LDS list: the overflow pass)"""
    seen = set()
    for seq in mates:
        for frame in translate(seq):
            for m in scan_aa(frame, **kw):
                if m is not None:
                    t = table.get(m)
                    if t:
                        seen.add(t)
    return len(seen)
