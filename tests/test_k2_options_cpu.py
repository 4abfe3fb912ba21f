"""Kraken 2's classify loop restated in Python, with the two options the HIP arm honours besides the thresholds:
--minimum-base-quality (MaskLowQualityBases: a FASTQ base whose Phred score is below N becomes 'x') and --quick (the call is
the first hit k-mer once minimum_hit_groups hit groups are seen; no ResolveTree).

Neither kraken2's source nor a binary is at hand; these statements are the spec.  With --quick off the
restatement must reproduce oracle/k2_oracle.c exactly (call, total_kmers, hit_groups, probes): that pins it before
tests/test_k2_options_gpu.py uses it as the reference of the quick mode.  PARITY UNPINNED (oracle/k2_oracle.h).
"""
import numpy as np

PHRED0 = 33            # '!'
NEVER_MASKED = 0xFF    # the quality byte of a FASTA record


def mask_bases(bases, quals, min_quality):
    """MaskLowQualityBases over a batch: 'x' where (qual - '!') < N; 0xFF bytes (FASTA) are never masked."""
    b = np.array(bases, dtype=np.uint8, copy=True)
    if min_quality <= 0:
        return b
    q = np.asarray(quals, dtype=np.int32)[: len(b)]
    b[(q != NEVER_MASKED) & (q - PHRED0 < min_quality)] = ord("x")
    return b


def n_masked(quals, offsets, min_quality):
    q = np.asarray(quals, dtype=np.int32)[int(offsets[0]): int(offsets[-1])]
    return int(((q != NEVER_MASKED) & (q - PHRED0 < min_quality)).sum()) if min_quality > 0 else 0


class Kraken2Loop:
    """ClassifySequence of kraken2 (classify.cc), k-mer by k-mer, over a K2Table; the scanner is oracle.k2_scan."""

    def __init__(self, oracle, table, opts):
        self.O, self.t, self.o = oracle, table, opts
        self.lookups = {}

    def _lookup(self, m):
        """(probed, taxon) of one minimizer: not looked up when a down-sampled database drops its hash"""
        r = self.lookups.get(m)
        if r is None:
            if self.o.min_acceptable_hash and self.O.lib().k2o_hash(m) < self.o.min_acceptable_hash:
                r = (0, 0)
            else:
                r = (1, self.t.get(m))
            self.lookups[m] = r
        return r

    def classify(self, mates, quick=False, min_hit_groups=None, confidence=None):
        mhg = self.o.min_hit_groups if min_hit_groups is None else min_hit_groups
        conf = self.o.confidence if confidence is None else confidence
        total = groups = probes = 0
        hits = {}
        for seq in mates:
            mins, amb = self.O.k2_scan(seq, self.o)
            last_min, last_taxon = None, 0
            for m, a in zip(mins.tolist(), amb.tolist()):
                if a:                               # ambiguous span: counted, never looked up, never stops the scan
                    total += 1
                    continue
                if m != last_min:
                    probed, taxon = self._lookup(m)
                    probes += probed
                    last_min, last_taxon = m, taxon
                    groups += taxon != 0
                else:
                    taxon = last_taxon
                if taxon:
                    if quick and groups >= mhg:     # goto finished_searching: the rest of this mate and mate 2 are skipped
                        return dict(call=taxon, total_kmers=total, hit_groups=groups, n_probes=probes)
                    hits[taxon] = hits.get(taxon, 0) + 1
                total += 1
        call = 0
        if not quick and hits:
            call = self.O.k2_resolve(list(hits), list(hits.values()), self.t.parent, total, conf)
        if call and groups < mhg:
            call = 0
        return dict(call=call, total_kmers=total, hit_groups=groups, n_probes=probes)

    def classify_batch(self, bases, offsets, paired, quick=False, min_hit_groups=None):
        bases = np.asarray(bases, dtype=np.uint8)
        off = [int(x) for x in offsets]
        n_rec = len(off) - 1
        out = []
        for u in range(n_rec // 2 if paired else n_rec):
            recs = (2 * u, 2 * u + 1) if paired else (u,)
            out.append(self.classify([bases[off[r]: off[r + 1]].tobytes() for r in recs], quick, min_hit_groups))
        return out


def _toy(oracle):
    """Two sequences over the KAT tree (tests/test_k2_oracle_cpu.py): `a` -> taxon 7, `b` -> taxon 8, shared prefix -> LCA 4."""
    rng = np.random.default_rng(5)
    p = np.array([0, 0, 1, 1, 2, 2, 3, 4, 4, 6], dtype=np.uint32)
    o = oracle.k2_default_opts()
    o.value_bits = 9
    a = bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 4000)])
    b = a[:2000] + bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 2000)])
    c = bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 2000)])
    t = oracle.K2Table.empty(40_009, p, 9)
    for seq, tax in ((a, 7), (b, 8), (c, 9)):
        mins, amb = oracle.k2_scan(seq, o)
        for m in np.unique(mins[amb == 0]):
            t.set(int(m), tax)
    return t, o, (a, b, c)


def _reads(seqs, n, rng, length=150):
    """n reads cut from the sequences or random, with substitutions, N runs and ragged lengths"""
    out = []
    for i in range(n):
        kind = i % 5
        ln = int(length - rng.integers(0, 40)) if kind == 4 else length
        if kind == 3:
            s = bytearray(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, ln)])
        else:
            src = seqs[kind % 3]
            o = int(rng.integers(0, len(src) - ln))
            s = bytearray(src[o: o + ln])
        for j in rng.integers(0, ln, int(rng.integers(0, 4))):
            s[j] = ord("ACGT"[int(rng.integers(0, 4))])
        if rng.random() < 0.2:
            j, w = int(rng.integers(0, ln)), int(rng.integers(1, 6))
            s[j: j + w] = b"N" * len(s[j: j + w])
        out.append(bytes(s[:ln]))
    return out


def _batch(recs):
    bases = np.frombuffer(b"".join(recs), dtype=np.uint8)
    off = np.zeros(len(recs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r in recs])
    return bases, off


def _quals(n, rng):
    """Phred+33 bytes: mostly good, with low-quality runs"""
    q = rng.integers(25, 42, n)
    for s in rng.integers(0, n, n // 40):
        q[s: s + int(rng.integers(3, 25))] = rng.integers(2, 15)
    return (q + PHRED0).astype(np.uint8)


def _same(res, c):
    for f in ("call", "total_kmers", "hit_groups", "n_probes"):
        assert [r[f] for r in res] == [int(x) for x in c[f]], f


def test_restatement_equals_the_oracle_without_quick(oracle):
    t, o, seqs = _toy(oracle)
    rng = np.random.default_rng(11)
    recs = _reads(seqs, 3000, rng)
    bases, off = _batch(recs)
    for conf, mhg in ((0.0, 2), (0.0, 1), (0.4, 2), (0.0, 4)):
        o.confidence, o.min_hit_groups = conf, mhg
        loop = Kraken2Loop(oracle, t, o)
        for paired in (False, True):
            c = t.classify(o, bases, off, paired=paired, threads=4)
            _same(loop.classify_batch(bases, off, paired), c)
            assert int((c["call"] != 0).sum()) > 200
    # masked bases ('x') go down the ambiguous path of both
    o.confidence, o.min_hit_groups = 0.0, 2
    masked = mask_bases(bases, _quals(len(bases), rng), 20)
    c = t.classify(o, masked, off, paired=True, threads=4)
    _same(Kraken2Loop(oracle, t, o).classify_batch(masked, off, True), c)


def test_restatement_on_a_down_sampled_database(oracle):
    t, o, seqs = _toy(oracle)
    o.min_acceptable_hash = 1 << 63
    recs = _reads(seqs, 1500, np.random.default_rng(12))
    bases, off = _batch(recs)
    c = t.classify(o, bases, off, paired=True, threads=4)
    _same(Kraken2Loop(oracle, t, o).classify_batch(bases, off, True), c)


def test_masking_rules(oracle):
    q = np.array([33, 34, 52, 53, 255, 20, 74], dtype=np.uint8)        # Phred 0, 1, 19, 20, never, below '!', 41
    b = np.frombuffer(b"ACGTACG", dtype=np.uint8)
    assert mask_bases(b, q, 20).tobytes() == b"xxxTAxG"
    assert mask_bases(b, q, 0).tobytes() == b"ACGTACG"
    assert mask_bases(b, q, 250).tobytes() == b"xxxxAxx"                # 0xFF stays, whatever N
    assert n_masked(q, [0, 7], 20) == 4
    t, o, seqs = _toy(oracle)
    s = seqs[0][300:450]
    base = t.classify_pair(o, s)
    qq = np.full(150, 40 + PHRED0, np.uint8); qq[75] = 5 + PHRED0
    r, taxa = t.classify_pair(o, mask_bases(np.frombuffer(s, np.uint8), qq, 10).tobytes(), want_taxa=True)
    assert r["total_kmers"] == base["total_kmers"] == 116 and int((taxa == oracle.K2_AMBIG).sum()) == 31    # one masked base: like an N


def test_quick_mode_by_hand(oracle):
    t, o, (a, b, c) = _toy(oracle)
    loop = Kraken2Loop(oracle, t, o)
    s = a[2500:2650]                               # only in a: every k-mer hits taxon 7
    mins, amb = oracle.k2_scan(s, o)
    starts = [0] + [i for i in range(1, len(mins)) if mins[i] != mins[i - 1]]
    full = loop.classify([s])
    assert full["call"] == 7 and full["hit_groups"] == len(starts)
    for mhg in (0, 1):
        assert loop.classify([s], quick=True, min_hit_groups=mhg) == dict(call=7, total_kmers=0, hit_groups=1, n_probes=1)
    for mhg in (2, 3):                              # stops on the first k-mer of the mhg-th run
        assert loop.classify([s], quick=True, min_hit_groups=mhg) == dict(call=7, total_kmers=starts[mhg - 1], hit_groups=mhg, n_probes=mhg)
    # more groups than the read has: never stops, unclassified, every k-mer counted
    r = loop.classify([s], quick=True, min_hit_groups=len(starts) + 1)
    assert r == dict(call=0, total_kmers=116, hit_groups=len(starts), n_probes=len(starts))
    # a random mate 1 without hits, then mate 2 from b: the k-mers of mate 1 count, the mate border does not
    rnd = bytes(np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(9).integers(0, 4, 150)])
    assert loop.classify([rnd])["hit_groups"] == 0
    r = loop.classify([rnd, b[2500:2650]], quick=True, min_hit_groups=2)
    mins2, _ = oracle.k2_scan(b[2500:2650], o)
    second = next(i for i in range(1, len(mins2)) if mins2[i] != mins2[i - 1])
    assert r["call"] == 8 and r["total_kmers"] == 116 + second and r["hit_groups"] == 2
    # the first hit decides, not the majority: a read starting in the shared prefix (LCA 4) and going on into a (7)
    s = a[1900:2150]
    assert loop.classify([s])["call"] == 7
    assert loop.classify([s], quick=True, min_hit_groups=2)["call"] == 4
    # ambiguous k-mers never stop the scan: N at the start, the stop moves behind them
    s = a[2500:2560] + b"N" + a[2561:2650]
    mins, amb = oracle.k2_scan(s, o)
    first_amb = int(np.argmax(amb))
    n_amb = int(amb.sum())
    assert n_amb > 0 and amb[first_amb: first_amb + n_amb].all()
    starts, last = [], None                        # first k-mers of the runs (consecutive equal minimizers, across ambiguity)
    for i in range(len(mins)):
        if not amb[i] and mins[i] != last:
            starts.append(i); last = mins[i]
    before = sum(1 for i in starts if i < first_amb)
    r = loop.classify([s], quick=True, min_hit_groups=before + 1)
    # stops on a hit run behind the ambiguous span (the first windows after it may miss: they are not the reference's)
    assert r["call"] == 7 and r["hit_groups"] == before + 1 and r["total_kmers"] in starts and r["total_kmers"] >= first_amb + n_amb
