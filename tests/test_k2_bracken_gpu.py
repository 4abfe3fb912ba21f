"""Abundance re-estimation on the GPU: sh_k2_distrib_add_device (the codes kernel and the window kernel), sh_k2_distrib_run,
`scrubby-hip k2-bracken-build` and `k2-bracken`.

Ground truth is the frozen oracle only: the per-k-mer codes are K2Table.classify_pair(..., want_taxa=True) on the table exported
from the GPU database, the windows are slid in plain Python (tests/k2_bracken_ref.py, written from the definitions in
include/scrubby_hip.h) and every distinct multiset is resolved by oracle.k2_resolve(taxa, counts, parent, W, 0.0).  Entries and
totals must be EQUAL: no tolerance, nothing left out.  PARITY WITH Bracken's own programs UNPINNED."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import k2_bracken_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "k2_build")
EXE = os.path.join(ROOT, "scrubby_amd", "scrubby-hip")
FIX_CAPACITY = 16_529
SEED = 0x5C2B0C01


@pytest.fixture(scope="module")
def K():
    from scrubby_amd import lib, k2
    lib.require_gpu()
    return k2


@pytest.fixture(scope="module")
def E():
    with open(os.path.join(GOLD, "expected.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def fixture_lib(E):
    """the records of tests/golden/k2_build/library.fna (read, never edited) and their internal taxa"""
    recs, parts = [], None
    with open(os.path.join(GOLD, "library.fna"), "rb") as f:
        for ln in f:
            ln = ln.rstrip(b"\r\n")
            if ln.startswith(b">"):
                parts = []
                recs.append(parts)
            elif parts is not None:
                parts.append(ln)
    recs = [b"".join(p) for p in recs]
    assert [len(s) for s in recs] == [r["length"] for r in E["records"]]
    return recs, [r["internal"] for r in E["records"]]


class Db:
    """a GPU database with the oracle's view of it: the exported table, the parent array, the options"""

    def __init__(self, K, oracle, db, min_hash=0):
        self.K, self.oracle, self.db = K, oracle, db
        cells, self.parent, self.ext = db.export()
        info = db.info()
        self.n_nodes, self.k = info["n_nodes"], info["k"]
        self.table = oracle.K2Table(cells, self.parent, info["value_bits"])
        self.o = oracle.k2_default_opts()
        self.o.value_bits = info["value_bits"]
        self.o.min_acceptable_hash = min_hash
        self._codes = {}

    def codes(self, seq):
        """one code per k-mer of a record, from the oracle (computed once per sequence)"""
        seq = bytes(seq)
        if seq not in self._codes:
            self._codes[seq] = self.table.classify_pair(self.o, seq, want_taxa=True)[1] if len(seq) >= self.k else np.zeros(0, np.uint32)
            assert len(self._codes[seq]) == max(len(seq) - self.k + 1, 0)
        return self._codes[seq]

    def reference(self, records, taxa, L, codes=None):
        W = L - self.k + 1
        if codes is None:
            codes = [self.codes(s) if 0 < t < self.n_nodes else [] for s, t in zip(records, taxa)]
        return R.distribution(codes, taxa, self.n_nodes, self.k, L,
                              lambda t, c: self.oracle.k2_resolve(t, c, self.parent, W, 0.0))


def as_maps(ent, tot):
    return {(int(g), int(m)): int(w) for g, m, w in ent}, {i: int(t) for i, t in enumerate(tot) if t}


def gpu_distribution(K, db, L, batches, misalign=0):
    """(entries, totals, summed stats) after one add_library call per batch of (records, taxa)"""
    d = K.KmerDistrib(db, L)
    try:
        st = {"n_windows": 0, "n_items": 0, "n_big": 0, "n_records": 0}
        for records, taxa in batches:
            s = d.add_library(records, taxa, misalign=misalign)
            for k in st:
                st[k] += s[k]
        ent, tot = d.entries(), d.totals()
        assert [tuple(x)[:2] for x in ent] == sorted(tuple(x)[:2] for x in ent) and len({tuple(x)[:2] for x in ent}) == len(ent)
        return (*as_maps(ent, tot), st)
    finally:
        d.close()


def check(K, D, L, records, taxa, misalign=0, codes=None):
    want_e, want_t = D.reference(records, taxa, L, codes)
    got_e, got_t, st = gpu_distribution(K, D.db, L, [(records, taxa)], misalign)
    print(f"L={L}: {len(want_e)} (genome, mapped) pairs, {sum(want_t.values())} windows, stats {st}")
    assert got_e == want_e and got_t == want_t
    S = K.distrib_stretch()
    n_win = [len(s) - L + 1 for s, t in zip(records, taxa) if 0 < t < D.n_nodes and len(s) >= L]
    assert st["n_windows"] == sum(n_win) == sum(want_t.values()) and st["n_items"] == sum((n + S - 1) // S for n in n_win)
    return want_e, want_t, st


@pytest.fixture(scope="module")
def fix(K, oracle, E, fixture_lib):
    """the k2_build fixture's database: its library inserted with insert_library at capacity 16 529"""
    records, taxa = fixture_lib
    tax = K.taxonomy_from_ncbi(os.path.join(GOLD, "nodes.dmp"), os.path.join(GOLD, "names.dmp"), os.path.join(GOLD, "seqid2taxid.map"), [1423])
    db = K.K2Db.create_from_taxonomy(K.default_opts(), FIX_CAPACITY, tax)
    db.insert_library(records, taxa)
    yield Db(K, oracle, db)
    db.close()


# ---- 1. the fixture ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [50, 100, 150])
def test_fixture_library(K, fix, fixture_lib, L):
    """seqE (20 bases), the two records without a taxon and the two records that pool under 1423 are part of the run"""
    records, taxa = fixture_lib
    want_e, want_t, st = check(K, fix, L, records, taxa)
    ext = fix.ext
    by_ext = {(int(ext[g]), int(ext[m])) for g, m in want_e}
    assert {(562, 543), (28901, 543), (562, 562), (28901, 28901)} <= by_ext          # the 600 shared bases map to the family
    if L <= 100:
        assert any(m == 0 for _, m in want_e)                                           # unclassified windows over the N run
    assert 0 not in want_t and set(want_t) == {t for s, t in zip(records, taxa) if t and len(s) >= L}


# ---- 2. edges of L and of the record length ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(K, oracle):
    """one random sequence, its two overlapping halves under two sibling taxa: calls change along it"""
    rng = np.random.default_rng(SEED)
    ref = rng.choice(np.frombuffer(b"ACGT", np.uint8), 4200).tobytes()
    db = K.K2Db.create(K.default_opts(), 20_011, [0, 0, 1, 2, 2], [0, 1, 10, 562, 28901], ["", "root", "a", "b", "c"], ["", "no rank", "genus", "species", "species"])
    db.insert_sequence(ref[:2600], 3)
    db.insert_sequence(ref[2200:], 4)
    yield Db(K, oracle, db), ref
    db.close()


def edge_records(ref, k, L, S):
    W = L - k + 1
    lens = {L - 1, L, L + 1}
    for j in (1, 2):
        for d in (-1, 0, 1):
            lens.add(L - 1 + j * S + d)          # the last stretch holds S - 1, S or 1 window starts
            lens.add(1024 * j + d)               # the codes kernel's segment
    recs = []
    for i, n in enumerate(sorted(x for x in lens if k - 1 <= x <= len(ref))):
        s = (131 * i) % (len(ref) - n + 1)
        recs.append(ref[s: s + n])
    n = min(max(L + 2 * S + 5, W + L + 5), len(ref) - 100)          # room for two N's W k-mers apart
    assert n > W + 1
    for at in ([0], [n - 1], [n // 3, n // 3 + W], [0, W], [n - 1 - W, n - 1]):      # W k-mers apart: an ambiguous code enters as one leaves
        b = bytearray(ref[100: 100 + n])
        for p in at:
            b[p] = ord("N")
        recs.append(bytes(b))
    return recs


@pytest.mark.parametrize("which", ["k", "k+1", "1024"])
def test_edges_of_read_length_and_record_length(K, small, which):
    D, ref = small
    L = {"k": D.k, "k+1": D.k + 1, "1024": 1024}[which]
    recs = edge_records(ref, D.k, L, K.distrib_stretch())
    assert any(len(r) == L - 1 for r in recs) and any(len(r) == L for r in recs)
    want_e, want_t, st = check(K, D, L, recs, [3] * len(recs))
    assert len(want_e) >= 2 and (L == 1024 or any(m == 0 for _, m in want_e))


@pytest.mark.parametrize("misalign", [1, 2, 3, 4, 5, 6, 7])
def test_misaligned_base_pointer(K, small, misalign):
    D, ref = small
    L = D.k + 1
    recs = edge_records(ref, D.k, L, K.distrib_stretch())
    check(K, D, L, recs, [3] * len(recs), misalign=misalign)


# ---- 3. many taxa per window: the exact fallback and the tie rule ------------------------------------------------------------------
@pytest.fixture(scope="module")
def mosaic(K, oracle):
    """a taxonomy of a root, 8 children and 24 leaves under each (201 taxa); every distinct minimizer of a random 3 000-base
    sequence under a random node"""
    parents = [0, 0] + [1] * 8 + [2 + i // 24 for i in range(8 * 24)]
    n = len(parents)
    rng = np.random.default_rng(SEED + 1)
    seq = rng.choice(np.frombuffer(b"ACGT", np.uint8), 3000).tobytes()
    db = K.K2Db.create(K.default_opts(), 8_209, parents, list(range(n)), [""] + [f"t{i}" for i in range(1, n)], ["", "no rank"] + ["genus"] * 8 + ["species"] * (n - 10))
    o = oracle.k2_default_opts()
    mins, amb = oracle.k2_scan(seq, o)
    keys = np.unique(mins[amb == 0])
    db.insert(keys, rng.integers(1, n, len(keys)).astype(np.uint32))
    yield Db(K, oracle, db), seq
    db.close()


@pytest.mark.parametrize("L", [60, 150, 300])
def test_many_taxa_per_window(K, mosaic, L):
    D, seq = mosaic
    W = L - D.k + 1
    codes = D.codes(seq)
    most = max(len(set(int(c) for c in codes[p: p + W]) - {0, R.AMBIGUOUS}) for p in range(len(codes) - W + 1))
    want_e, want_t, st = check(K, D, L, [seq], [5])
    print(f"L={L}: up to {most} distinct taxa per window, n_big {st['n_big']}, {want_e.get((5, 1), 0)} windows called root")
    assert most > 8
    if L == 150:
        assert st["n_big"] > 0           # a condition on the fixture: the LDS table holds fewer taxa than these windows do
        assert want_e.get((5, 1), 0) > 0         # calls that land at the root through tied scores


# ---- 4. batching does not matter ---------------------------------------------------------------------------------------------------
def test_batching_does_not_matter(K, fix, fixture_lib, tmp_path):
    records, taxa = fixture_lib
    L = 100
    one = gpu_distribution(K, fix.db, L, [(records, taxa)])
    three = gpu_distribution(K, fix.db, L, [(records[:2], taxa[:2]), (records[2:3], taxa[2:3]), (records[3:], taxa[3:])])
    assert one[:2] == three[:2] == fix.reference(records, taxa, L)
    dbdir = tmp_path / "db"
    dbdir.mkdir()
    fix.db.save(dbdir)
    res = K.build_kmer_distrib(dbdir, os.path.join(GOLD, "library.fna"), L, seqid2taxid=os.path.join(GOLD, "seqid2taxid.map"), chunk_bytes=1500)
    assert res["n_cuts"] >= 20 and res["n_batches"] >= 20 and res["n_records"] == len(records) and res["n_skipped"] == 2
    assert res["n_windows"] == sum(one[1].values()) and res["n_entries"] == len(one[0])
    cut = (dbdir / "database100mers.kmer_distrib").read_bytes()
    ent = np.array(sorted((g, m, w) for (g, m), w in one[0].items()), dtype=K.DISTRIB_DTYPE)
    tot = [one[1].get(i, 0) for i in range(fix.n_nodes)]
    K.write_kmer_distrib(ent, tot, fix.ext, L, tmp_path / "one.kmer_distrib")
    assert cut == (tmp_path / "one.kmer_distrib").read_bytes() == R.distrib_text(one[0], one[1], fix.ext).encode()
    back_e, back_t = as_maps(*K.read_kmer_distrib(dbdir / "database100mers.kmer_distrib", fix.ext))
    assert back_e == {k: v for k, v in one[0].items() if k[1]} and back_t == one[1]


def test_batch_beyond_the_code_scratch(K, fix, fixture_lib):
    """a batch of more bases than the accumulator's code scratch holds at first (2^22 codes; records without a taxon count too):
    the scratch grows and the batch is done again, and nothing of the first attempt is counted; a taxon outside the taxonomy is
    skipped like taxon 0"""
    records, taxa = fixture_lib
    filler = b"ACGT" * ((1 << 20) + 64)
    check(K, fix, 100, [filler] + records + [filler[:1000]], [0] + taxa + [fix.n_nodes])


# ---- 5. the codes agree with the hit lists -----------------------------------------------------------------------------------------
def test_codes_agree_with_the_hit_lists(K, fix, fixture_lib):
    """the same distribution from db.classify(..., hits=True) over the records as single reads: the two device paths cross"""
    records, taxa = fixture_lib
    bases = np.frombuffer(b"".join(records), dtype=np.uint8)
    offs = np.zeros(len(records) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(r) for r in records])
    out, st, (ho, he) = fix.db.classify(bases, offs, hits=True)
    codes = [np.repeat(he["code"][int(ho[i]): int(ho[i + 1])], he["count"][int(ho[i]): int(ho[i + 1])]) for i in range(len(records))]
    assert [len(c) for c in codes] == [max(len(r) - fix.k + 1, 0) for r in records]
    for c, r in zip(codes, records):
        assert np.array_equal(c, fix.codes(r))
    check(K, fix, 100, records, taxa, codes=codes)


# ---- 6. a down-sampled database ----------------------------------------------------------------------------------------------------
def test_min_acceptable_hash(K, oracle, fix, fixture_lib):
    records, taxa = fixture_lib
    tax = K.taxonomy_from_ncbi(os.path.join(GOLD, "nodes.dmp"), os.path.join(GOLD, "names.dmp"), os.path.join(GOLD, "seqid2taxid.map"), [1423])
    db = K.K2Db.create_from_taxonomy(K.default_opts(), FIX_CAPACITY, tax)
    try:
        db.set_min_acceptable_hash(1 << 63)
        db.insert_library(records, taxa)
        D = Db(K, oracle, db, min_hash=1 << 63)
        assert 0 < db.info()["size"] < fix.db.info()["size"]
        full = [fix.codes(r) for r in records]
        half = [D.codes(r) for r in records]
        assert sum(int((h == 0).sum()) for h in half) > sum(int((f == 0).sum()) for f in full)       # minimizers that are not looked up count as 0
        want_e, _, _ = check(K, D, 100, records, taxa)
        assert want_e != fix.reference(records, taxa, 100)[0]
    finally:
        db.close()


# ---- 7. the CLI pair ----------------------------------------------------------------------------------------------------------------
def test_cli_pair(K, E, fix, fixture_lib, tmp_path):
    records, taxa = fixture_lib
    L = 100
    dbdir = tmp_path / "db"
    dbdir.mkdir()
    fix.db.save(dbdir)
    p = subprocess.run([EXE, "k2-bracken-build", "-d", str(dbdir), "-i", os.path.join(GOLD, "library.fna"), "-m", os.path.join(GOLD, "seqid2taxid.map"), "-l", str(L)],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    dist = (dbdir / f"database{L}mers.kmer_distrib").read_text()
    want_e, want_t = fix.reference(records, taxa, L)
    assert dist == R.distrib_text(want_e, want_t, fix.ext)
    # a few hundred reads drawn from the library, a third of them from the 600 bases two species share
    rng = np.random.default_rng(SEED + 2)
    family = int(np.flatnonzero(fix.ext == 543)[0])
    shared = np.flatnonzero(fix.codes(records[0]) == family)          # k-mers of seqA inside the 600 bases it shares with seqB
    assert len(shared) > 400
    reads = []
    for i in range(360):
        r = records[int(rng.integers(0, 4))]
        s = int(rng.integers(0, len(r) - L))
        if i % 3 == 0:
            r, s = records[0], min(int(shared[int(rng.integers(0, len(shared)))]), len(records[0]) - L)
        reads.append(r[s: s + L])
    with open(tmp_path / "reads.fastq", "w") as f:
        for i, s in enumerate(reads):
            f.write(f"@r{i}\n{s.decode()}\n+\n{'I' * len(s)}\n")
    K.kraken_run([tmp_path / "reads.fastq"], [tmp_path / "out.fastq"], dbdir, taxa=["Bacteria"], workdir=tmp_path / "w")
    report = (tmp_path / "w" / "kraken.report").read_text()
    nodes = E["nodes"]
    cols = [[n[c] for n in nodes] for c in ("parent", "rank", "external", "name")]
    direct, lost = R.parse_report(report, cols[2])
    assert lost == 0 and sum(direct) == len(reads)
    want = R.estimate(*cols, direct, *R.parse_distrib(dist, cols[2]), "S", 10)
    p = subprocess.run([EXE, "k2-bracken", "-d", str(dbdir), "-r", str(tmp_path / "w" / "kraken.report"), "-l", str(L), "-o", str(tmp_path / "sample.bracken")],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "sample.bracken").read_text() == want["text"]
    print(want["text"])
    assert len(want["rows"]) >= 3 and want["reads_distributed"] > 0          # reads above the species level went down to species
    res = K.bracken(dbdir, tmp_path / "w" / "kraken.report", tmp_path / "lib.bracken", read_len=L)
    assert (tmp_path / "lib.bracken").read_text() == want["text"] and res["reads_distributed"] == want["reads_distributed"]
