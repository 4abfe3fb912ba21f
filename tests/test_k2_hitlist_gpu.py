"""Kraken 2's per-k-mer hit list on the GPU (k_k2_classify's HITS instances, sh_k2_classify_ex_* with hits, column 5 of kraken.reads)
against the per-k-mer taxa of oracle/k2_oracle.c, run-length encoded as tests/test_k2_hitlist_cpu.py restates it.  The
table is built on the GPU and exported, so both sides probe the same cells."""
import os
import subprocess

import numpy as np
import pytest

from tests import workloads as W
from tests.test_k2_hitlist_cpu import col5, rle
from tests.test_k2_options_cpu import mask_bases
from tests.test_k2_options_gpu import phred

pytestmark = pytest.mark.gpu

STATS = ("n_units", "n_classified", "n_probes", "n_kmers", "n_overflow", "n_masked_bases")


@pytest.fixture(scope="module")
def K():
    from scrubby_amd import lib, k2
    lib.require_gpu()
    return k2


@pytest.fixture(scope="module")
def cfg1(oracle):
    return W.cfg1(oracle, 20000)


@pytest.fixture(scope="module")
def tax():
    return W.k2_taxonomy()


@pytest.fixture(scope="module")
def db(K, cfg1, tax):
    """the database of tests/test_k2_gpu.py (three species over contigs 0-2, a 64-taxon mosaic of contig 3, random filler)"""
    P, R, ref, seqs, reads, off = cfg1
    parents, externals, names, ranks, ids = tax
    d = K.K2Db.create(K.default_opts(), 6_000_011, parents, externals, names, ranks)
    d.insert_sequence(seqs[0], ids["Homo sapiens"])
    d.insert_sequence(seqs[0][:200_000], ids["Homo heidelbergensis"])
    d.insert_sequence(seqs[1], ids["Pan troglodytes"])
    bact = [i for i, r in enumerate(ranks) if r == "species" and i > ids["Bacteria"] and names[i].startswith("species_")]
    d.insert_sequence(seqs[2], bact[0])
    for j in range(64):
        d.insert_sequence(seqs[3][1000 + 120 * j: 1000 + 120 * (j + 1) + 34], bact[1 + j % (len(bact) - 1)])
    d.insert_random(0xC0FFEE, 300_000, ids["Bacteria"], len(parents) - 1)
    yield d
    d.close()


@pytest.fixture(scope="module")
def table(oracle, db):
    cells, parent, ext = db.export()
    return oracle.K2Table(cells, parent, db.info()["value_bits"]), ext


def batch(recs):
    bases = np.frombuffer(b"".join(recs), dtype=np.uint8) if recs else np.zeros(0, np.uint8)
    offs = np.zeros(len(recs) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(r) for r in recs])
    return bases, offs


def oracle_lists(oracle, t, o, bases, offs, paired):
    """per unit: the oracle's result and its per-k-mer taxa, run-length encoded"""
    n_rec = len(offs) - 1
    res, lists = [], []
    for u in range(n_rec // 2 if paired else n_rec):
        rec = [2 * u, 2 * u + 1] if paired else [u]
        s = [bytes(bases[int(offs[r]): int(offs[r + 1])]) for r in rec]
        r, taxa = t.classify_pair(o, s[0], s[1] if paired else None, want_taxa=True)
        res.append(r); lists.append(rle(taxa))
    return res, lists


def check(K, db, oracle, t, ext, bases, offs, paired, o=None, go=None, quals=None):
    """the hit lists equal the oracle's, the counts add up to total_kmers, results and stats equal the plain entry's"""
    o = o if o is not None else oracle.k2_default_opts()
    out, st, (hoff, ent) = db.classify(bases, offs, paired=paired, opts=go, quals=quals, hits=True)
    plain, pst = db.classify(bases, offs, paired=paired, opts=go, quals=quals)
    assert np.array_equal(out, plain)
    assert {k: st[k] for k in STATS} == {k: pst[k] for k in STATS}
    obases = mask_bases(bases, quals, go.min_base_quality) if quals is not None else bases
    res, lists = oracle_lists(oracle, t, o, obases, offs, paired)
    assert len(hoff) == len(out) + 1 and int(hoff[-1]) == len(ent)
    bad = 0
    for u, want in enumerate(lists):
        e = ent[int(hoff[u]): int(hoff[u + 1])]
        got = [(int(c), int(n)) for c, n in zip(e["code"], e["count"])]
        bad += got != want
        if got != want and bad <= 3:
            print("unit", u, "got", got, "want", want)
        assert sum(n for c, n in got if c != K.HIT_BORDER) == int(out["total_kmers"][u])
        assert int(out["total_kmers"][u]) == res[u]["total_kmers"] and int(out["hit_groups"][u]) == res[u]["hit_groups"]
    assert bad == 0, f"{bad} of {len(lists)} hit lists differ"
    # column 5 as the writers print it
    strings = [K.format_hits(ent[int(hoff[u]): int(hoff[u + 1])], ext) for u in range(min(len(lists), 300))]
    assert strings == [col5(w, ext) for w in lists[:300]]
    return out, st, lists


def test_single_and_paired_ragged_mates(K, oracle, db, table, cfg1):
    P, R, ref, seqs, reads, off = cfg1
    t, ext = table
    rng = np.random.default_rng(3)
    recs = []
    for i in range(3000):
        s = bytearray(reads[i * 150:(i + 1) * 150])
        if i % 5 == 0:                                   # runs of N inside, at the start and at the end
            for _ in range(int(rng.integers(1, 4))):
                p, m = int(rng.integers(0, 150)), int(rng.integers(1, 12))
                s[p: p + m] = b"N" * len(s[p: p + m])
            if i % 10 == 0:
                s[:5], s[-4:] = b"NNNNN", b"NNNN"
        ln = 150 if i % 7 and i % 50 not in (20, 21) else int(rng.integers(0, 40))    # mates shorter than k, empty ones, both
        recs.append(bytes(s[:ln]))
    bases, offs = batch(recs)
    for paired in (False, True):
        out, st, lists = check(K, db, oracle, t, ext, bases, offs, paired)
        assert int((out["call"] != 0).sum()) > 100
        flat = [c for l in lists for c, _ in l]
        assert K.HIT_AMBIGUOUS in flat and 0 in flat
        if paired:
            assert all(sum(c == K.HIT_BORDER for c, _ in l) == 1 for l in lists) and [(K.HIT_BORDER, 0)] in lists
        else:
            assert [] in lists


def test_misaligned_device_entry(K, oracle, db, table, cfg1):
    import torch
    P, R, ref, seqs, reads, off = cfg1
    t, ext = table
    n = 1200
    bases = reads[: n * 150].copy()
    bases[np.arange(5, len(bases), 97)] = ord("N")
    hb = np.concatenate([np.frombuffer(b"GATTACA", dtype=np.uint8), bases, np.full(64, ord("N"), np.uint8)])
    d_b = torch.from_numpy(hb).cuda()
    d_off = torch.from_numpy(off[: n + 1].astype(np.int64)).cuda()
    d_out = torch.zeros((n // 2, 4), dtype=torch.int32, device="cuda")
    st, (hoff, ent) = db.classify_device_hits(d_b[7:], d_off, n, True, d_out)
    assert d_b[7:].data_ptr() % 8 == 7
    g = d_out.cpu().numpy().view(K.RESULT_DTYPE).reshape(-1)
    res, lists = oracle_lists(oracle, t, oracle.k2_default_opts(), bases, off[: n + 1], True)
    assert [r["call"] for r in res] == [int(x) for x in g["call"]]
    got = [[(int(c), int(k)) for c, k in zip(e["code"], e["count"])] for e in (ent[int(hoff[u]): int(hoff[u + 1])] for u in range(n // 2))]
    assert got == lists
    # the handle's device pointers: the same entries
    st2, (po, pe, nu, ne, h) = db.classify_device_hits(d_b[7:], d_off, n, True, d_out, to_host=False)
    try:
        assert nu == n // 2 and ne == len(ent) and po and pe
    finally:
        K.K2Db.free_hits(h)


def test_down_sampled_database(K, oracle, cfg1, tax):
    P, R, ref, seqs, reads, off = cfg1
    parents, externals, names, ranks, ids = tax
    go = K.default_opts(); go.min_acceptable_hash = 3 << 62
    d = K.K2Db.create(go, 1_000_003, parents, externals, names, ranks)
    d.insert_sequence(seqs[0], ids["Homo sapiens"])
    cells, parent, ext = d.export()
    t = oracle.K2Table(cells, parent, 17)
    o = oracle.k2_default_opts(); o.min_acceptable_hash = 3 << 62
    n = 2000
    out, st, lists = check(K, d, oracle, t, ext, reads[: n * 150], off[: n + 1], True, o=o, go=go)
    assert int((out["call"] != 0).sum()) > 50
    d.close()


@pytest.mark.parametrize("k, l", [(31, 31), (35, 20)])          # W = 1 and W = 16 instances
def test_other_k_l(K, oracle, cfg1, tax, k, l):
    P, R, ref, seqs, reads, off = cfg1
    parents, externals, names, ranks, ids = tax
    go = K.default_opts(); go.k, go.l, go.spaced_seed_mask = k, l, 0
    d = K.K2Db.create(go, 2_000_003, parents, externals, names, ranks)
    d.insert_sequence(seqs[0], ids["Homo sapiens"])
    d.insert_sequence(seqs[1], ids["Pan troglodytes"])
    d.insert_random(7, 100_000, ids["Bacteria"], len(parents) - 1)
    cells, parent, ext = d.export()
    t = oracle.K2Table(cells, parent, 17)
    o = oracle.k2_default_opts(); o.k, o.l, o.spaced_seed_mask = k, l, 0
    n = 1500
    bases = reads[: n * 150].copy()
    bases[np.arange(11, len(bases), 131)] = ord("N")
    for paired in (False, True):
        out, st, lists = check(K, d, oracle, t, ext, bases, off[: n + 1], paired, o=o, go=go)
        assert int((out["call"] != 0).sum()) > 50
    d.close()


def test_many_taxa_and_long_lists(K, oracle, db, table, cfg1):
    """units with more than 8 taxa (the BIG pass) and units with more entries than fit inline (the overflow pass)"""
    P, R, ref, seqs, reads, off = cfg1
    t, ext = table
    recs = [bytes(seqs[3][900 + 50 * j: 900 + 50 * j + 3000]) for j in range(30)]
    for i in range(100):                                 # an N every 40-55 bases: many A: entries, few taxa
        s = bytearray(seqs[0][5000 * i: 5000 * i + 1000])
        for p in range(3 + i % 7, len(s), 40 + i % 16):
            s[p] = ord("N")
        recs.append(bytes(s))
    recs += [bytes(reads[i * 150:(i + 1) * 150]) for i in range(200, 330)]
    bases, offs = batch(recs)
    out, st, lists = check(K, db, oracle, t, ext, bases, offs, False)
    assert st["n_overflow"] >= 20 and st["n_hits_redone"] >= 100
    assert max(len(l) for l in lists) > 50 and sum(len(l) <= 8 for l in lists) > 100
    out, st, lists = check(K, db, oracle, t, ext, bases, offs, True)
    assert st["n_hits_redone"] >= 50


def test_minimum_base_quality(K, oracle, db, table, cfg1):
    P, R, ref, seqs, reads, off = cfg1
    t, ext = table
    n = 2000
    bases, o = reads[: n * 150], off[: n + 1]
    q = phred(len(bases), 81)
    go = db.opts(); go.min_base_quality = 20
    for paired in (False, True):
        out, st, lists = check(K, db, oracle, t, ext, bases, o, paired, go=go, quals=q)
        assert st["n_masked_bases"] > 0 and any(c == K.HIT_AMBIGUOUS for l in lists for c, _ in l)


def test_quick_has_no_hit_list_entry(K, db, cfg1):
    from scrubby_amd.lib import ScrubbyHipError
    P, R, ref, seqs, reads, off = cfg1
    go = db.opts(); go.quick = 1
    with pytest.raises(ScrubbyHipError, match="quick"):
        db.classify(reads[:1500], off[:11], paired=False, opts=go, hits=True)


# ---- end to end: kraken.reads -------------------------------------------------------------------------------------------
def _fastq(path, ids, seqs):
    with open(path, "w") as f:
        for i, s in zip(ids, seqs):
            f.write(f"@{i}\n{s.decode()}\n+\n{'I' * len(s)}\n")


def test_kraken_reads_column5(K, oracle, db, table, cfg1, tmp_path, monkeypatch):
    P, R, ref, seqs, reads, off = cfg1
    t, ext = table
    dbdir = tmp_path / "db"; dbdir.mkdir()
    db.save(dbdir)
    n = 1500
    r1 = [bytes(reads[(2 * i) * 150:(2 * i + 1) * 150]) for i in range(n)]
    r2 = []
    for i in range(n):
        s = bytearray(reads[(2 * i + 1) * 150:(2 * i + 2) * 150][: 150 if i % 9 else 20 + i % 30])
        if i % 4 == 0 and len(s) > 60:
            s[40:47] = b"NNNNNNN"
        r2.append(bytes(s))
    ids = [f"p{i}" for i in range(n)]
    _fastq(tmp_path / "a_1.fastq", ids, r1)
    _fastq(tmp_path / "a_2.fastq", ids, r2)
    bases, offs = batch([x for p in zip(r1, r2) for x in p])
    res, lists = oracle_lists(oracle, t, oracle.k2_default_opts(), bases, offs, True)
    want_p = [col5(l, ext) for l in lists]
    sb, so = batch(r1)
    res_s, lists_s = oracle_lists(oracle, t, oracle.k2_default_opts(), sb, so, False)
    want_s = [col5(l, ext) for l in lists_s]
    for env in ("0", "1"):                 # the streaming writer and the collect-then-classify writer
        monkeypatch.setenv("SCRUBBY_HIP_LEGACY_HOST", env)
        w = tmp_path / f"w{env}"
        K.kraken_run([tmp_path / "a_1.fastq", tmp_path / "a_2.fastq"], [tmp_path / f"o{env}_1.fastq", tmp_path / f"o{env}_2.fastq"], dbdir,
                     taxa=["Chordata"], workdir=w)
        lines = [l.split("\t") for l in open(w / "kraken.reads").read().splitlines()]
        assert [l[4] for l in lines] == want_p and all(len(l) == 5 for l in lines)
        assert [int(l[2]) for l in lines] == [int(ext[r["call"]]) for r in res]
        ws = tmp_path / f"s{env}"
        K.kraken_run([tmp_path / "a_1.fastq"], [tmp_path / f"s{env}.fastq"], dbdir, taxa=["Chordata"], workdir=ws)
        assert [l.split("\t")[4] for l in open(ws / "kraken.reads").read().splitlines()] == want_s
        # --quick: "<taxid>:Q"
        wq = tmp_path / f"q{env}"
        K.kraken_run([tmp_path / "a_1.fastq", tmp_path / "a_2.fastq"], [tmp_path / f"q{env}_1.fastq", tmp_path / f"q{env}_2.fastq"], dbdir,
                     taxa=["Chordata"], workdir=wq, quick=True)
        ql = [l.split("\t") for l in open(wq / "kraken.reads").read().splitlines()]
        assert all(l[4] == f"{l[2]}:Q" for l in ql) and any(l[4] == "0:Q" for l in ql) and any(l[4] != "0:Q" for l in ql)
    assert open(tmp_path / "w0" / "kraken.reads").read() == open(tmp_path / "w1" / "kraken.reads").read()
    # the CLI writes the same file as the library
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scrubby_amd", "scrubby-hip")
    p = subprocess.run([exe, "reads", "-i", str(tmp_path / "a_1.fastq"), "-o", str(tmp_path / "c.fastq"), "-c", "kraken2", "-I", str(dbdir),
                        "-T", "Chordata", "-w", str(tmp_path / "wc")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    assert open(tmp_path / "wc" / "kraken.reads").read() == open(tmp_path / "s0" / "kraken.reads").read()
