"""kraken2's --minimum-base-quality and --quick on the GPU (k_k2_classify's QMASK / QUICK instances, sh_k2_classify_ex_*,
sh_kraken_run, the CLI's -C), against oracle/k2_oracle.c on host-masked bases and against the restated classify loop of
tests/test_k2_options_cpu.py.  The table is built on the GPU and exported, so both sides probe the same cells.
"""
import gzip
import json
import os
import subprocess

import numpy as np
import pytest

from tests import workloads as W
from tests.test_k2_options_cpu import Kraken2Loop, PHRED0, mask_bases, n_masked

pytestmark = pytest.mark.gpu

FIELDS = ("call", "total_kmers", "hit_groups")


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
    """the database of tests/test_k2_gpu.py: contigs 0-2 under three species (contig 0's first 200 kb also under a second
    Homo species), 64 pieces of contig 3 under 64 taxa, 300 k random filler keys"""
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


def phred(n, seed):
    """Phred+33 bytes: mostly 25-41, with low-quality runs of 3-30 bases at 2-14 (about one per two reads)"""
    rng = np.random.default_rng(seed)
    q = rng.integers(25, 42, n)
    for s in rng.integers(0, n, n // 300):
        q[s: s + int(rng.integers(3, 31))] = rng.integers(2, 15)
    return (q + PHRED0).astype(np.uint8)


def gopts(K, db, **kw):
    o = db.opts()
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def oopts(oracle, **kw):
    o = oracle.k2_default_opts()
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def same(g, c, ext):
    for f in FIELDS:
        assert np.array_equal(g[f], c[f]), f"{f}: {int((g[f] != c[f]).sum())} of {len(g)} differ"
    assert np.array_equal(g["taxid"], ext[c["call"]])


def same_loop(g, res, ext):
    for f in FIELDS:
        want = np.array([r[f] for r in res], dtype=np.uint32)
        assert np.array_equal(g[f], want), f"{f}: {int((g[f] != want).sum())} of {len(g)} differ"
    assert np.array_equal(g["taxid"], ext[np.array([r["call"] for r in res], dtype=np.int64)])


# ---- --minimum-base-quality --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paired", [False, True])
def test_masking_equals_the_oracle_on_masked_bases(K, oracle, db, table, cfg1, paired):
    P, R, ref, seqs, reads, off = cfg1
    t, ext = table
    n_rec = 10_000 if paired else 5_000                               # 5 000 pairs / 5 000 single reads
    base0 = 0 if paired else 10_000
    bases = reads[base0 * 150: (base0 + n_rec) * 150]
    o = off[: n_rec + 1]
    q = phred(len(bases), 31 + paired)
    plain, _ = db.classify(bases, o, paired=paired)
    n_called = {}
    for N in (0, 10, 20, 60):
        g, st = db.classify(bases, o, paired=paired, opts=gopts(K, db, min_base_quality=N), quals=q)
        c = t.classify(oopts(oracle), mask_bases(bases, q, N), o, paired=paired)
        same(g, c, ext)
        assert st["n_masked_bases"] == n_masked(q, o, N)
        assert st["n_kmers"] == int(c["total_kmers"].sum()) and st["n_probes"] == int(c["n_probes"].sum())
        n_called[N] = int((g["call"] != 0).sum())
        if N == 20:
            assert int((g["hit_groups"] != plain["hit_groups"]).sum()) > 0    # the masked runs cost hits
        if N == 0:
            assert np.array_equal(g, plain) and st["n_masked_bases"] == 0      # bit-identical to the entry without qualities
        if N == 60:
            assert n_called[N] == 0 and st["n_masked_bases"] == len(bases) and int(g["hit_groups"].max()) == 0
    assert n_called[0] >= n_called[20] > 0 and 0 < n_masked(q, o, 10) < n_masked(q, o, 20)


def test_masking_misaligned_pointers_and_device_entry(K, oracle, db, table, cfg1):
    """device-resident bases and qualities that start 7 bytes past an 8-byte boundary (both the same modulo 8)"""
    import torch
    from scrubby_amd.lib import ScrubbyHipError
    P, R, ref, seqs, reads, off = cfg1
    t, ext = table
    n = 1500
    bases = reads[: n * 150]
    q = phred(len(bases), 41)
    pad = np.frombuffer(b"GATTACA", dtype=np.uint8)
    hb = np.concatenate([pad, bases, np.full(64, ord("N"), np.uint8)])
    hq = np.concatenate([np.full(7, 0xFF, np.uint8), q, np.full(64, 0xFF, np.uint8)])
    d_b, d_q = torch.from_numpy(hb).cuda(), torch.from_numpy(hq).cuda()
    d_off = torch.from_numpy(off[: n + 1].astype(np.int64)).cuda()
    d_out = torch.zeros((n // 2, 4), dtype=torch.int32, device="cuda")
    st = db.classify_device(d_b[7:], d_off, n, True, d_out, opts=gopts(K, db, min_base_quality=20), d_quals=d_q[7:])
    assert d_b[7:].data_ptr() % 8 == 7
    g = d_out.cpu().numpy().view(K.RESULT_DTYPE).reshape(-1)
    c = t.classify(oopts(oracle), mask_bases(bases, q, 20), off[: n + 1], paired=True)
    same(g, c, ext)
    assert st["n_masked_bases"] == n_masked(q, off[: n + 1], 20) > 0
    # the batch entry with the records at odd offsets of the host arrays
    g2, _ = db.classify(hb[: 7 + len(bases)], off[: n + 1] + np.uint64(7), paired=True, opts=gopts(K, db, min_base_quality=20), quals=hq)
    assert np.array_equal(g2, g)
    # qualities at another address modulo 8 than the bases: refused, not misread
    with pytest.raises(ScrubbyHipError, match="modulo 8"):
        db.classify_device(d_b[7:], d_off, n, True, d_out, opts=gopts(K, db, min_base_quality=20), d_quals=d_q[4:])


def test_masking_many_taxa_overflow_path(K, oracle, db, table, cfg1):
    """long reads over the 64-taxon mosaic of contig 3: the units redone by the BIG pass are masked there as well"""
    P, R, ref, seqs, reads, off = cfg1
    t, ext = table
    recs = [bytes(seqs[3][900 + 50 * j: 900 + 50 * j + 6000]) for j in range(40)] + [bytes(seqs[0][1000 * j: 1000 * j + 3000]) for j in range(40)]
    bases = np.frombuffer(b"".join(recs), dtype=np.uint8)
    offs = np.zeros(len(recs) + 1, dtype=np.uint64); offs[1:] = np.cumsum([len(r) for r in recs])
    q = phred(len(bases), 43)
    g, st = db.classify(bases, offs, paired=False, opts=gopts(K, db, min_base_quality=20), quals=q)
    c = t.classify(oopts(oracle), mask_bases(bases, q, 20), offs, paired=False)
    assert st["n_overflow"] >= 30
    same(g, c, ext)
    assert st["n_probes"] == int(c["n_probes"].sum()) and st["n_masked_bases"] == n_masked(q, offs, 20)


def test_fasta_records_are_never_masked(K, oracle, db, table, cfg1):
    P, R, ref, seqs, reads, off = cfg1
    t, ext = table
    n = 2000
    bases, o = reads[: n * 150], off[: n + 1]
    plain, _ = db.classify(bases, o, paired=True)
    for N in (20, 250):
        g, st = db.classify(bases, o, paired=True, opts=gopts(K, db, min_base_quality=N), quals=np.full(len(bases), 0xFF, np.uint8))
        assert np.array_equal(g, plain) and st["n_masked_bases"] == 0
    # FASTQ and FASTA records mixed in one batch: odd records FASTA
    q = phred(len(bases), 47)
    for r in range(1, n, 2):
        q[int(o[r]): int(o[r + 1])] = 0xFF
    g, st = db.classify(bases, o, paired=True, opts=gopts(K, db, min_base_quality=20), quals=q)
    same(g, t.classify(oopts(oracle), mask_bases(bases, q, 20), o, paired=True), ext)
    assert st["n_masked_bases"] == n_masked(q, o, 20) > 0


# ---- --quick -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paired", [False, True])
def test_quick_mode_equals_the_restated_loop(K, oracle, db, table, cfg1, paired):
    P, R, ref, seqs, reads, off = cfg1
    t, ext = table
    n_rec = 4000 if paired else 2000
    base0 = 0 if paired else 12_000
    bases, o = reads[base0 * 150: (base0 + n_rec) * 150], off[: n_rec + 1]
    loop = Kraken2Loop(oracle, t, oopts(oracle))
    n_units = n_rec // 2 if paired else n_rec
    full, _ = db.classify(bases, o, paired=paired)
    for mhg in (0, 1, 2, 3):
        g, st = db.classify(bases, o, paired=paired, opts=gopts(K, db, quick=1, min_hit_groups=mhg))
        res = loop.classify_batch(bases, o, paired, quick=True, min_hit_groups=mhg)
        same_loop(g, res, ext)
        assert st["n_overflow"] == 0 and st["n_units"] == n_units
        assert st["n_kmers"] == sum(r["total_kmers"] for r in res) and st["n_probes"] == sum(r["n_probes"] for r in res)
        assert st["n_classified"] == sum(r["call"] != 0 for r in res) > n_units // 5
        assert int(g["total_kmers"].sum()) < int(full["total_kmers"].sum())      # the scans really stop early


def test_quick_mode_down_sampled_database_and_many_taxa(K, oracle, cfg1, db, table, tax):
    P, R, ref, seqs, reads, off = cfg1
    parents, externals, names, ranks, ids = tax
    # many-taxa reads: no hit list in quick mode, so nothing overflows
    t, ext = table
    recs = [bytes(seqs[3][900 + 50 * j: 900 + 50 * j + 6000]) for j in range(20)] + [bytes(seqs[0][1000 * j: 1000 * j + 3000]) for j in range(20)]
    bases = np.frombuffer(b"".join(recs), dtype=np.uint8)
    offs = np.zeros(len(recs) + 1, dtype=np.uint64); offs[1:] = np.cumsum([len(r) for r in recs])
    g, st = db.classify(bases, offs, paired=False, opts=gopts(K, db, quick=1, min_hit_groups=3))
    same_loop(g, Kraken2Loop(oracle, t, oopts(oracle)).classify_batch(bases, offs, False, quick=True, min_hit_groups=3), ext)
    assert st["n_overflow"] == 0
    # a down-sampled database: skipped minimizers are neither hits nor probes
    go = K.default_opts(); go.min_acceptable_hash = 3 << 62
    d = K.K2Db.create(go, 1_000_003, parents, externals, names, ranks)
    d.insert_sequence(seqs[0], ids["Homo sapiens"])
    cells, parent, ext2 = d.export()
    t2 = oracle.K2Table(cells, parent, 17)
    n = 3000
    for mhg in (1, 2):
        go.quick, go.min_hit_groups = 1, mhg
        g, st = d.classify(reads[: n * 150], off[: n + 1], paired=True, opts=go)
        res = Kraken2Loop(oracle, t2, oopts(oracle, min_acceptable_hash=3 << 62)).classify_batch(reads[: n * 150], off[: n + 1], True, quick=True, min_hit_groups=mhg)
        same_loop(g, res, ext2)
        assert st["n_probes"] == sum(r["n_probes"] for r in res) and int((g["call"] != 0).sum()) > 100
    d.close()


def test_quick_mode_with_masking(K, oracle, db, table, cfg1):
    P, R, ref, seqs, reads, off = cfg1
    t, ext = table
    n = 3000
    bases, o = reads[: n * 150], off[: n + 1]
    q = phred(len(bases), 53)
    masked = mask_bases(bases, q, 20)
    loop = Kraken2Loop(oracle, t, oopts(oracle))
    for paired in (False, True):
        for mhg in (1, 2):
            g, st = db.classify(bases, o, paired=paired, opts=gopts(K, db, quick=1, min_hit_groups=mhg, min_base_quality=20), quals=q)
            same_loop(g, loop.classify_batch(masked, o, paired, quick=True, min_hit_groups=mhg), ext)
            assert st["n_masked_bases"] == n_masked(q, o, 20) > 0


# ---- end to end: sh_kraken_run and the CLI ---------------------------------------------------------------------------------
def _write_pairs(tmp_path, reads, n_pairs):
    """plain ids (pairs removable from both files), random qualities, mate 2 gzipped and ragged"""
    q1 = phred(n_pairs * 150, 61)
    q2 = phred(n_pairs * 150, 62)
    with open(tmp_path / "a_1.fastq", "w") as f1, gzip.open(tmp_path / "a_2.fastq.gz", "wt") as f2:
        for i in range(n_pairs):
            s1, s2 = bytes(reads[(2 * i) * 150:(2 * i + 1) * 150]).decode(), bytes(reads[(2 * i + 1) * 150:(2 * i + 2) * 150]).decode()
            l2 = 100 + i % 50
            f1.write(f"@syn.{i} 1:N:0\n{s1}\n+\n{q1[150 * i: 150 * (i + 1)].tobytes().decode()}\n")
            f2.write(f"@syn.{i} 2:N:0\n{s2[:l2]}\n+\n{q2[150 * i: 150 * i + l2].tobytes().decode()}\n")
    # the same batch as the files hold: mates interleaved
    recs, quals = [], []
    for i in range(n_pairs):
        l2 = 100 + i % 50
        recs += [bytes(reads[(2 * i) * 150:(2 * i + 1) * 150]), bytes(reads[(2 * i + 1) * 150:(2 * i + 1) * 150 + l2])]
        quals += [q1[150 * i: 150 * (i + 1)].tobytes(), q2[150 * i: 150 * i + l2].tobytes()]
    bases = np.frombuffer(b"".join(recs), dtype=np.uint8)
    offs = np.zeros(len(recs) + 1, dtype=np.uint64); offs[1:] = np.cumsum([len(r) for r in recs])
    return bases, np.frombuffer(b"".join(quals), dtype=np.uint8), offs


def test_kraken_run_with_both_options(K, oracle, db, cfg1, tmp_path, monkeypatch):
    from scrubby_amd import lib as S
    P, R, ref, seqs, reads, off = cfg1
    dbdir = tmp_path / "db"; dbdir.mkdir()
    db.save(dbdir)
    n_pairs = 5000
    bases, quals, offs = _write_pairs(tmp_path, reads, n_pairs)
    monkeypatch.setenv("SCRUBBY_HIP_CHUNK_MB", "1")
    out = {}
    for name, env in (("stream", "0"), ("legacy", "1")):
        monkeypatch.setenv("SCRUBBY_HIP_LEGACY_HOST", env)
        w = tmp_path / f"w_{name}"
        res = K.kraken_run([tmp_path / "a_1.fastq", tmp_path / "a_2.fastq.gz"], [tmp_path / f"{name}_1.fastq", tmp_path / f"{name}_2.fastq.gz"], dbdir,
                           taxa=["Chordata"], taxa_direct=["9606"], workdir=w, json=tmp_path / f"{name}.json", read_ids=tmp_path / f"{name}.tsv",
                           confidence=0.1, min_base_quality=20, quick=True)
        rep = json.load(open(tmp_path / f"{name}.json"))
        out[name] = (res["reads_in"], res["reads_out"], res["reads_removed"], res["n_depleted_ids"],
                     open(w / "kraken.reads").read(), open(w / "kraken.report").read(),
                     open(tmp_path / f"{name}_1.fastq").read(), gzip.open(tmp_path / f"{name}_2.fastq.gz", "rt").read(),
                     sorted(open(tmp_path / f"{name}.tsv").read().split()), {k: v for k, v in rep.items() if k not in ("date", "output")})
    assert out["stream"] == out["legacy"]
    # the removed pairs are exactly the ones whose batch call falls under the selected taxa
    g, st = db.classify(bases, offs, paired=True, opts=gopts(K, db, confidence=0.1, quick=1, min_base_quality=20), quals=quals)
    lines = out["stream"][4].splitlines()
    assert [int(l.split("\t")[2]) for l in lines] == [int(x) for x in g["taxid"]]
    taxids = set(S.classifier_taxids(str(tmp_path / "w_stream" / "kraken.report"), taxa=["Chordata"], taxa_direct=["9606"]))
    hit = {f"syn.{i}" for i in range(n_pairs) if str(int(g["taxid"][i])) in taxids}
    assert out["stream"][3] == len(hit) > 500 and out["stream"][2] == 2 * len(hit)
    assert set(out["stream"][8]) - {"id"} == hit
    kept = {l[1:].split()[0] for l in out["stream"][6].splitlines() if l.startswith("@syn.")}
    assert kept == {f"syn.{i}" for i in range(n_pairs)} - hit
    # the outputs keep the original bases and qualities (only the classification saw the masked ones)
    def records(text):
        l = text.splitlines()
        return {l[i].split()[0]: tuple(l[i: i + 4]) for i in range(0, len(l), 4)}
    src, got = records(open(tmp_path / "a_1.fastq").read()), records(out["stream"][6])
    assert len(got) == n_pairs - len(hit) and all(src[k] == v for k, v in got.items())
    # and the options were applied: quick scans stop early, masked bases were seen
    g0, _ = db.classify(bases, offs, paired=True, opts=gopts(K, db, confidence=0.1))
    assert int(g["total_kmers"].sum()) < int(g0["total_kmers"].sum()) and st["n_masked_bases"] == n_masked(quals, offs, 20) > 0


def test_cli_classifier_args(K, db, cfg1, tmp_path):
    P, R, ref, seqs, reads, off = cfg1
    dbdir = tmp_path / "db"; dbdir.mkdir()
    db.save(dbdir)
    n = 1200
    q = phred(n * 150, 71)
    with open(tmp_path / "in.fastq", "w") as f:
        for i in range(n):
            f.write(f"@r{i}\n{bytes(reads[i * 150:(i + 1) * 150]).decode()}\n+\n{q[i * 150:(i + 1) * 150].tobytes().decode()}\n")
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scrubby_amd", "scrubby-hip")
    cargs = "--confidence 0.1 --minimum-base-quality 20 --quick"
    p = subprocess.run([exe, "reads", "-i", str(tmp_path / "in.fastq"), "-o", str(tmp_path / "out.fastq"), "-c", "kraken2", "-I", str(dbdir),
                        "-T", "Chordata", "-w", str(tmp_path / "w"), "-C", cargs, "-j", str(tmp_path / "r.json")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    assert "ignored" not in p.stderr
    K.kraken_run([tmp_path / "in.fastq"], [tmp_path / "lib.fastq"], dbdir, taxa=["Chordata"], workdir=tmp_path / "wl",
                 confidence=0.1, min_base_quality=20, quick=True)
    assert open(tmp_path / "w" / "kraken.reads").read() == open(tmp_path / "wl" / "kraken.reads").read()
    assert open(tmp_path / "out.fastq").read() == open(tmp_path / "lib.fastq").read()
    assert json.load(open(tmp_path / "r.json"))["settings"]["classifier_args"] == cargs
    # the "=" form, and a token the HIP backend does not use: named once on stderr, same exit status, same outputs
    p = subprocess.run([exe, "reads", "-i", str(tmp_path / "in.fastq"), "-o", str(tmp_path / "out2.fastq"), "-c", "kraken2", "-I", str(dbdir),
                        "-T", "Chordata", "-w", str(tmp_path / "w2"), "-C", "--use-mpa-style --confidence 0.1 --minimum-base-quality=20 --quick"],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    ign = [l for l in p.stderr.splitlines() if "ignored" in l]
    assert len(ign) == 1 and "--use-mpa-style" in ign[0] and "--quick" not in ign[0]
    assert open(tmp_path / "w2" / "kraken.reads").read() == open(tmp_path / "w" / "kraken.reads").read()
