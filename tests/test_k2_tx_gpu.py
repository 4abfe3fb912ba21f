"""Translated search on the GPU against the longhand model (tests/k2_tx_ref.py): k_k2_translate, the protein form of
k_k2_classify over the committed protein database (tests/golden/k2_protdb, written byte by byte by make_k2_protdb.py), a
database made through the C ABI, the refusals, the build from an amino-acid library, and `reads -c kraken2` end to end.
PARITY UNPINNED: the model restates the rules as DESIGN.md §7 "Translated search" recalls them."""
import json
import os
import shutil
import struct

import numpy as np
import pytest

from tests import k2_tx_ref as M
from tests.test_k2_tx_cpu import _records, check_translation

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
PROTDB = os.path.join(GOLD, "k2_protdb")
BUILD = os.path.join(GOLD, "k2_prot_build")
THRESHOLDS = [(c, g) for c in (0.0, 0.5, 1.0) for g in (1, 2, 3)]


@pytest.fixture(scope="module")
def K():
    from scrubby_amd import lib, k2
    lib.require_gpu()
    return k2


@pytest.fixture(scope="module")
def EXP():
    return json.load(open(os.path.join(GOLD, "k2_protdb_expected.json")))


@pytest.fixture(scope="module")
def db(K):
    d = K.K2Db.open(PROTDB)
    yield d
    d.close()


@pytest.fixture(scope="module")
def table(EXP):
    h = open(os.path.join(PROTDB, "hash.k2d"), "rb").read()
    t = M.Table(EXP["capacity"], EXP["value_bits"], EXP["parents"])
    t.cells = list(struct.unpack_from("<%dI" % EXP["capacity"], h, 32))
    return t


def pack(units):
    """units: lists of one or of two mates (not mixed) -> bases, offsets, paired"""
    paired = len(units[0]) == 2
    assert all(len(u) == len(units[0]) for u in units)
    recs = [m.encode() for u in units for m in u]
    off = np.zeros(len(recs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r in recs], dtype=np.uint64)
    return np.frombuffer(b"".join(recs) + b"N" * 8, dtype=np.uint8), off, paired


def run(K, db, units, conf=0.0, mhg=2):
    bases, off, paired = pack(units)
    o = db.opts()
    o.confidence, o.min_hit_groups = conf, mhg
    return db.classify(bases, off, paired=paired, opts=o)


def same(got, want, ext):
    """want: (call, total_kmers, hit_groups) per unit"""
    assert [(int(g["call"]), int(g["total_kmers"]), int(g["hit_groups"])) for g in got] == [tuple(w) for w in want]
    assert [int(g["taxid"]) for g in got] == [ext[w[0]] for w in want]


# ---- k_k2_translate ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("as_letters", [False, True])
def test_translate_device_matches_the_model(K, as_letters):
    recs = _records()
    out, off = K.translate_device([r.encode() for r in recs], as_letters=as_letters)
    check_translation(out, off, recs, as_letters=as_letters)
    host, _ = K.translate_host([r.encode() for r in recs], as_letters=as_letters)
    assert np.array_equal(out, host)                       # the unwritten bytes stay zero on both sides


def test_translate_device_every_alignment_and_record_count(K):
    recs = _records()
    for mis in range(8):                                   # the first base at every address modulo 8
        out, off = K.translate_device([r.encode() for r in recs[10:]], misalign=mis)
        check_translation(out, off, recs[10:])
    many = [recs[10 + i % 7] for i in range(65)]           # 44 .. 152 bases: a wave's 64 bases span one to three records
    for n in (1, 63, 64, 65):
        out, off = K.translate_device([r.encode() for r in many[:n]])
        check_translation(out, off, many[:n])
    spans = [recs[10 + i % 7] for i in range(130)]         # 13 000 bases: the wave's spans of 4 096 bases end inside records
    out, off = K.translate_device([r.encode() for r in spans], misalign=5)
    check_translation(out, off, spans)
    tiny = [recs[i % 10] for i in range(200)]              # records of 0 .. 9 bases: many records inside one wave's span
    out, off = K.translate_device([r.encode() for r in tiny])
    check_translation(out, off, tiny)


def test_translate_device_quality_threshold(K):
    recs = _records()[14:17]
    quals = [bytes([ord("I")] * len(r)) for r in recs]
    q1 = bytearray(quals[1]); q1[70] = ord("!") + 9; quals[1] = bytes(q1)
    for mis in (0, 3):
        out, off = K.translate_device([r.encode() for r in recs], quals=quals, min_qual=10, misalign=mis)
        check_translation(out, off, recs, quals, 10)
    out, off = K.translate_device([r.encode() for r in recs], quals=quals, min_qual=0)
    check_translation(out, off, recs)


# ---- classification over the committed database -----------------------------------------------------------------------------------
def test_open_reports_a_protein_database(K, db, EXP):
    o, i = db.opts(), db.info()
    assert (o.protein, o.k, o.l, o.spaced_seed_mask) == (1, 15, 12, 0) and o.toggle_mask == M.TOGGLE
    assert (i["capacity"], i["size"], i["value_bits"], i["n_nodes"]) == (EXP["capacity"], EXP["size"], EXP["value_bits"], len(EXP["parents"]))
    hdr = db.inspect_header()
    assert "protein db, k = 15, l = 12" in hdr and "# Spaced mask = " + "0" * 48 + "\n" in hdr


@pytest.mark.parametrize("ti", range(len(THRESHOLDS)))
def test_classify_matches_expected(K, db, EXP, ti):
    conf, mhg = THRESHOLDS[ti]
    for n_mates in (1, 2):
        units = [u for u in EXP["units"] if len(u["mates"]) == n_mates]
        assert len(units) >= 4
        got, st = run(K, db, [u["mates"] for u in units], conf, mhg)
        want = [(u["results"][ti]["call"], u["results"][ti]["total_kmers"], u["results"][ti]["hit_groups"]) for u in units]
        assert all(u["results"][ti]["confidence"] == conf and u["results"][ti]["min_hit_groups"] == mhg for u in units)
        same(got, want, EXP["external"])
        assert st["n_units"] == len(units) and st["n_kmers"] == sum(w[1] for w in want) and st["n_classified"] == sum(1 for w in want if w[0])
        assert st["n_long_units"] == 0 and st["ms_translate"] > 0.0
        # the 600-base unit counts for more taxa than the in-LDS list holds: the BIG pass redoes it
        assert st["n_overflow"] == sum(1 for u in units if u["n_taxa"] > 8) >= 1
        # (one frame of six carries the protein: a confidence of 0.5 or more leaves every unit unclassified, by the rules)
        assert any(w[0] for w in want) == (conf == 0.0)


def test_expected_cases_are_what_they_say(EXP):
    u = {x["what"][:8]: x for x in EXP["units"]}
    assert u["44 bases"]["results"][1]["total_kmers"] == 0 and u["44 bases"]["results"][1]["call"] == 0
    assert u["45 bases"]["results"][0]["total_kmers"] == 2 and u["47 bases"]["results"][0]["total_kmers"] == 6
    names = EXP["names"]
    assert names[u["a stretc"]["results"][1]["call"]] == "Alphavirus"
    assert names[u["shared b"]["results"][1]["call"]] == "Viruses"
    assert u["random: "]["results"][0]["call"] == 0


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_batch_sizes(K, db, EXP, n):
    singles = [u for u in EXP["units"] if len(u["mates"]) == 1]
    units = [singles[i % len(singles)] for i in range(n)]
    got, st = run(K, db, [u["mates"] for u in units], 0.0, 2)
    same(got, [(u["results"][1]["call"], u["results"][1]["total_kmers"], u["results"][1]["hit_groups"]) for u in units], EXP["external"])
    pairs = [u for u in EXP["units"] if len(u["mates"]) == 2]
    units = [pairs[i % len(pairs)] for i in range(n)]
    got, st = run(K, db, [u["mates"] for u in units], 0.0, 2)
    same(got, [(u["results"][1]["call"], u["results"][1]["total_kmers"], u["results"][1]["hit_groups"]) for u in units], EXP["external"])


def test_empty_and_600_base_units_in_one_wave(K, db, table, EXP):
    big = next(u for u in EXP["units"] if u["what"].startswith("600 bases"))["mates"][0]
    own = EXP["s_decides"]["mates"][0]
    units = [[""], [big], ["AC"], [own], [""], [big[:299]], [own[:45]]] + [[own[i:]] for i in range(1, 20)]
    got, st = run(K, db, units, 0.0, 1)
    same(got, [M.classify(table, u, 0.0, 1) for u in units], EXP["external"])
    assert got["total_kmers"][0] == 0 and got["call"][0] == 0 and st["n_overflow"] >= 1
    # ... and as pairs: an empty mate beside a 600-base one
    pairs = [["", big], [big, ""], [own, big], ["", ""]]
    got, st = run(K, db, pairs, 0.0, 1)
    same(got, [M.classify(table, u, 0.0, 1) for u in pairs], EXP["external"])


def test_s_decides_the_call(K, db, table, EXP):
    sd = EXP["s_decides"]
    got, _ = run(K, db, [sd["mates"]], sd["confidence"], sd["min_hit_groups"])
    assert int(got["call"][0]) == sd["call"] != sd["call_without_s"]
    # a pair of the same read: S = 6 over twice the k-mers
    pair = [sd["mates"][0], sd["mates"][0]]
    for conf in (sd["confidence"] - 0.004, sd["confidence"] - 0.002, sd["confidence"], sd["confidence"] + 0.002):
        got, _ = run(K, db, [pair], conf, 1)
        same(got, [M.classify(table, pair, conf, 1)], EXP["external"])


def test_quality_masking_happens_at_translation(K, db, table, EXP):
    own = EXP["s_decides"]["mates"][0]
    bases, off, _ = pack([[own], [own]])
    q = bytearray(b"I" * (2 * len(own)) + b"\xff" * 8)
    q[len(own) + 60] = ord("!") + 5                        # one base of the second read below the threshold
    o = db.opts(); o.min_hit_groups, o.min_base_quality = 1, 10
    got, st = db.classify(bases, off, paired=False, opts=o, quals=np.frombuffer(bytes(q), dtype=np.uint8))
    quals = [bytes(q[:len(own)]), bytes(q[len(own):2 * len(own)])]
    want = [M.classify(table, [own], 0.0, 1, quals=[quals[i]], min_qual=10) for i in range(2)]
    same(got, want, EXP["external"])
    assert "X" in "".join(M.translate(own, quals[1], 10)) and "X" not in "".join(M.translate(own, quals[0], 10))
    assert want[1][1] == want[0][1] and st["n_masked_bases"] == 1           # the k-mers over the X still count in total_kmers


# ---- a database made through sh_k2_create / sh_k2_insert_device ---------------------------------------------------------------------
def test_created_database_and_a_dna_database_beside_it(K, db, EXP, tmp_path):
    o = K.default_protein_opts()
    o.value_bits = EXP["value_bits"]
    cap = 4099
    made = K.K2Db.create(o, cap, EXP["parents"], EXP["external"], EXP["names"], EXP["ranks"])
    t = M.Table(cap, EXP["value_bits"], EXP["parents"])
    keys, taxa = [], []
    for s, p in EXP["proteins"].items():
        for m in t.add_protein(p, int(s)):
            keys.append(m); taxa.append(int(s))
    made.insert(np.array(keys, dtype=np.uint64), np.array(taxa, dtype=np.uint32))
    assert made.opts().protein == 1 and made.info()["size"] == t.size()
    units = [u["mates"] for u in EXP["units"] if len(u["mates"]) == 1]
    for conf, mhg in ((0.0, 2), (0.5, 1)):
        got, _ = run(K, made, units, conf, mhg)
        same(got, [M.classify(t, u, conf, mhg) for u in units], EXP["external"])
    # saved and reopened: still a protein database, the same answers
    made.save(tmp_path)
    raw = open(tmp_path / "opts.k2d", "rb").read()
    assert struct.unpack_from("<QQQQB", raw) == (15, 12, 0, M.TOGGLE, 0)
    again = K.K2Db.open(tmp_path)
    assert again.opts().protein == 1
    got2, _ = run(K, again, units, 0.5, 1)
    assert np.array_equal(got, got2)
    # a DNA database opened beside the two: its own answers, unchanged
    dexp = json.load(open(os.path.join(GOLD, "k2_pydb_expected.json")))
    dna = K.K2Db.open(os.path.join(GOLD, "k2_pydb"))
    assert dna.opts().protein == 0
    for n_mates in (1, 2):
        us = [u for u in dexp["units"] if u["confidence"] == 0.0 and u["min_hit_groups"] == 2 and len(u["mates"]) == n_mates]
        got, _ = run(K, dna, [u["mates"] for u in us], 0.0, 2)
        same(got, [(u["call"], u["total_kmers"], u["hit_groups"]) for u in us], dexp["external"])
    for d in (made, again, dna):
        d.close()


# ---- what a protein database refuses ------------------------------------------------------------------------------------------------
def refused(K, word, f):
    from scrubby_amd import lib
    with pytest.raises(lib.ScrubbyHipError) as e:
        f()
    assert e.value.status == 1 and word in e.value.message, e.value.message          # SH_ERR_BAD_ARG


def test_refusals(K, db, EXP, tmp_path):
    own = EXP["s_decides"]["mates"][0]
    bases, off, _ = pack([[own]])
    o = db.opts(); o.quick = 1
    refused(K, "--quick", lambda: db.classify(bases, off, opts=o))
    refused(K, "hit lists", lambda: db.classify(bases, off, hits=True))
    md = K.MinimizerData(db)
    refused(K, "minimizer data", lambda: db.classify(bases, off, minimizer_data=md))
    md.close()
    refused(K, "protein", lambda: K.KmerDistrib(db, 100))
    refused(K, "protein", lambda: K.build_kmer_distrib(PROTDB, [os.path.join(BUILD, "library.faa")], 100, taxid=1, output=tmp_path / "d.kmer_distrib"))
    refused(K, "--mask-low-complexity", lambda: K.build_database([os.path.join(BUILD, "library.faa")], tmp_path / "m", taxid=9, protein=True, mask=True))
    refused(K, "protein", lambda: db.insert_sequence(own.encode(), 6))
    # opts->protein against the database's kind, both ways, naming both
    refused(K, "nucleotide options on a protein database", lambda: db.classify(bases, off, opts=K.default_opts()))
    dna = K.K2Db.open(os.path.join(GOLD, "k2_pydb"))
    po = dna.opts(); po.protein = 1
    refused(K, "protein options on a nucleotide database", lambda: dna.classify(bases, off, opts=po))
    dna.close()
    # the runner refuses by name
    (tmp_path / "none.fastq").write_text(f"@r0\n{own}\n+\n{'I' * len(own)}\n")
    for kw, word in ((dict(quick=True), "--quick"), (dict(report_minimizer_data=True), "--report-minimizer-data")):
        refused(K, word, lambda: K.kraken_run([tmp_path / "none.fastq"], [tmp_path / "o.fastq"], PROTDB, taxa=["Viruses"], workdir=tmp_path / "w", **kw))
    # long_unit_bases is ignored: the answers and the route are the same
    o = db.opts(); o.long_unit_bases = 16
    got, st = db.classify(bases, off, opts=o)
    assert st["n_long_units"] == 0 and int(got["call"][0]) == next(u for u in EXP["units"] if u["mates"] == [own])["results"][1]["call"]


# ---- the build from an amino-acid library -------------------------------------------------------------------------------------------
def read_library(EXP):
    """(residues, internal taxon or 0) per record of the fixture library, from its own parsing"""
    ext_to_int = {e: i for i, e in enumerate(EXP["external"]) if i}
    idmap = dict(l.split() for l in open(os.path.join(BUILD, "seqid2taxid.map")).read().splitlines())
    recs, hdr, seq = [], None, []
    for line in open(os.path.join(BUILD, "library.faa")).read().splitlines() + [">"]:
        if line.startswith(">"):
            if hdr is not None:
                sid = hdr.split()[0]
                ext = int(sid.split("|")[1]) if sid.startswith("kraken:taxid|") else int(idmap.get(sid, 0))
                recs.append(("".join(seq), ext_to_int.get(ext, 0)))
            hdr, seq = line[1:], []
        else:
            seq.append(line)
    return recs


def test_build_from_a_protein_library(K, EXP, tmp_path):
    recs = read_library(EXP)
    lib_text = "".join(r for r, _ in recs)
    assert len(recs) == 13 and sum(1 for _, t in recs if t) == 12
    assert all(c in lib_text for c in "UOX*") and any(c.islower() for c in lib_text)
    res = K.build_database([os.path.join(BUILD, "library.faa")], tmp_path / "db", taxonomy_dir=BUILD, seqid2taxid=os.path.join(BUILD, "seqid2taxid.map"),
                           protein=True, capacity=2503)
    assert res["n_records"] == 13 and res["n_skipped"] == 1 and res["n_nodes"] == len(EXP["parents"])
    built = K.K2Db.open(tmp_path / "db")
    o, info = built.opts(), built.info()
    assert (o.protein, o.k, o.l, o.spaced_seed_mask) == (1, 15, 12, 0) and info["capacity"] == 2503
    cells, parent, ext = built.export()
    assert list(parent) == EXP["parents"] and list(ext) == EXP["external"]
    t = M.Table(2503, info["value_bits"], EXP["parents"])
    keys = []
    for p, taxon in recs:
        if taxon:
            keys += t.add_protein(p, taxon)
    assert info["size"] == t.size() == res["size"]
    g = M.Table(2503, info["value_bits"], EXP["parents"])
    g.cells = [int(c) for c in cells]
    assert all(g.get(m) == t.get(m) != 0 for m in keys)                  # the table equals the model's per key
    for n_mates in (1, 2):
        units = [u["mates"] for u in EXP["units"] if len(u["mates"]) == n_mates]
        got, _ = run(K, built, units, 0.0, 2)
        same(got, [M.classify(t, u, 0.0, 2) for u in units], EXP["external"])
    built.close()
    # the estimator follows the options' kind: the distinct minimizers whose hash falls in 4 of 1024 residues
    est = K.estimate_capacity([p.encode() for p, _ in recs], opts=K.default_protein_opts())
    every = set()
    for p, _ in recs:
        every |= {m for m in M.scan_aa(p) if m is not None}
    assert est["n_sampled"] == sum(1 for m in every if (M.fmix64(m) & 1023) < 4)


# ---- reads -c kraken2 end to end ----------------------------------------------------------------------------------------------------
def first_codon(r):
    c = M.CODE_TABLE.index(r)
    return "ACGT"[c >> 4] + "ACGT"[(c >> 2) & 3] + "ACGT"[c & 3]


def revcomp(s):
    return "".join({"A": "T", "C": "G", "G": "C", "T": "A"}.get(c, "N") for c in reversed(s))


@pytest.mark.parametrize("extract", [False, True])
def test_kraken_run_end_to_end(K, db, table, EXP, tmp_path, extract):
    rng = np.random.default_rng(7)
    species = sorted(int(s) for s in EXP["proteins"])
    pairs = []
    for i in range(40):
        if i % 8 == 7:
            m1, m2 = ("".join("ACGT"[x] for x in rng.integers(0, 4, 120)) for _ in range(2))
        else:
            p = EXP["proteins"][str(species[i % len(species)])]
            a, b = int(rng.integers(0, 40)), int(rng.integers(40, 80))
            m1 = "ACG"[: i % 3] + "".join(first_codon(r) for r in p[a:a + 40])
            m2 = revcomp("".join(first_codon(r) for r in p[b:b + 40]))
        pairs.append((m1, m2))
    for f in (0, 1):
        with open(tmp_path / f"r_{f + 1}.fastq", "w") as out:
            for i, p in enumerate(pairs):
                out.write(f"@r{i} {f + 1}\n{p[f]}\n+\n{'I' * len(p[f])}\n")
    w = tmp_path / "w"
    res = K.kraken_run([tmp_path / "r_1.fastq", tmp_path / "r_2.fastq"], [tmp_path / "o_1.fastq", tmp_path / "o_2.fastq"], PROTDB,
                       taxa=["Alphavirus"], workdir=w, extract=extract)
    want = [M.classify(table, list(p), 0.0, 2) for p in pairs]
    ext = EXP["external"]
    lines = [l.split("\t") for l in open(w / "kraken.reads").read().splitlines()]
    assert [l[:4] for l in lines] == [["C" if c else "U", f"r{i}", str(ext[c]), f"{len(pairs[i][0])}|{len(pairs[i][1])}"] for i, (c, _, _) in enumerate(want)]
    assert all(l[4] == "0:0" and len(l) == 5 for l in lines)              # no hit lists over a protein database
    # kraken.report: the report of the model's calls
    model = np.zeros(40, dtype=K.RESULT_DTYPE)
    model["call"] = [c for c, _, _ in want]
    db.write_report(model, tmp_path / "model.report")
    assert open(w / "kraken.report").read() == open(tmp_path / "model.report").read()
    # the reads removed are the model's: every pair called inside the genus
    genus = EXP["names"].index("Alphavirus")
    hit = [i for i, (c, _, _) in enumerate(want) if c and table.is_ancestor(genus, c)]
    assert 5 <= len(hit) <= 30
    kept = [l[1:].split()[0] for l in open(tmp_path / "o_1.fastq").read().splitlines()[0::4]]
    assert kept == [f"r{i}" for i in range(40) if (i in hit) == extract]
    assert res["reads_in"] == 80 and res["reads_out"] == 2 * len(kept)
    shutil.rmtree(w)
