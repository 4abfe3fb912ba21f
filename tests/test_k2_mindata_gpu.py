"""kraken2 --report-minimizer-data on the GPU (k_k2_classify's MIND instances, sh_k2_mindata_*, sh_k2_classify_ex_*,
kraken.minimizer.report) against the model of tests/k2_mindata_ref.py, which is accepted per input only where its events and
lookups equal the oracle's hit_groups and n_probes.  The table is built on the GPU and exported, so both sides probe the same
cells.  Counting a unit twice (in the BIG pass, in the hit lists' redo pass) is what the shapes below are chosen to catch."""
import math
import os
import subprocess

import numpy as np
import pytest

from tests import k2_mindata_ref as R
from tests import workloads as W
from tests.test_k2_hitlist_gpu import STATS, batch
from tests.test_k2_options_cpu import mask_bases

pytestmark = pytest.mark.gpu


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
    """the database of tests/test_k2_hitlist_gpu.py (three species over contigs 0-2, a 64-taxon mosaic of contig 3, random filler)"""
    P, Rp, ref, seqs, reads, off = cfg1
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


@pytest.fixture(scope="module")
def md(K, db):
    m = K.MinimizerData(db)
    yield m
    m.close()


def same_estimate(got, regs):
    want = R.estimate(regs)
    assert abs(got - want) <= 1e-12 * max(want, 1.0) and R.rounded(got) == R.rounded(want), (got, want)


def check_md(m, exp):
    """every taxon: n_minimizers, all registers, the clade values and the four estimates equal the model's"""
    c = m.counts()
    assert np.array_equal(c["n_minimizers"], exp.count)
    assert np.array_equal(c["clade_minimizers"], exp.clade_count())
    cr = exp.clade_regs()
    for t in range(exp.n):
        own, clade = m.registers(t), m.registers(t, clade=True)
        assert np.array_equal(own, exp.regs(t)), t
        assert np.array_equal(clade, cr[t]), t
        same_estimate(c["distinct"][t], own)
        same_estimate(c["clade_distinct"][t], clade)
    return c


def run(K, db, m, bases, offs, paired, opts=None, quals=None, hits=False):
    """one call into the accumulator; results and the six statistics equal the plain entry's"""
    got = db.classify(bases, offs, paired=paired, opts=opts, quals=quals, hits=hits, minimizer_data=m)
    plain = db.classify(bases, offs, paired=paired, opts=opts, quals=quals, hits=hits)
    assert np.array_equal(got[0], plain[0])
    assert {k: got[1][k] for k in STATS} == {k: plain[1][k] for k in STATS}
    if hits:
        assert got[1]["n_hits_redone"] == plain[1]["n_hits_redone"]
        assert np.array_equal(got[2][0], plain[2][0]) and np.array_equal(got[2][1], plain[2][1])
    return got


def with_n_runs(s, rng, n):
    s = bytearray(s)
    for _ in range(n):
        p, w = int(rng.integers(0, max(len(s), 1))), int(rng.integers(1, 12))
        s[p: p + w] = b"N" * len(s[p: p + w])
    return bytes(s)


@pytest.fixture(scope="module")
def singles(cfg1):
    """200 single reads (not a multiple of 64): lengths 20 (shorter than k), 35, 36, 150 and 300, N runs in every fifth, and 20
    random reads without hits"""
    P, Rp, ref, seqs, reads, off = cfg1
    rng = np.random.default_rng(31)
    recs = []
    for i in range(180):
        ln = (20, 35, 36, 150, 300)[i % 5]
        src = seqs[(i // 5) % 4]
        o = int(rng.integers(0, len(src) - ln))
        s = bytes(src[o: o + ln])
        recs.append(with_n_runs(s, rng, 2) if i % 7 == 3 else s)
    recs += [bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 150)]) for _ in range(20)]
    return batch(recs)


@pytest.fixture(scope="module")
def singles_events(oracle, table, singles):
    """the model's events of `singles`, computed once and left unchanged"""
    t, ext = table
    return R.Model(oracle, t, oracle.k2_default_opts()).events(singles[0], singles[1], False)


def test_mixed_singles(K, db, table, md, singles, singles_events):
    t, ext = table
    md.reset()
    out, st = run(K, db, md, singles[0], singles[1], False)
    assert [len(e) for e in singles_events] == [int(x) for x in out["hit_groups"]]
    assert sum(len(e) for e in singles_events[-20:]) == 0 and sum(len(e) for e in singles_events) > 1000
    c = check_md(md, R.Expected(t.parent).add(singles_events))
    assert int((c["n_minimizers"] > 0).sum()) >= 4


def test_pairs(K, oracle, db, table, md, cfg1):
    P, Rp, ref, seqs, reads, off = cfg1
    t, ext = table
    recs = [bytes(reads[i * 150:(i + 1) * 150]) for i in range(260)]
    recs[10] = recs[10][:20]                                             # mate 1 of pair 5 has no k-mers
    recs[14], recs[15] = bytes(seqs[0][50_000: 50_150]), bytes(seqs[0][50_115: 50_265])       # mate 2 begins with mate 1's last k-mer
    bases, offs = batch(recs)
    model = R.Model(oracle, t, oracle.k2_default_opts())
    ev = model.events(bases, offs, True)
    e1, e2 = model.unit([recs[14]])[0], model.unit([recs[15]])[0]
    assert e1[-1] == e2[0] and ev[7] == e1 + e2                          # the shared minimizer is looked up, and counted, in both mates
    md.reset()
    out, st = run(K, db, md, bases, offs, True)
    assert len(out) == 130 and [len(e) for e in ev] == [int(x) for x in out["hit_groups"]]
    check_md(md, R.Expected(t.parent).add(ev))


def test_accumulation(K, db, table, md, singles, singles_events):
    t, ext = table
    bases, offs = singles
    md.reset()
    run(K, db, md, bases, offs, False)
    once = [md.registers(x) for x in range(len(t.parent))]
    run(K, db, md, bases, offs, False)
    check_md(md, R.Expected(t.parent).add(singles_events, times=2))     # counters double ...
    assert all(np.array_equal(a, md.registers(x)) for x, a in enumerate(once))        # ... registers do not move
    # calls of 1, 63 and the rest equal one call
    md.reset()
    for lo, hi in ((0, 1), (1, 64), (64, len(offs) - 1)):
        run(K, db, md, bases, offs[lo: hi + 1], False)
    check_md(md, R.Expected(t.parent).add(singles_events))
    md.reset()
    c = md.counts()
    assert not c["n_minimizers"].any() and not c["clade_minimizers"].any() and not c["distinct"].any() and not c["clade_distinct"].any()
    assert not md.registers(3).any() and not md.registers(1, clade=True).any()


@pytest.fixture(scope="module")
def mosaic(cfg1):
    """reads over the 64-taxon mosaic of contig 3: more than 8 taxa per unit (the BIG pass) and, with an N every 40-55 bases,
    more than 16 hit-list entries (the hit lists' redo pass); a few ordinary reads beside them"""
    P, Rp, ref, seqs, reads, off = cfg1
    recs = [bytes(seqs[3][900 + 150 * j: 900 + 150 * j + 2000]) for j in range(12)]
    for i in range(12):
        s = bytearray(seqs[0][5000 * i: 5000 * i + 1000])
        for p in range(3 + i % 7, len(s), 40 + i % 16):
            s[p] = ord("N")
        recs.append(bytes(s))
    recs += [bytes(reads[i * 150:(i + 1) * 150]) for i in range(200, 240)]
    return batch(recs)


@pytest.fixture(scope="module")
def mosaic_events(oracle, table, mosaic):
    t, ext = table
    return R.Model(oracle, t, oracle.k2_default_opts()).events(mosaic[0], mosaic[1], False)


def test_big_pass_does_not_count_twice(K, db, table, md, mosaic, mosaic_events):
    t, ext = table
    md.reset()
    out, st = run(K, db, md, mosaic[0], mosaic[1], False)
    assert st["n_overflow"] > 0                                          # the BIG pass ran
    c = check_md(md, R.Expected(t.parent).add(mosaic_events))
    assert int(c["n_minimizers"].sum()) == int(out["hit_groups"].sum())


def test_hits_redo_pass_does_not_count_twice(K, db, table, md, mosaic, mosaic_events):
    t, ext = table
    md.reset()
    out, st, lists = run(K, db, md, mosaic[0], mosaic[1], False, hits=True)
    assert st["n_hits_redone"] > 0 and st["n_overflow"] > 0              # the redo pass ran (and the BIG pass beside it)
    c = check_md(md, R.Expected(t.parent).add(mosaic_events))
    assert int(c["n_minimizers"].sum()) == int(out["hit_groups"].sum())


@pytest.mark.parametrize("mhg", [1, 2])
def test_quick(K, oracle, db, table, md, cfg1, mhg):
    P, Rp, ref, seqs, reads, off = cfg1
    t, ext = table
    n = 200
    bases, offs = reads[: n * 150], off[: n + 1]
    go = db.opts(); go.quick = 1; go.min_hit_groups = mhg
    o = oracle.k2_default_opts()
    for paired in (False, True):
        ev = R.Model(oracle, t, o).events(bases, offs, paired, quick=True, min_hit_groups=mhg)
        md.reset()
        out, st = run(K, db, md, bases, offs, paired, opts=go)
        assert [len(e) for e in ev] == [int(x) for x in out["hit_groups"]] and max(len(e) for e in ev) == mhg
        check_md(md, R.Expected(t.parent).add(ev))


def test_minimum_base_quality(K, oracle, db, table, md, cfg1):
    P, Rp, ref, seqs, reads, off = cfg1
    t, ext = table
    n = 200
    bases, offs = reads[: n * 150], off[: n + 1]
    q = np.full(n * 150, ord("I"), np.uint8)
    for i in range(0, n, 2):                                             # a masked run in every second read
        q[i * 150 + 60: i * 150 + 72] = ord("#")
    go = db.opts(); go.min_base_quality = 20
    masked = mask_bases(bases, q, 20)
    plain_ev = R.Model(oracle, t, oracle.k2_default_opts()).events(bases, offs, True)
    ev = R.Model(oracle, t, oracle.k2_default_opts()).events(masked, offs, True)
    assert sum(len(e) for e in ev) < sum(len(e) for e in plain_ev)       # minimizers under masked bases are not counted
    md.reset()
    out, st = run(K, db, md, bases, offs, True, opts=go, quals=q)
    assert st["n_masked_bases"] == 12 * (n // 2)
    check_md(md, R.Expected(t.parent).add(ev))


def test_rejected_calls_count_nothing_and_leave_the_handles_usable(K, oracle, db, table, md, cfg1):
    """The checks the host and the device entry share, through each: --quick with hit lists, the minimizer data of another
    database (another node count), paired with an odd record count.  Each is SH_ERR_BAD_ARG and counts nothing; the same
    database and accumulator then classify the batch as the oracle does."""
    import torch
    from scrubby_amd.lib import ScrubbyHipError
    from tests.test_k2_options_gpu import same
    P, Rp, ref, seqs, reads, off = cfg1
    t, ext = table
    n = 10
    bases, offs = reads[: n * 150], off[: n + 1]
    d_b = torch.from_numpy(np.concatenate([bases, np.full(64, ord("N"), np.uint8)])).cuda()
    d_off = torch.from_numpy(offs.astype(np.int64)).cuda()
    d_out = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
    quick = db.opts(); quick.quick = 1
    small = K.K2Db.create(K.default_opts(), 1009, [0, 0, 1], [0, 1, 2], ["", "root", "other"], ["", "no rank", "species"])
    other = K.MinimizerData(small)
    want = t.classify(oracle.k2_default_opts(), bases, offs, paired=False)
    exp = R.Expected(t.parent).add(R.Model(oracle, t, oracle.k2_default_opts()).events(bases, offs, False))
    rejected = {
        "quick with hits": (lambda: db.classify(bases, offs, opts=quick, hits=True, minimizer_data=md),
                            lambda: db.classify_device_hits(d_b, d_off, n, False, d_out, opts=quick, minimizer_data=md)),
        "minimizer data of another database": (lambda: db.classify(bases, offs, minimizer_data=other),
                                               lambda: db.classify_device(d_b, d_off, n, False, d_out, minimizer_data=other)),
        "paired, odd record count": (lambda: db.classify(bases[: 9 * 150], offs[:10], paired=True, minimizer_data=md),
                                     lambda: db.classify_device(d_b, d_off, 9, True, d_out, minimizer_data=md)),
    }
    try:
        md.reset()
        for name, calls in rejected.items():
            for call in calls:
                with pytest.raises(ScrubbyHipError) as ei:
                    call()
                assert ei.value.status == 1, name                      # SH_ERR_BAD_ARG
                assert not md.counts()["n_minimizers"].any() and not other.counts()["n_minimizers"].any(), name
            got, st, lists = db.classify(bases, offs, hits=True, minimizer_data=md)
            same(got, want, ext)
            assert len(lists[0]) == n + 1 and int(lists[0][-1]) == len(lists[1]) > 0
            check_md(md, exp)
            md.reset()
    finally:
        other.close(); small.close()


def test_down_sampled_database(K, oracle, cfg1, tax):
    P, Rp, ref, seqs, reads, off = cfg1
    parents, externals, names, ranks, ids = tax
    d = K.K2Db.create(K.default_opts(), 1_000_003, parents, externals, names, ranks)
    d.set_min_acceptable_hash(1 << 63)                                   # about half the hash range
    d.insert_sequence(seqs[0], ids["Homo sapiens"])
    m = K.MinimizerData(d)
    try:
        cells, parent, ext = d.export()
        t = oracle.K2Table(cells, parent, 17)
        o = oracle.k2_default_opts(); o.min_acceptable_hash = 1 << 63
        n = 200
        ev = R.Model(oracle, t, o).events(reads[: n * 150], off[: n + 1], True)
        assert 0 < sum(len(e) for e in ev) and all(R.fmix64(mm) >= 1 << 63 for e in ev for _, mm in e)
        run(K, d, m, reads[: n * 150], off[: n + 1], True)
        check_md(m, R.Expected(parent).add(ev))
    finally:
        m.close(); d.close()


def test_single_taxon_database(K, oracle, cfg1):
    """a host-depletion database: every update of the batch lands on one taxon's counter and registers"""
    P, Rp, ref, seqs, reads, off = cfg1
    tx = K.taxonomy_single(9606, "Homo sapiens", "species")
    go = K.default_opts()
    d = K.K2Db.create_from_taxonomy(go, 1_000_003, tx)
    taxon = tx.internal(9606)
    d.insert_sequence(seqs[0], taxon)
    m = K.MinimizerData(d)
    try:
        cells, parent, ext = d.export()
        vb = d.info()["value_bits"]
        t = oracle.K2Table(cells, parent, vb)
        o = oracle.k2_default_opts(); o.value_bits = vb
        rng = np.random.default_rng(41)
        recs = [bytes(seqs[0][s: s + 150]) for s in rng.integers(0, len(seqs[0]) - 150, 300)]
        bases, offs = batch(recs)
        ev = R.Model(oracle, t, o).events(bases, offs, False)
        out, st = run(K, d, m, bases, offs, False, opts=d.opts())
        c = check_md(m, R.Expected(parent).add(ev))
        assert int(c["n_minimizers"][taxon]) == int(out["hit_groups"].sum()) == int(c["n_minimizers"].sum()) > 300 * 20
        assert int(c["clade_minimizers"][1]) == int(c["n_minimizers"][taxon])
    finally:
        m.close(); d.close(); tx.close()


def test_one_long_read(K, oracle, db, table, md, cfg1):
    """20 kb in one lane: many drains, the lane's pending count carried through all of them"""
    P, Rp, ref, seqs, reads, off = cfg1
    t, ext = table
    bases, offs = batch([bytes(seqs[1][30_000: 50_000])])
    ev = R.Model(oracle, t, oracle.k2_default_opts()).events(bases, offs, False)
    assert len(ev[0]) > 1000
    md.reset()
    run(K, db, md, bases, offs, False)
    check_md(md, R.Expected(t.parent).add(ev))


def test_clade_merge(K, oracle, db, table, md, cfg1, tax):
    """Homo sapiens and Homo heidelbergensis share 200 kb.  The table keeps a shared minimizer at the LCA, so those live at the
    genus itself and the rest of contig 0 at Homo sapiens; the genus clade holds the union of its subtree."""
    P, Rp, ref, seqs, reads, off = cfg1
    parents, externals, names, ranks, ids = tax
    t, ext = table
    rng = np.random.default_rng(51)
    starts = list(rng.integers(0, 199_000, 150)) + list(rng.integers(201_000, len(seqs[0]) - 300, 150))
    bases, offs = batch([bytes(seqs[0][int(s): int(s) + 300]) for s in starts])
    ev = R.Model(oracle, t, oracle.k2_default_opts()).events(bases, offs, False)
    exp = R.Expected(t.parent).add(ev)
    md.reset()
    run(K, db, md, bases, offs, False)
    c = check_md(md, exp)
    g, hs, hh = ids["Homo"], ids["Homo sapiens"], ids["Homo heidelbergensis"]
    assert len(exp.sets[g]) > 1000 and len(exp.sets[hs]) > 1000
    union = exp.sets[g] | exp.sets[hs] | exp.sets[hh]
    assert exp.clade_sets()[g] == union
    assert np.array_equal(md.registers(g, clade=True), R.registers(union))
    # the clade's estimate is an estimate of the union: within five standard errors (1.04 / sqrt(4096) each) of its size
    assert abs(c["clade_distinct"][g] - len(union)) <= 5 * 1.04 / math.sqrt(R.M) * len(union)
    # reads that repeat minimizers do not add to it: the same batch again moves the count, not the estimate
    run(K, db, md, bases, offs, False)
    c2 = md.counts()
    assert c2["clade_distinct"][g] == c["clade_distinct"][g] and int(c2["clade_minimizers"][g]) == 2 * int(c["clade_minimizers"][g])
    assert c["clade_distinct"][g] < int(c2["clade_minimizers"][g])


# ---- end to end: kraken.minimizer.report ------------------------------------------------------------------------------------
def _fastq(path, ids, seqs):
    with open(path, "w") as f:
        for i, s in zip(ids, seqs):
            f.write(f"@{i}\n{s.decode()}\n+\n{'I' * len(s)}\n")


def test_kraken_run(K, oracle, db, table, cfg1, tax, tmp_path, monkeypatch):
    P, Rp, ref, seqs, reads, off = cfg1
    parents, externals, names, ranks, ids = tax
    t, ext = table
    dbdir = tmp_path / "db"; dbdir.mkdir()
    db.save(dbdir)
    n = 2000
    r1 = [bytes(reads[(2 * i) * 150:(2 * i + 1) * 150]) for i in range(n)]
    r2 = [bytes(reads[(2 * i + 1) * 150:(2 * i + 2) * 150]) for i in range(n)]
    names_ = [f"p{i}" for i in range(n)]
    _fastq(tmp_path / "a_1.fastq", names_, r1)
    _fastq(tmp_path / "a_2.fastq", names_, r2)
    ins = [tmp_path / "a_1.fastq", tmp_path / "a_2.fastq"]
    text = {}
    for env in ("0", "1"):                 # the streaming form and the collect-then-classify form
        monkeypatch.setenv("SCRUBBY_HIP_LEGACY_HOST", env)
        for opt in (False, True):
            w = tmp_path / f"w{env}{int(opt)}"
            outs = [tmp_path / f"o{env}{int(opt)}_1.fastq", tmp_path / f"o{env}{int(opt)}_2.fastq"]
            r = K.kraken_run(ins, outs, dbdir, taxa=["Chordata"], taxa_direct=["9606"], workdir=w, json=w / "report.json", report_minimizer_data=opt)
            text[env, opt] = [open(w / "kraken.report").read(), open(w / "kraken.reads").read(), open(outs[0]).read(), open(outs[1]).read(), r["reads_removed"]]
            assert os.path.exists(w / "kraken.minimizer.report") == opt
        assert text[env, False] == text[env, True], env
        assert text[env, True][4] > 0, env
    a, b = (open(tmp_path / f"w{e}1" / "kraken.minimizer.report").read() for e in ("0", "1"))
    assert a == b
    # the model's report: the calls come from the plain entry, the minimizer columns from the model's events
    bases, offs = batch([x for p in zip(r1, r2) for x in p])
    res, _ = db.classify(bases, offs, paired=True)
    ev = R.Model(oracle, t, oracle.k2_default_opts()).events(bases, offs, True)
    exp = R.Expected(t.parent).add(ev)
    direct = np.bincount(res["call"][res["call"] != 0], minlength=len(parents))
    nodes, _, _ = K.make_taxonomy(parents, externals, names, ranks)
    cd = [R.rounded(R.estimate(x)) for x in exp.clade_regs()]
    want = R.report_text(parents, [nd.first_child for nd in nodes], [nd.child_count for nd in nodes], names, ranks, externals, direct, exp.clade_count(), cd, n)
    assert a == want
    assert all(len(l.split("\t")) == 8 for l in a.splitlines()) and all(len(l.split("\t")) == 6 for l in text["0", True][0].splitlines())
    # the CLI: the token sets the option and is no longer named as ignored
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scrubby_amd", "scrubby-hip")
    p = subprocess.run([exe, "reads", "-i", str(ins[0]), str(ins[1]), "-o", str(tmp_path / "c_1.fastq"), str(tmp_path / "c_2.fastq"), "-c", "kraken2",
                        "-I", str(dbdir), "-T", "Chordata", "-w", str(tmp_path / "wc"), "-C", "--report-minimizer-data --confidence 0.1"],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    assert "ignored" not in p.stderr and "report-minimizer-data" not in p.stderr
    cli = open(tmp_path / "wc" / "kraken.minimizer.report").read()
    assert cli and all(len(l.split("\t")) == 8 for l in cli.splitlines())
    assert all(len(l.split("\t")) == 6 for l in open(tmp_path / "wc" / "kraken.report").read().splitlines())
    # --confidence changes calls, never what was looked up: columns 4 and 5 of the root row are those of the library run
    root = lambda s: next(l.split("\t") for l in s.splitlines() if l.split("\t")[5] == "R")
    assert root(cli)[3:5] == root(a)[3:5]
