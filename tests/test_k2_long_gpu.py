"""The Kraken arm's wave route (k_k2_classify_wave: one wave classifies one unit, opts.long_unit_bases) against
oracle/k2_oracle.c and against the lane route on the same units: results, counters, hit lists and minimizer data must not
depend on the route.  Every test forces the route with long_unit_bases and reads n_long_units."""
import numpy as np
import pytest

from tests import workloads as W
from tests.test_k2_hitlist_cpu import col5
from tests.test_k2_hitlist_gpu import batch, check, oracle_lists
from tests.test_k2_options_cpu import mask_bases
from tests.test_k2_options_gpu import phred

pytestmark = pytest.mark.gpu

FIELDS = ("call", "total_kmers", "hit_groups")
STATS = ("n_units", "n_classified", "n_probes", "n_kmers", "n_overflow", "n_masked_bases")


@pytest.fixture(scope="module")
def K():
    from scrubby_amd import lib, k2
    lib.require_gpu()
    return k2


@pytest.fixture(scope="module")
def cfg1(oracle):
    return W.cfg1(oracle, 4000)


@pytest.fixture(scope="module")
def tax():
    return W.k2_taxonomy()


@pytest.fixture(scope="module")
def db(K, cfg1, tax):
    """the database of tests/test_k2_hitlist_gpu.py, plus a poly-A stretch and a 7-base tandem repeat under two taxa"""
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
    d.insert_sequence(np.frombuffer(b"A" * 200, dtype=np.uint8), bact[2])
    d.insert_sequence(np.frombuffer(b"ACGGTCA" * 30, dtype=np.uint8), bact[3])
    d.insert_random(0xC0FFEE, 300_000, ids["Bacteria"], len(parents) - 1)
    yield d
    d.close()


@pytest.fixture(scope="module")
def table(oracle, db):
    cells, parent, ext = db.export()
    return oracle.K2Table(cells, parent, db.info()["value_bits"]), ext


def lopts(K, db, long_unit_bases, **kw):
    o = db.opts()
    o.long_unit_bases = long_unit_bases
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def same(g, c, ext):
    for f in FIELDS:
        assert np.array_equal(g[f], c[f]), f"{f}: {int((g[f] != c[f]).sum())} of {len(g)} differ, first at {int(np.flatnonzero(g[f] != c[f])[0])}"
    assert np.array_equal(g["taxid"], ext[c["call"]])


def forced(K, db, oracle, t, ext, recs, o=None, **kw):
    """every record on the wave route, against the oracle"""
    bases, offs = batch(recs)
    g, st = db.classify(bases, offs, opts=lopts(K, db, 1, **kw))
    c = t.classify(o if o is not None else oracle.k2_default_opts(), bases, offs)
    assert st["n_long_units"] == sum(len(r) >= 1 for r in recs)
    same(g, c, ext)
    assert st["n_probes"] == int(c["n_probes"].sum()) and st["n_kmers"] == int(c["total_kmers"].sum())
    return g, st, c


# ---- 1. lengths --------------------------------------------------------------------------------------------------------
def test_length_sweep(K, oracle, db, table, cfg1):
    P, R, ref, seqs, reads, off = cfg1
    t, ext = table
    k, tile = 35, K.K2_WAVE_TILE
    lens = list(range(k - 1, k + 201)) + [tile + k - 1 + d for d in range(-2, 3)] + [5 * tile // 2 + k - 1]
    recs = [bytes(seqs[0][7 * i: 7 * i + n]) for i, n in enumerate(lens)]
    recs += [bytes(seqs[3][900 + 3 * i: 900 + 3 * i + n]) for i, n in enumerate(lens)]      # the 64-taxon mosaic
    g, st, c = forced(K, db, oracle, t, ext, recs)
    assert int((g["call"] != 0).sum()) > len(recs) // 2 and st["n_overflow"] > 0


# ---- 2. runs across lanes ----------------------------------------------------------------------------------------------
def test_runs_across_lanes(K, oracle, db, table):
    t, ext = table
    clean = [b"A" * 5000, (b"ACGGTCA" * 715)[:5000]]
    # the case tests what it claims: one minimizer run over the whole poly-A read, every lane but the first continues it
    assert t.classify_pair(oracle.k2_default_opts(), clean[0])["hit_groups"] == 1
    assert t.classify_pair(oracle.k2_default_opts(), clean[1])["hit_groups"] > 64
    recs = list(clean)
    for r in clean:         # lanes without a valid k-mer, a run that resumes after ambiguity
        s = bytearray(r)
        s[1000:1300] = b"N" * 300
        s[3000:3300] = b"N" * 300
        recs.append(bytes(s))
    recs.append(b"N" * 5000)
    g, st, c = forced(K, db, oracle, t, ext, recs)
    assert int(g["hit_groups"][0]) == 1 and int(g["hit_groups"][2]) == 1 and int(g["total_kmers"][4]) == 5000 - 34
    bases, offs = batch(recs)
    check(K, db, oracle, t, ext, bases, offs, False, go=lopts(K, db, 1))


# ---- 3. the routes agree -----------------------------------------------------------------------------------------------
def mixed_records(cfg1):
    P, R, ref, seqs, reads, off = cfg1
    rng = np.random.default_rng(11)
    recs = []
    for i in range(120):
        recs.append(bytes(reads[i * 150:(i + 1) * 150]))
        if i % 3 == 0:
            n = int(rng.integers(2000, 20001))
            src = seqs[(0, 3, 1, 2)[i // 3 % 4]]
            p = int(rng.integers(900, 3000)) if i // 3 % 4 == 1 else int(rng.integers(0, len(src) - n))
            s = bytearray(src[p: p + n])
            if i % 2:
                for q in rng.integers(0, n, 6):
                    piece = s[int(q): int(q) + int(rng.integers(1, 60))]
                    s[int(q): int(q) + len(piece)] = b"N" * len(piece)
            recs.append(bytes(s))
    recs.insert(10, b"")
    recs.insert(20, bytes(seqs[0][500:534]))
    return recs


def test_routes_agree(K, oracle, db, table, cfg1):
    t, ext = table
    recs = mixed_records(cfg1)
    import torch
    bases, offs = batch(recs)
    n = len(recs)
    hb = np.concatenate([np.frombuffer(b"GATTACA", dtype=np.uint8), bases, np.full(64, ord("N"), np.uint8)])
    d_b = torch.from_numpy(hb).cuda()                     # the base pointer 7 bytes past an aligned address
    d_off = torch.from_numpy(offs.astype(np.int64)).cuda()
    assert d_b[7:].data_ptr() % 8 == 7
    runs = {}
    for lub in (-1, 512):
        md = K.MinimizerData(db)
        d_out = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
        st, (hoff, ent) = db.classify_device_hits(d_b[7:], d_off, n, False, d_out, opts=lopts(K, db, lub), minimizer_data=md)
        out = d_out.cpu().numpy().view(K.RESULT_DTYPE).reshape(-1)
        d_out2 = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
        pst = db.classify_device(d_b[7:], d_off, n, False, d_out2, opts=lopts(K, db, lub))
        assert np.array_equal(out, d_out2.cpu().numpy().view(K.RESULT_DTYPE).reshape(-1)) and {k: st[k] for k in STATS} == {k: pst[k] for k in STATS}
        counts = md.counts()
        hit = np.flatnonzero(counts["n_minimizers"])
        runs[lub] = (out, st, hoff, ent, counts, {int(x): md.registers(int(x)) for x in hit})
        md.close()
    (o0, s0, h0, e0, c0, r0), (o1, s1, h1, e1, c1, r1) = runs[-1], runs[512]
    assert s0["n_long_units"] == 0 and s1["n_long_units"] == sum(len(r) >= 512 for r in recs) > 30
    assert np.array_equal(o0, o1)
    for k in STATS + ("n_hits_redone",):
        assert s0[k] == s1[k], k
    assert s1["n_overflow"] > 0 and s1["n_hits_redone"] > 0
    assert np.array_equal(h0, h1) and np.array_equal(e0, e1)
    assert np.array_equal(c0["n_minimizers"], c1["n_minimizers"]) and int(c0["n_minimizers"].sum()) == int(o0["hit_groups"].sum())
    assert r0.keys() == r1.keys() and all(np.array_equal(r0[x], r1[x]) for x in r0)
    # and both are the oracle's
    c = t.classify(oracle.k2_default_opts(), bases, offs)
    same(o1, c, ext)


# ---- 4. hit lists ------------------------------------------------------------------------------------------------------
def test_hit_lists(K, oracle, db, table, cfg1):
    P, R, ref, seqs, reads, off = cfg1
    t, ext = table
    recs = [bytes(seqs[3][900 + 50 * j: 900 + 50 * j + 3000]) for j in range(12)]       # many entries, more than 8 taxa
    recs += [bytes(seqs[0][5000 * i: 5000 * i + 4500]) for i in range(12)]              # one entry
    bases, offs = batch(recs)
    lane = db.classify(bases, offs, opts=lopts(K, db, -1), hits=True)[1]
    out, st, lists = check(K, db, oracle, t, ext, bases, offs, False, go=lopts(K, db, 1))
    assert st["n_long_units"] == len(recs) and lane["n_overflow"] > 0 and lane["n_hits_redone"] > 0
    assert st["n_overflow"] == lane["n_overflow"] and st["n_hits_redone"] == lane["n_hits_redone"]
    assert max(len(l) for l in lists) > 16 and sum(len(l) == 1 for l in lists) >= 5
    # pairs: a 4-kb mate with a 150-bp mate, and two long mates
    pr = []
    for i in range(10):
        pr += [bytes(seqs[0][9000 * i: 9000 * i + 4000]), bytes(reads[i * 150:(i + 1) * 150])]
        pr += [bytes(seqs[3][900 + 70 * i: 900 + 70 * i + 4200]), bytes(seqs[1][3000 * i: 3000 * i + 5000])]
    pr += [b"", bytes(seqs[0][100:4300]), bytes(seqs[0][100:4300]), bytes(seqs[0][10:40])]
    bases, offs = batch(pr)
    lane = db.classify(bases, offs, paired=True, opts=lopts(K, db, -1), hits=True)[1]
    out, st, lists = check(K, db, oracle, t, ext, bases, offs, True, go=lopts(K, db, 1000))
    assert st["n_long_units"] == len(pr) // 2 and st["n_overflow"] == lane["n_overflow"] > 0 and st["n_hits_redone"] == lane["n_hits_redone"] > 0
    assert all(sum(c == K.HIT_BORDER for c, _ in l) == 1 for l in lists)


# ---- 5. many taxa ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wide(K, oracle):
    """3 000 leaves under one parent, 2 000 pieces of 120 bp each under its own leaf, and the reads tiled from them"""
    n_leaf = 3000
    parents = [0, 0, 1] + [2] * n_leaf
    externals = [0, 1, 2] + [1000 + i for i in range(n_leaf)]
    names = ["", "root", "clade"] + [f"leaf_{i}" for i in range(n_leaf)]
    ranks = ["", "no rank", "genus"] + ["species"] * n_leaf
    d = K.K2Db.create(K.default_opts(), 1_000_003, parents, externals, names, ranks)
    rng = np.random.default_rng(5)
    genome = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 2000 * 120)]
    d.insert_library([genome[120 * i: 120 * (i + 1)] for i in range(2000)], [3 + i for i in range(2000)])
    cells, parent, ext = d.export()
    yield d, oracle.K2Table(cells, parent, d.info()["value_bits"]), ext, genome
    d.close()


@pytest.mark.parametrize("confidence", [0.0, 0.5])
def test_many_taxa(K, oracle, wide, confidence):
    """(Nearly all of a case's seven seconds is the lane route's BIG pass, where one lane resolves the 2 000 taxa of the first
    read; the wave route takes about 20 ms for the three reads.  More than K2_BIG_CAP distinct taxa, where either route drops
    taxa, is not covered.)"""
    d, t, ext, genome = wide
    # 2 000 taxa (past the wave's LDS table: the spill to HBM), 300 (inside it), 9 (just past the lane route's LDS list)
    recs = [bytes(genome), bytes(genome[: 300 * 120]), bytes(genome[120 * 500: 120 * 509])]
    bases, offs = batch(recs)
    o = oracle.k2_default_opts(); o.confidence = confidence
    c = t.classify(o, bases, offs)
    got = {}
    for lub in (-1, 1):
        go = d.opts(); go.long_unit_bases, go.confidence = lub, confidence
        got[lub] = d.classify(bases, offs, opts=go)
        same(got[lub][0], c, ext)
    assert got[1][1]["n_long_units"] == 3 and got[-1][1]["n_long_units"] == 0
    for k in STATS:
        assert got[1][1][k] == got[-1][1][k], k
    assert got[1][1]["n_overflow"] == 3
    assert int(c["call"][0]) != 0


# ---- 6. options --------------------------------------------------------------------------------------------------------
def test_minimum_base_quality(K, oracle, db, table, cfg1):
    P, R, ref, seqs, reads, off = cfg1
    t, ext = table
    recs = [bytes(seqs[0][20_000 * i: 20_000 * i + 3000 + 611 * i]) for i in range(10)] + [bytes(seqs[3][900: 900 + 9000])]
    bases, offs = batch(recs)
    q = phred(len(bases), 82)
    for i, r in enumerate(recs):            # low-quality runs across the borders of the 64 segments of each read
        seg = min(-(-(len(r) - 34) // 64) | 1, 63)
        for j in range(1, 64, 5):
            p = int(offs[i]) + j * seg + 34 - 3
            q[p: p + 9] = 33 + 5
    q[int(offs[3]): int(offs[3]) + 40] = 33 + 2
    go = lopts(K, db, 1, min_base_quality=20)
    g, st = db.classify(bases, offs, opts=go, quals=q)
    lane, lst = db.classify(bases, offs, opts=lopts(K, db, -1, min_base_quality=20), quals=q)
    c = t.classify(oracle.k2_default_opts(), mask_bases(bases, q, 20), offs)
    same(g, c, ext)
    assert st["n_long_units"] == len(recs) and st["n_masked_bases"] == lst["n_masked_bases"] > 0
    assert np.array_equal(g, lane) and st["n_probes"] == lst["n_probes"] == int(c["n_probes"].sum())
    check(K, db, oracle, t, ext, bases, offs, False, go=go, quals=q)


def test_down_sampled_database(K, oracle, cfg1, tax):
    P, R, ref, seqs, reads, off = cfg1
    parents, externals, names, ranks, ids = tax
    go = K.default_opts(); go.min_acceptable_hash = 3 << 62
    d = K.K2Db.create(go, 1_000_003, parents, externals, names, ranks)
    d.insert_sequence(seqs[0], ids["Homo sapiens"])
    cells, parent, ext = d.export()
    t = oracle.K2Table(cells, parent, 17)
    o = oracle.k2_default_opts(); o.min_acceptable_hash = 3 << 62
    recs = [bytes(seqs[0][30_000 * i: 30_000 * i + 2500 + 997 * i]) for i in range(12)]
    g, st, c = forced(K, d, oracle, t, ext, recs, o=o, min_acceptable_hash=3 << 62)
    assert int((g["call"] != 0).sum()) >= 10
    bases, offs = batch(recs)
    go.long_unit_bases = 1
    check(K, d, oracle, t, ext, bases, offs, False, o=o, go=go)
    d.close()


@pytest.mark.parametrize("k, l", [(25, 17), (31, 31)])          # the W = 16 and W = 1 instances
def test_other_k_l(K, oracle, cfg1, tax, k, l):
    P, R, ref, seqs, reads, off = cfg1
    parents, externals, names, ranks, ids = tax
    go = K.default_opts(); go.k, go.l, go.spaced_seed_mask = k, l, 0
    d = K.K2Db.create(go, 2_000_003, parents, externals, names, ranks)
    d.insert_sequence(seqs[0][:300_000], ids["Homo sapiens"])
    d.insert_sequence(seqs[1][:300_000], ids["Pan troglodytes"])
    d.insert_random(7, 100_000, ids["Bacteria"], len(parents) - 1)
    cells, parent, ext = d.export()
    t = oracle.K2Table(cells, parent, 17)
    o = oracle.k2_default_opts(); o.k, o.l, o.spaced_seed_mask = k, l, 0
    tile = K.K2_WAVE_TILE
    recs = [bytes(seqs[i % 2][20_000 * i: 20_000 * i + n]) for i, n in enumerate([k - 1, k, k + 63, k + 64, 3000, tile + k - 2, tile + k - 1, tile + k, 9001])]
    s = bytearray(recs[4]); s[700:760] = b"N" * 60; s[2999:] = b"N"; recs.append(bytes(s))
    g, st, c = forced(K, d, oracle, t, ext, recs, o=o)
    assert int((g["call"] != 0).sum()) >= 6
    bases, offs = batch(recs)
    go.long_unit_bases = 1
    check(K, d, oracle, t, ext, bases, offs, False, o=o, go=go)
    d.close()


def test_quick_stays_on_the_lane_route(K, db, cfg1):
    P, R, ref, seqs, reads, off = cfg1
    recs = [bytes(seqs[0][10_000 * i: 10_000 * i + 5000]) for i in range(20)] + [bytes(seqs[3][900:7000])]
    bases, offs = batch(recs)
    a, sa = db.classify(bases, offs, opts=lopts(K, db, 1, quick=1))
    b, sb = db.classify(bases, offs, opts=lopts(K, db, -1, quick=1))
    assert sa["n_long_units"] == 0 and np.array_equal(a, b) and {k: sa[k] for k in STATS} == {k: sb[k] for k in STATS}
    assert int((a["call"] != 0).sum()) >= 20


# ---- 7. defaults -------------------------------------------------------------------------------------------------------
def test_default_short_reads_take_no_wave(K, oracle, db, table, cfg1):
    P, R, ref, seqs, reads, off = cfg1
    t, ext = table
    assert K.default_opts().long_unit_bases == 0 and db.opts().long_unit_bases == 0
    g, st = db.classify(reads[: 2000 * 150], off[:2001])
    assert st["n_long_units"] == 0 and st["ms_long"] == 0.0
    same(g, t.classify(oracle.k2_default_opts(), reads[: 2000 * 150], off[:2001]), ext)


def test_kraken_run_long_reads(K, oracle, db, table, cfg1, tmp_path):
    P, R, ref, seqs, reads, off = cfg1
    t, ext = table
    dbdir = tmp_path / "db"; dbdir.mkdir()
    db.save(dbdir)
    rng = np.random.default_rng(2)
    recs = []
    for i in range(40):         # every read longer than any default threshold the measurements could choose (32 768)
        src = seqs[i % 4]
        n = int(rng.integers(33_000, 60_000))
        p = int(rng.integers(0, len(src) - n))
        s = bytearray(src[p: p + n])
        if i % 4 == 0:
            s[5000:5040] = b"N" * 40
        recs.append(bytes(s))
    with open(tmp_path / "long.fastq", "w") as f:
        for i, s in enumerate(recs):
            f.write(f"@r{i}\n{s.decode()}\n+\n{'I' * len(s)}\n")
    bases, offs = batch(recs)
    res, lists = oracle_lists(oracle, t, oracle.k2_default_opts(), bases, offs, False)
    K.kraken_run([tmp_path / "long.fastq"], [tmp_path / "out.fastq"], dbdir, taxa=["Chordata"], workdir=tmp_path / "w")
    lines = [l.split("\t") for l in open(tmp_path / "w" / "kraken.reads").read().splitlines()]
    assert len(lines) == 40 and all(len(l) == 5 for l in lines)
    assert [int(l[2]) for l in lines] == [int(ext[r["call"]]) for r in res] and sum(r["call"] != 0 for r in res) >= 30
    assert [l[4] for l in lines] == [col5(l, ext) for l in lists]
