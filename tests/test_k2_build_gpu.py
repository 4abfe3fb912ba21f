"""Database build on the GPU: sh_k2_insert_library_device, sh_k2_estimate_capacity_device, sh_k2_build_run, `scrubby-hip k2-build`.

Ground truth comes from the frozen oracle only (k2o_scan, k2o_hash, k2o_cht_set with `parent`, k2o_cht_get, k2o_lca): for EVERY
distinct minimizer of a library, k2o_cht_get on the exported GPU table must give the LCA of the taxa of all records that hold it,
with no tolerance and no key left out.  That is exact only if no two distinct minimizers with the same truncated key lie in one
occupied run of the table (insertion order, which is free on a GPU, could then merge them).  The occupied runs of a linear-probing
table do not depend on the insertion order, so `assert_no_alias` computes them on the CPU from the keys' home cells and ASSERTS that
the library has no such pair: a condition on the fixtures (seed 20261016 of tests/golden/make_k2_build.py, seeds SYN_SEED below),
not an exclusion.  PARITY UNPINNED against Kraken 2 itself (oracle/k2_oracle.h)."""
import gzip
import json
import os
import struct
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "k2_build")
EXE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scrubby_amd", "scrubby-hip")
FIX_CAPACITY = 16_529          # explicit capacity of the fixture's table (11 570 distinct minimizers: load 0.7)
SYN_SEED = 0x5C2B0B01
SYN_CAPACITY = 907_003          # 634 882 distinct minimizers: load 0.7


@pytest.fixture(scope="module")
def K():
    from scrubby_amd import lib, k2
    lib.require_gpu()
    return k2


@pytest.fixture(scope="module")
def E():
    with open(os.path.join(GOLD, "expected.json")) as f:
        return json.load(f)


def read_fasta(path):
    """[(header, sequence bytes)] of a FASTA file, plain Python"""
    out, h, parts = [], None, []
    op = gzip.open if str(path).endswith(".gz") else open
    with op(path, "rb") as f:
        for ln in f:
            ln = ln.rstrip(b"\r\n")
            if ln.startswith(b">"):
                if h is not None:
                    out.append((h, b"".join(parts)))
                h, parts = ln[1:].decode("latin-1"), []
            elif h is not None:
                parts.append(ln)
    if h is not None:
        out.append((h, b"".join(parts)))
    return out


def write_fasta(path, records, width=80):
    op = gzip.open if str(path).endswith(".gz") else open
    with op(path, "wb") as f:
        for h, s in records:
            s = bytes(s)
            f.write(b">" + h.encode("latin-1") + b"\n")
            for p in range(0, len(s), width):
                f.write(s[p: p + width] + b"\n")


@pytest.fixture(scope="module")
def fixture_lib(E):
    recs = read_fasta(os.path.join(GOLD, "library.fna"))
    assert [h for h, _ in recs] == [r["header"] for r in E["records"]] and [len(s) for _, s in recs] == [r["length"] for r in E["records"]]
    return [s for _, s in recs], [r["internal"] for r in E["records"]]


@pytest.fixture(scope="module")
def fixture_parent(E):
    return np.array([n["parent"] for n in E["nodes"]], dtype=np.uint32)


def o_opts(oracle, value_bits):
    o = oracle.k2_default_opts()
    o.value_bits = value_bits
    return o


def expected_map(oracle, o, records, taxa, parent):
    """(keys, values): every distinct minimizer k2o_scan finds in the records that have a taxon, and the k2o_lca of the taxa of all
    records holding it"""
    ks, ts = [], []
    for seq, t in zip(records, taxa):
        if t == 0:
            continue
        mins, amb = oracle.k2_scan(seq, o)
        u = np.unique(mins[amb == 0])
        ks.append(u); ts.append(np.full(len(u), t, dtype=np.uint32))
    if not ks:
        return np.zeros(0, np.uint64), np.zeros(0, np.uint32)
    k, t = np.concatenate(ks), np.concatenate(ts)
    order = np.lexsort((t, k))
    k, t = k[order], t[order]
    first = np.concatenate([[True], k[1:] != k[:-1]])
    keys, start = k[first], np.flatnonzero(first)
    vals = t[start].copy()
    end = np.concatenate([start[1:], [len(k)]])
    for i in np.flatnonzero(t[end - 1] != t[start]):         # keys under more than one taxon
        v = 0
        for x in np.unique(t[start[i]: end[i]]):
            v = oracle.k2_lca(parent, v, int(x))
        vals[i] = v
    return keys, vals


def hashes(oracle, keys):
    return np.array([oracle.lib().k2o_hash(int(x)) for x in keys], dtype=np.uint64)


def assert_no_alias(h, capacity, value_bits):
    """h: fmix64 of the distinct keys.  If every key takes a cell of its own, the cells they occupy are fixed by their home cells
    alone; no two keys of one occupied run may share the truncated key (then no insertion order merges any two of them, and
    every key does take a cell of its own).  Returns the load."""
    n = len(h)
    assert n < capacity
    home = (h % np.uint64(capacity)).astype(np.int64)
    srt = np.sort(home)
    # first-come placement over two laps of the table: the second lap starts with whatever the first pushed round the end
    two = np.concatenate([srt, srt + capacity])
    idx = np.arange(2 * n, dtype=np.int64)
    occ = np.sort((np.maximum.accumulate(two - idx) + idx)[n:] % capacity)
    assert len(np.unique(occ)) == n
    run = np.concatenate([[0], np.cumsum(occ[1:] != occ[:-1] + 1)])
    if occ[0] == 0 and occ[-1] == capacity - 1:
        run[run == run[-1]] = 0          # one run round the end of the table
    at = np.searchsorted(occ, home)
    assert np.array_equal(occ[at], home)          # a key's home cell is always occupied: the key lies in that cell's run
    comp = h >> np.uint64(32 + value_bits)
    pairs = np.stack([run[at].astype(np.uint64), comp], axis=1)
    assert len(np.unique(pairs, axis=0)) == n, "two distinct minimizers of one occupied run share a truncated key: choose another seed"
    return len(h) / capacity


def check_every_key(oracle, cells, value_bits, keys, vals):
    t = oracle.K2Table(cells, np.zeros(1, np.uint32), value_bits)
    got = np.array([t.get(int(k)) for k in keys], dtype=np.uint32)
    bad = np.flatnonzero(got != vals)
    assert len(bad) == 0, (len(bad), [(hex(int(keys[i])), int(got[i]), int(vals[i])) for i in bad[:5]])


def sequential_table(oracle, o, records, taxa, parent, capacity, value_bits, min_hash=0):
    """the same library inserted one minimizer at a time with k2o_cht_set (LCA on an existing key)"""
    t = oracle.K2Table.empty(capacity, parent, value_bits)
    for seq, tx in zip(records, taxa):
        if tx == 0:
            continue
        mins, amb = oracle.k2_scan(seq, o)
        for m in np.unique(mins[amb == 0]):
            if min_hash and oracle.lib().k2o_hash(int(m)) < min_hash:
                continue
            assert t.set(int(m), tx)
    return t


def write_map(path, ids_taxa):
    with open(path, "w") as f:
        for s, t in ids_taxa:
            f.write(f"{s}\t{t}\n")


def build_fixture(K, out, **kw):
    return K.build_database([os.path.join(GOLD, "library.fna")], out, taxonomy_dir=GOLD, seqid2taxid=os.path.join(GOLD, "seqid2taxid.map"), **kw)


def open_export(K, path):
    d = K.K2Db.open(path)
    try:
        return d.export(), d.info()
    finally:
        d.close()


# ---- every key of the fixture ------------------------------------------------------------------------------------------------
def test_every_key_of_the_fixture(K, oracle, E, fixture_lib, fixture_parent, tmp_path):
    records, taxa = fixture_lib
    vb = E["value_bits"]
    o = o_opts(oracle, vb)
    keys, vals = expected_map(oracle, o, records, taxa, fixture_parent)
    load = assert_no_alias(hashes(oracle, keys), FIX_CAPACITY, vb)
    assert len(set(vals.tolist())) >= 5 and (vals == 8).sum() > 100          # LCAs above the species really occur (8 = Enterobacteriaceae)
    res = build_fixture(K, tmp_path / "db", capacity=FIX_CAPACITY)
    print(f"fixture: {len(keys)} distinct minimizers, load {load:.3f}, result {res}")
    assert (res["n_records"], res["n_skipped"], res["capacity"], res["n_nodes"], res["value_bits"]) == (len(records), 2, FIX_CAPACITY, E["n_nodes"], vb)
    assert res["size"] == len(keys) and res["n_cuts"] == 0 and res["n_sampled"] == 0 and res["min_acceptable_hash"] == 0
    assert res["n_bases"] == sum(len(s) for s, t in zip(records, taxa) if t)
    (cells, parent, ext), info = open_export(K, tmp_path / "db")
    assert info["size"] == len(keys) and info["capacity"] == FIX_CAPACITY and (info["value_bits"], info["key_bits"]) == (vb, 32 - vb)
    assert np.array_equal(parent, fixture_parent) and list(ext) == [n["external"] for n in E["nodes"]]
    assert int((cells != 0).sum()) == len(keys)
    check_every_key(oracle, cells, vb, keys, vals)
    # the same table built sequentially gives the same answer for every key: this pins the expectation itself
    seq = sequential_table(oracle, o, records, taxa, fixture_parent, FIX_CAPACITY, vb)
    check_every_key(oracle, seq.cells, vb, keys, vals)
    assert int((seq.cells != 0).sum()) == len(keys)


# ---- a synthetic library: many short records and one long one, in one call and in three -------------------------------------------
@pytest.fixture(scope="module")
def synth_lib(oracle):
    """2 100 short records (35..1 500 bases; some too short, some without a taxon) cut from the last 0.4 Mb of a 2.4 Mb synthetic
    reference, whose first 2.1 Mb are one more record: the short ones overlap each other and the long one, under 7 taxa"""
    P = oracle.ref_params(SYN_SEED, [2_400_000])
    ref = np.asarray(oracle.synth_ref(P, 0, P.genome_len))
    rng = np.random.default_rng(SYN_SEED)
    taxa_pool = [7, 12, 13, 14, 10, 11, 9]
    records, taxa = [], []
    for i in range(2100):
        n = int(rng.integers(20, 1500))
        p = int(rng.integers(2_000_000, 2_400_000 - n))
        records.append(ref[p: p + n].copy())
        taxa.append(0 if i % 97 == 0 else taxa_pool[int(rng.integers(0, len(taxa_pool)))])
    records.insert(1000, ref[:2_100_000].copy())
    taxa.insert(1000, 13)
    records[5] = np.frombuffer(bytes(records[5]).lower(), dtype=np.uint8)          # lower case is ACGT
    return records, taxa


def lib_db(K, E, capacity, min_hash=0):
    tax = K.taxonomy_from_ncbi(os.path.join(GOLD, "nodes.dmp"), os.path.join(GOLD, "names.dmp"), os.path.join(GOLD, "seqid2taxid.map"), [1423])
    d = K.K2Db.create_from_taxonomy(K.default_opts(), capacity, tax)
    assert d.info()["value_bits"] == E["value_bits"]
    if min_hash:
        d.set_min_acceptable_hash(min_hash)
    return d


def test_synthetic_library_in_one_call_and_in_three(K, oracle, E, synth_lib, fixture_parent):
    records, taxa = synth_lib
    assert len(records) >= 2001 and max(len(r) for r in records) >= 2_000_000 and len(set(taxa) - {0}) >= 6
    vb = E["value_bits"]
    o = o_opts(oracle, vb)
    keys, vals = expected_map(oracle, o, records, taxa, fixture_parent)
    load = assert_no_alias(hashes(oracle, keys), SYN_CAPACITY, vb)
    assert len(set(vals.tolist()) - set(taxa)) >= 1          # LCAs that are no record's own taxon
    d1 = lib_db(K, E, SYN_CAPACITY)
    st = d1.insert_library(records, taxa)
    print(f"synthetic: {len(keys)} distinct minimizers, load {load:.3f}, one call {st}")
    assert st["size"] == len(keys) and st["n_runs"] >= len(keys) and st["n_records"] == len(records)
    cells1 = d1.export()[0]
    check_every_key(oracle, cells1, vb, keys, vals)
    assert int((cells1 != 0).sum()) == len(keys)
    d3 = lib_db(K, E, SYN_CAPACITY)
    cut = [0, 700, 1400, len(records)]
    for a, b in zip(cut[:-1], cut[1:]):
        st3 = d3.insert_library(records[a:b], taxa[a:b])
    assert st3["size"] == len(keys)
    cells3 = d3.export()[0]
    check_every_key(oracle, cells3, vb, keys, vals)
    assert int((cells3 != 0).sum()) == len(keys)
    d1.close(); d3.close()


def synth_files(tmp_path, synth_lib, E):
    """the synthetic library as a FASTA file with an id map over the fixture's taxonomy"""
    records, taxa = synth_lib
    ext = [n["external"] for n in E["nodes"]]
    write_fasta(tmp_path / "syn.fna", [(f"syn{i} record {i}", r) for i, r in enumerate(records)], width=100)
    write_map(tmp_path / "syn.map", [(f"syn{i}", ext[t]) for i, t in enumerate(taxa) if t])
    return tmp_path / "syn.fna", tmp_path / "syn.map"


def sampled_count(oracle, o, records):
    """the estimator's number restated with the oracle: distinct minimizers m of all records with (k2o_hash(m) & 1023) < 4"""
    seen = set()
    for seq in records:
        mins, amb = oracle.k2_scan(seq, o)
        for m in np.unique(mins[amb == 0]):
            if (oracle.lib().k2o_hash(int(m)) & 1023) < 4:
                seen.add(int(m))
    return len(seen)


def test_cut_record_equals_uncut(K, oracle, E, synth_lib, fixture_parent, tmp_path):
    """sh_k2_build_run with batches of 300 000 bases: the 2.1 Mb record is cut several times, each piece starting with the k - 1
    bases before it; same table per key, same size, same n_sampled as with one batch"""
    records, taxa = synth_lib
    fna, mp = synth_files(tmp_path, synth_lib, E)
    vb = E["value_bits"]
    o = o_opts(oracle, vb)
    keys, vals = expected_map(oracle, o, records, taxa, fixture_parent)
    n_s = sampled_count(oracle, o, records)          # the estimate is over every record, with or without a taxon
    _, cap, _ = K.capacity_plan(n_s)
    assert_no_alias(hashes(oracle, keys), cap, vb)
    whole = K.build_database([fna], tmp_path / "whole", taxonomy_dir=GOLD, seqid2taxid=mp)
    cutup = K.build_database([fna], tmp_path / "cut", taxonomy_dir=GOLD, seqid2taxid=mp, chunk_bytes=300_000)
    print(f"whole {whole}\ncut   {cutup}")
    assert whole["n_cuts"] == 0 and whole["n_batches"] == 1 and cutup["n_cuts"] >= 6 and cutup["n_batches"] >= 8
    for r in (whole, cutup):
        assert (r["n_sampled"], r["capacity"], r["size"], r["n_records"], r["n_skipped"]) == (n_s, cap, len(keys), len(records), taxa.count(0))
    assert cutup["n_bases"] == whole["n_bases"]
    # the same file given twice (several inputs; 7.5 MB, so the reader's 4 MiB blocks end inside lines of the first copy): every
    # minimizer is inserted and sampled twice, which changes nothing
    twice = K.build_database([fna, fna], tmp_path / "twice", taxonomy_dir=GOLD, seqid2taxid=mp, chunk_bytes=1_000_000)
    assert (twice["n_sampled"], twice["capacity"], twice["size"], twice["n_records"], twice["n_skipped"]) == (n_s, cap, len(keys), 2 * len(records), 2 * taxa.count(0))
    assert twice["n_bases"] == 2 * whole["n_bases"] and twice["n_batches"] >= 7
    for name in ("whole", "cut", "twice"):
        (cells, _, _), info = open_export(K, tmp_path / name)
        assert info["size"] == len(keys)
        check_every_key(oracle, cells, vb, keys, vals)
        assert int((cells != 0).sum()) == len(keys)


def test_record_border(K, oracle, E, fixture_parent):
    """two records whose concatenation holds k-mers that neither has: none of those minimizers is in the table"""
    P = oracle.ref_params(SYN_SEED + 1, [20_000])
    ref = np.asarray(oracle.synth_ref(P, 0, P.genome_len))
    a, b = ref[:7_013].copy(), ref[9_000:17_531].copy()
    vb = E["value_bits"]
    o = o_opts(oracle, vb)
    keys, vals = expected_map(oracle, o, [a, b], [13, 14], fixture_parent)
    assert_no_alias(hashes(oracle, keys), 20_011, vb)
    joined, _ = expected_map(oracle, o, [np.concatenate([a, b])], [13], fixture_parent)
    foreign = np.setdiff1d(joined, keys)
    assert 1 <= len(foreign) <= 34
    d = lib_db(K, E, 20_011)
    st = d.insert_library([a, b], [13, 14])
    assert st["size"] == len(keys)
    cells = d.export()[0]
    check_every_key(oracle, cells, vb, keys, vals)
    check_every_key(oracle, cells, vb, foreign, np.zeros(len(foreign), np.uint32))
    d.close()


# ---- the estimator ------------------------------------------------------------------------------------------------------------
def test_estimator_counts_the_distinct_sampled_minimizers(K, oracle, E, synth_lib, fixture_parent):
    records, taxa = synth_lib
    assert sum(len(r) for r in records) >= 2_000_000
    o = o_opts(oracle, E["value_bits"])
    n_s = sampled_count(oracle, o, records)
    one = K.estimate_capacity(records, batches=1)
    three = K.estimate_capacity(records, batches=3)
    print(f"estimator: oracle {n_s}, one batch {one}, three batches {three}")
    assert one["n_sampled"] == n_s and three["n_sampled"] == n_s
    assert one["estimate"] == 256 * n_s and one["capacity"] == -(-256 * n_s * 10 // 7) and one == three
    # the capacity derived from it holds the real build
    every = [1 if t == 0 else t for t in taxa]          # the estimate is over every record: insert them all
    d = lib_db(K, E, one["capacity"])
    st = d.insert_library(records, every)              # SH_ERR_OOM would raise
    load = st["size"] / one["capacity"]
    print(f"estimator: {st['size']} distinct minimizers in {one['capacity']} cells: load {load:.4f} (aimed at 0.7)")
    assert load <= 0.8
    d.close()


# ---- down-sampling ------------------------------------------------------------------------------------------------------------
def test_max_db_size_keeps_exactly_the_upper_hashes(K, oracle, E, fixture_lib, fixture_parent, tmp_path):
    records, taxa = fixture_lib
    vb = E["value_bits"]
    o = o_opts(oracle, vb)
    keys, vals = expected_map(oracle, o, records, taxa, fixture_parent)
    h = hashes(oracle, keys)
    res = build_fixture(K, tmp_path / "db", capacity=FIX_CAPACITY, max_db_size=2 * FIX_CAPACITY)        # half of the 4 * capacity bytes
    cap, min_hash = FIX_CAPACITY // 2, 1 << 63
    assert (res["capacity"], res["min_acceptable_hash"]) == (cap, min_hash) == K.max_db_size(FIX_CAPACITY, 2 * FIX_CAPACITY)
    kept = h >= np.uint64(min_hash)
    assert 0.4 < kept.mean() < 0.6
    assert_no_alias(h[kept], cap, vb)
    assert res["size"] == int(kept.sum())
    with open(tmp_path / "db" / "opts.k2d", "rb") as f:
        assert struct.unpack_from("<Q", f.read(), 40)[0] == min_hash
    (cells, _, _), info = open_export(K, tmp_path / "db")
    assert int((cells != 0).sum()) == int(kept.sum())
    check_every_key(oracle, cells, vb, keys[kept], vals[kept])
    check_every_key(oracle, cells, vb, keys[~kept], np.zeros(int((~kept).sum()), np.uint32))
    seq = sequential_table(oracle, o, records, taxa, fixture_parent, cap, vb, min_hash=min_hash)
    check_every_key(oracle, seq.cells, vb, keys[kept], vals[kept])


# ---- round trips --------------------------------------------------------------------------------------------------------------
def parse_taxo(path):
    """taxo.k2d by its layout (the one tests/golden/make_k2_pydb.py packs): "K2TAXDAT", node_count, name_data_len, rank_data_len
    (u64), node_count x 7 u64 (parent, first_child, child_count, name_offset, rank_offset, external_id, godparent), the two pools"""
    raw = open(path, "rb").read()
    assert raw[:8] == b"K2TAXDAT"
    n, nl, rl = struct.unpack_from("<3Q", raw, 8)
    assert len(raw) == 32 + 56 * n + nl + rl
    nodes = [struct.unpack_from("<7Q", raw, 32 + 56 * i) for i in range(n)]
    names, ranks = raw[32 + 56 * n: 32 + 56 * n + nl], raw[32 + 56 * n + nl:]
    s = lambda pool, off: pool[off: pool.index(b"\0", off)].decode()
    return [dict(parent=p, first_child=fc, child_count=cc, name=s(names, no), rank=s(ranks, ro), external=e, godparent=g) for p, fc, cc, no, ro, e, g in nodes]


def mutated_reads(records, rng, n, length=150, subs=3):
    out = []
    long_enough = [r for r in records if len(r) >= length]
    for i in range(n):
        r = long_enough[int(rng.integers(0, len(long_enough)))]
        p = int(rng.integers(0, len(r) - length + 1))
        s = np.frombuffer(bytes(r[p: p + length]).upper(), dtype=np.uint8).copy()
        for q in rng.integers(0, length, subs):
            s[q] = ord("ACGT"[int(rng.integers(0, 4))])
        out.append(s)
    return out


def test_cli_and_library_round_trip(K, oracle, E, fixture_lib, fixture_parent, tmp_path):
    records, taxa = fixture_lib
    vb = E["value_bits"]
    res = build_fixture(K, tmp_path / "lib", capacity=FIX_CAPACITY)
    p = subprocess.run([EXE, "k2-build", "-i", os.path.join(GOLD, "library.fna"), "-o", str(tmp_path / "cli"), "-n", GOLD, "-m", os.path.join(GOLD, "seqid2taxid.map"),
                        "--capacity", str(FIX_CAPACITY)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    assert "99999" in p.stderr
    j = json.loads(p.stdout.strip().splitlines()[-1])
    assert (j["records"], j["records_skipped"], j["size"], j["capacity"], j["nodes"]) == (res["n_records"], res["n_skipped"], res["size"], FIX_CAPACITY, E["n_nodes"])
    for name in ("opts.k2d", "taxo.k2d"):
        assert open(tmp_path / "lib" / name, "rb").read() == open(tmp_path / "cli" / name, "rb").read(), name
    opts_raw = open(tmp_path / "lib" / "opts.k2d", "rb").read()
    assert len(opts_raw) == 64 and struct.unpack_from("<4Q", opts_raw) == (35, 31, (0x3ffffffff << 28) | 0x3333333, 0xe37e28c4271b5a2d) and opts_raw[32] == 1
    tx = parse_taxo(tmp_path / "lib" / "taxo.k2d")
    assert len(tx) == E["n_nodes"]
    for got, e in zip(tx[1:], E["nodes"][1:]):
        assert got == dict(parent=e["parent"], first_child=e["first_child"], child_count=e["child_count"], name=e["name"], rank=e["rank"], external=e["external"], godparent=0)
    hdr = struct.unpack_from("<4Q", open(tmp_path / "lib" / "hash.k2d", "rb").read(32))
    assert hdr == (FIX_CAPACITY, res["size"], 32 - vb, vb) and os.path.getsize(tmp_path / "lib" / "hash.k2d") == 32 + 4 * FIX_CAPACITY
    o = o_opts(oracle, vb)
    keys, vals = expected_map(oracle, o, records, taxa, fixture_parent)
    tables = {}
    for name in ("lib", "cli"):
        (cells, parent, ext), info = open_export(K, tmp_path / name)
        check_every_key(oracle, cells, vb, keys, vals)
        tables[name] = (cells, parent, ext)
    # classification through the opened database = the oracle on its exported cells and taxonomy
    rng = np.random.default_rng(11)
    reads = mutated_reads([r for r, t in zip(records, taxa) if t], rng, 600) + [rng.integers(0, 4, 150).astype(np.uint8).view(np.uint8) for _ in range(20)]
    reads = [np.frombuffer(bytes(b"ACGT"[int(x)] for x in r), dtype=np.uint8) if r.max() < 4 else r for r in reads]
    bases = np.concatenate(reads)
    off = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.uint64)
    d = K.K2Db.open(tmp_path / "cli")
    g, st = d.classify(bases, off)
    d.close()
    cells, parent, ext = tables["cli"]
    c = oracle.K2Table(cells, parent, vb).classify(o, bases, off, threads=4)
    for name in ("call", "total_kmers", "hit_groups"):
        assert np.array_equal(g[name], c[name]), name
    assert np.array_equal(g["taxid"], ext[c["call"]]) and st["n_probes"] == int(c["n_probes"].sum())
    assert int((g["call"] != 0).sum()) >= 400 and len(set(g["call"].tolist())) >= 5


def test_single_taxon_database_depletes_exactly_the_oracles_reads(K, oracle, tmp_path):
    """the host-depletion case: one gzipped FASTA under --taxid 9606, capacity estimated; sh_kraken_run -D 9606 removes exactly the
    reads the oracle classifies under that taxon"""
    P = oracle.ref_params(SYN_SEED + 2, [300_000, 150_000])
    ref = np.asarray(oracle.synth_ref(P, 0, P.genome_len))
    contigs = [ref[:300_000], ref[300_000:450_000]]
    write_fasta(tmp_path / "host.fa.gz", [("chr1 synthetic", contigs[0]), ("chr2", contigs[1])], width=60)
    p = subprocess.run([EXE, "k2-build", "-i", str(tmp_path / "host.fa.gz"), "-o", str(tmp_path / "hostdb"), "--taxid", "9606", "--name", "Homo sapiens"],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    j = json.loads(p.stdout.strip().splitlines()[-1])
    o = o_opts(oracle, 2)
    keys, vals = expected_map(oracle, o, contigs, [2, 2], np.array([0, 0, 1], dtype=np.uint32))
    n_s = sampled_count(oracle, o, contigs)
    assert (j["records"], j["records_skipped"], j["bases"], j["nodes"], j["value_bits"], j["n_sampled"]) == (2, 0, 450_000, 3, 2, n_s)
    assert j["size"] == len(keys) and j["capacity"] == K.capacity_plan(n_s)[1] and j["size"] / j["capacity"] <= 0.8
    tx = parse_taxo(tmp_path / "hostdb" / "taxo.k2d")
    assert [(t["external"], t["parent"], t["name"], t["rank"]) for t in tx[1:]] == [(1, 0, "root", "no rank"), (9606, 1, "Homo sapiens", "species")]
    (cells, parent, ext), info = open_export(K, tmp_path / "hostdb")
    assert_no_alias(hashes(oracle, keys), j["capacity"], 2)
    check_every_key(oracle, cells, 2, keys, vals)
    rng = np.random.default_rng(5)
    reads = mutated_reads(contigs, rng, 400) + [np.frombuffer(bytes(b"ACGT"[int(x)] for x in rng.integers(0, 4, 150)), dtype=np.uint8) for _ in range(400)]
    order = rng.permutation(len(reads))
    reads = [reads[i] for i in order]
    with open(tmp_path / "in.fastq", "w") as f:
        for i, r in enumerate(reads):
            f.write(f"@r{i}\n{bytes(r).decode()}\n+\n{'I' * len(r)}\n")
    bases = np.concatenate(reads)
    off = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.uint64)
    c = oracle.K2Table(cells, parent, 2).classify(o, bases, off, threads=4)
    host = {f"r{i}" for i in np.flatnonzero(c["call"] == 2)}
    assert 300 <= len(host) <= 400
    res = K.kraken_run([tmp_path / "in.fastq"], [tmp_path / "out.fastq"], tmp_path / "hostdb", taxa_direct=["9606"], workdir=tmp_path / "w")
    kept = {ln[1:].strip() for ln in open(tmp_path / "out.fastq") if ln.startswith("@r")}
    assert kept == {f"r{i}" for i in range(len(reads))} - host
    assert res["n_depleted_ids"] == len(host)


def test_full_table_is_an_error_that_names_capacity(K, E, fixture_lib, tmp_path):
    from scrubby_amd import lib as S
    with pytest.raises(S.ScrubbyHipError) as ei:
        build_fixture(K, tmp_path / "db", capacity=5_003)          # the fixture has 11 570 distinct minimizers
    assert ei.value.status == 5 and "--capacity" in ei.value.message          # SH_ERR_OOM
    p = subprocess.run([EXE, "k2-build", "-i", os.path.join(GOLD, "library.fna"), "-o", str(tmp_path / "cli"), "-n", GOLD, "-m", os.path.join(GOLD, "seqid2taxid.map"),
                        "--capacity", "5003"], capture_output=True, text=True)
    assert p.returncode == 1 and "--capacity" in p.stderr
    # the device is fine afterwards
    res = build_fixture(K, tmp_path / "db2", capacity=FIX_CAPACITY)
    assert res["size"] > 5_003
