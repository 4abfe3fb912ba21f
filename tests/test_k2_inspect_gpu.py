"""Database inspection on the GPU: k_k2_value_counts (sh_k2_value_counts[_device]), sh_k2_inspect_header, sh_k2_inspect_run and
`scrubby-hip k2-inspect`.

The tests write their databases themselves, in plain struct / NumPy after the layouts in the docstring of tests/golden/make_k2_pydb.py
(opts.k2d 64 bytes; taxo.k2d "K2TAXDAT", three uint64, nodes of 7 x uint64, the name and rank pools; hash.k2d four uint64 and the
cells), so every cell is theirs.  The ground truth is NumPy on the array the test wrote, np.bincount(cells[cells != 0] & mask), never a
second call of the code under test; integer adds only, so every comparison is `==`.  PARITY WITH kraken2-inspect UNPINNED."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from tests.test_k2_build_gpu import (E, FIX_CAPACITY, GOLD as BUILD_GOLD, build_fixture, expected_map, fixture_lib, fixture_parent,  # noqa: F401
                                     o_opts)
from tests.test_k2_inspect_cpu import expected_report, taxonomy_lists

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PYDB = os.path.join(HERE, "golden", "k2_pydb")
EXE = os.path.join(os.path.dirname(HERE), "scrubby_amd", "scrubby-hip")
K_, L_ = 35, 31
SPACED = (0x3ffffffff << 28) | 0x3333333
TOGGLE = 0xe37e28c4271b5a2d
BLOCKS, LDS_BINS = "SCRUBBY_HIP_K2_INSPECT_BLOCKS", "SCRUBBY_HIP_K2_INSPECT_LDS_BINS"

# the 13-node taxonomy of tests/golden/make_k2_pydb.py: name, rank, external id, parent
TAXA13 = [("", "", 0, 0), ("root", "no rank", 1, 0), ("Bacteria", "superkingdom", 2, 1), ("Eukaryota", "superkingdom", 2759, 1),
          ("Pseudomonadota", "phylum", 1224, 2), ("Chordata", "phylum", 7711, 3), ("Escherichia", "genus", 561, 4), ("Homo", "genus", 9605, 5),
          ("Pan", "genus", 9596, 5), ("Escherichia coli", "species", 562, 6), ("Homo sapiens", "species", 9606, 7),
          ("Homo neanderthalensis", "species", 63221, 7), ("Pan troglodytes", "species", 9598, 8)]
TAXA3 = [("", "", 0, 0), ("root", "no rank", 1, 0), ("Homo sapiens", "species", 9606, 1)]
TAXA2 = TAXA3[:2]


@pytest.fixture(scope="module")
def K():
    from scrubby_amd import lib, k2
    lib.require_gpu()
    return k2


def heap_taxa(n):
    """n nodes, node i >= 2 under node i // 2: breadth-first ids, children consecutive"""
    return [("", "", 0, 0), ("root", "no rank", 1, 0)] + [("t%d" % i, "no rank", 100 + i, i // 2) for i in range(2, n)]


def write_taxo(path, taxa):
    n = len(taxa)
    parent = np.array([t[3] for t in taxa], dtype=np.uint64)
    nodes = np.zeros((n, 7), dtype="<u8")
    nodes[:, 0] = parent
    kid = np.arange(2, n, dtype=np.uint64)
    first = np.full(n, n, dtype=np.uint64)
    np.minimum.at(first, parent[2:].astype(np.int64), kid)
    count = np.bincount(parent[2:].astype(np.int64), minlength=n).astype(np.uint64)
    nodes[:, 1] = np.where(count > 0, first, 0)
    nodes[:, 2] = count
    name_len = np.array([len(t[0].encode()) + 1 for t in taxa], dtype=np.uint64)
    nodes[:, 3] = np.cumsum(name_len) - name_len
    rank_list = []
    for t in taxa:
        if t[1] not in rank_list:
            rank_list.append(t[1])
    rank_off = {r: sum(len(x) + 1 for x in rank_list[:i]) for i, r in enumerate(rank_list)}
    nodes[:, 4] = [rank_off[t[1]] for t in taxa]
    nodes[:, 5] = [t[2] for t in taxa]
    names = b"".join(t[0].encode() + b"\0" for t in taxa)
    ranks = b"".join(r.encode() + b"\0" for r in rank_list)
    with open(path, "wb") as f:
        f.write(b"K2TAXDAT" + struct.pack("<QQQ", n, len(names), len(ranks)) + nodes.tobytes() + names + ranks)


def write_db(d, cells, value_bits, taxa, size=None, min_hash=0):
    os.makedirs(d)
    cells = np.ascontiguousarray(cells, dtype="<u4")
    with open(os.path.join(d, "opts.k2d"), "wb") as f:
        f.write(struct.pack("<QQQQB7xQiii4x", K_, L_, SPACED, TOGGLE, 1, min_hash, 1, 0, 0))
    write_taxo(os.path.join(d, "taxo.k2d"), taxa)
    with open(os.path.join(d, "hash.k2d"), "wb") as f:
        f.write(struct.pack("<QQQQ", len(cells), int((cells != 0).sum()) if size is None else size, 32 - value_bits, value_bits))
        f.write(cells.tobytes())
    return str(d)


def make_cells(rng, values, value_bits, load):
    """cell i = random truncated key << value_bits | values[i], or 0 (empty) with probability 1 - load"""
    n = len(values)
    keys = rng.integers(0, 1 << (32 - value_bits), n, dtype=np.uint64)
    cells = (keys << np.uint64(value_bits) | np.asarray(values, dtype=np.uint64)).astype(np.uint32)
    if load < 1.0:
        cells[rng.random(n) >= load] = 0
    return cells


def truth(cells, value_bits, n_nodes):
    return np.bincount(cells[cells != 0] & np.uint32((1 << value_bits) - 1), minlength=n_nodes).astype(np.uint64)


def check_db(K, path, cells, value_bits, n_nodes, monkeypatch=None, switches=({},)):
    """opens the database once and compares value_counts() with NumPy under every setting of the switches"""
    exp = truth(cells, value_bits, n_nodes)
    d = K.K2Db.open(path)
    try:
        for sw in switches:
            for name in (BLOCKS, LDS_BINS):
                if name in sw:
                    monkeypatch.setenv(name, str(sw[name]))
                elif monkeypatch is not None:
                    monkeypatch.delenv(name, raising=False)
            counts, st = d.value_counts(return_stats=True)
            assert counts.dtype == np.uint64 and np.array_equal(counts, exp), (sw, np.flatnonzero(counts != exp)[:5])
            assert (st["n_cells"], st["n_occupied"], st["n_bad_values"]) == (len(cells), int((cells != 0).sum()), 0), sw
    finally:
        d.close()
    return exp


def parse_taxo(path):
    from scrubby_amd import k2
    raw = open(path, "rb").read()
    n, nl, rl = struct.unpack_from("<QQQ", raw, 8)
    nodes = (k2.K2TaxNode * n).from_buffer_copy(raw[32: 32 + 56 * n])
    return nodes, raw[32 + 56 * n: 32 + 56 * n + nl], raw[32 + 56 * n + nl: 32 + 56 * n + nl + rl]


def pydb_cells():
    raw = open(os.path.join(PYDB, "hash.k2d"), "rb").read()
    cap, size, kb, vb = struct.unpack_from("<QQQQ", raw, 0)
    return np.frombuffer(raw, dtype="<u4", offset=32, count=cap), size, vb


def header_lines(k, l, spaced, toggle, n_nodes, size, capacity, min_hash):
    return ("# Database options: nucleotide db, k = %d, l = %d\n# Spaced mask = %s\n# Toggle mask = %s\n# Total taxonomy nodes: %d\n"
            "# Table size: %d\n# Table capacity: %d\n# Min clear hash value = %d\n"
            % (k, l, format(spaced & ((1 << (2 * l)) - 1), "0%db" % (2 * l)), format(toggle, "064b"), n_nodes, size, capacity, min_hash))


# ---- 1. the fixture database ---------------------------------------------------------------------------------------------------------
def test_fixture_database(K):
    cells, size, vb = pydb_cells()
    assert (len(cells), size, vb) == (4099, 736, 6)
    exp = check_db(K, PYDB, cells, vb, 13)
    assert int(exp.sum()) == 736 and exp[0] == 0
    d = K.K2Db.open(PYDB)
    try:
        assert d.inspect_header() == header_lines(35, 31, SPACED, TOGGLE, 13, 736, 4099, 0)
        assert d.inspect_header().splitlines()[1] == "# Spaced mask = " + format(SPACED, "062b")
    finally:
        d.close()


# ---- 2. small capacities and tails ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("capacity", [1, 2, 3, 4, 5, 7, 63, 64, 65, 255, 257, 1023, 1025])
def test_small_capacities_and_tails(K, tmp_path, capacity):
    for seed in (1, 2):          # two seeded tables per capacity (at capacity 1 one of them is the single occupied cell)
        rng = np.random.default_rng(1000 * capacity + seed)
        cells = make_cells(rng, rng.integers(1, 3, capacity), 2, 0.7)
        if capacity == 1 and seed == 1:
            cells[:] = 1 << 2 | 2
        check_db(K, write_db(tmp_path / ("db%d" % seed), cells, 2, TAXA3), cells, 2, 3)


# ---- 3. single taxon -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("load", [0.7, 1.0])
def test_single_taxon(K, tmp_path, monkeypatch, load):
    n = (1 << 22) + 1
    rng = np.random.default_rng(3)
    cells = make_cells(rng, np.full(n, 2), 2, load)
    exp = check_db(K, write_db(tmp_path / "db", cells, 2, TAXA3), cells, 2, 3, monkeypatch, ({}, {BLOCKS: 1}))
    assert exp[2] == (cells != 0).sum() and exp[1] == 0


# ---- 4. patterns around the uniform-wave test ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ["waves", "lanes", "alternating", "one_differs"])
def test_patterns_around_the_uniform_wave(K, tmp_path, monkeypatch, pattern):
    n = 1 << 20
    i = np.arange(n, dtype=np.uint64)
    rng = np.random.default_rng(4)
    if pattern == "waves":
        v = 1 + (i // 256) % 2
    elif pattern == "lanes":
        v = 1 + (i // 4) % 2
    elif pattern == "alternating":
        v = 1 + i % 2
    else:
        v = np.full(n, 1, dtype=np.uint64)
        v[777_777] = 2          # exactly one cell in 2^20 differs
    for load in (1.0, 0.7):
        cells = make_cells(rng, v, 2, load)
        if pattern == "one_differs":
            cells[777_777] = 5 << 2 | 2
            assert truth(cells, 2, 3)[2] == 1
        check_db(K, write_db(tmp_path / ("db%d" % int(load * 10)), cells, 2, TAXA3), cells, 2, 3, monkeypatch, ({}, {BLOCKS: 2}))


# ---- 5. / 6. diverse tables: the LDS bins, the HBM adds, and both at once -------------------------------------------------------------------
@pytest.fixture(scope="module")
def diverse13(tmp_path_factory):
    n = (1 << 22) + 3
    rng = np.random.default_rng(5)
    cells = make_cells(rng, rng.integers(1, 13, n), 6, 0.7)
    return write_db(tmp_path_factory.mktemp("diverse13") / "db", cells, 6, TAXA13), cells


def test_diverse_lds_path(K, diverse13, monkeypatch):
    path, cells = diverse13
    exp = check_db(K, path, cells, 6, 13, monkeypatch, ({}, {BLOCKS: 1}, {BLOCKS: 3}))
    assert (exp[1:] > 100_000).all()


def test_hbm_path_and_the_border_between_the_two(K, diverse13, monkeypatch):
    path, cells = diverse13
    # no LDS bins at all; then ids 1..4 in LDS and 5..12 in HBM, from one block and from many
    check_db(K, path, cells, 6, 13, monkeypatch, ({LDS_BINS: 0}, {LDS_BINS: 0, BLOCKS: 3}, {LDS_BINS: 5}, {LDS_BINS: 5, BLOCKS: 1}))


def test_large_taxonomy(K, tmp_path, monkeypatch):
    n_nodes, vb, n = 70_001, 17, (1 << 22) + 3
    rng = np.random.default_rng(6)
    hot = np.concatenate([rng.choice(np.arange(1, 4096), 10, replace=False), rng.choice(np.arange(4096, n_nodes), 10, replace=False)])
    v = rng.integers(1, n_nodes, n)
    half = rng.random(n) < 0.5
    v[half] = hot[rng.integers(0, 20, int(half.sum()))]
    cells = make_cells(rng, v, vb, 0.7)
    exp = check_db(K, write_db(tmp_path / "db", cells, vb, heap_taxa(n_nodes)), cells, vb, n_nodes, monkeypatch,
                   ({}, {BLOCKS: 3}, {LDS_BINS: 0}, {LDS_BINS: 16384}))
    assert exp[hot].min() > 50_000 and exp[n_nodes - 1] > 0


# ---- 7. extreme value_bits -------------------------------------------------------------------------------------------------------------
def test_extreme_value_bits(K, tmp_path):
    rng = np.random.default_rng(7)
    n = 100_003
    cells = make_cells(rng, rng.integers(1, 13, n), 31, 0.7)          # key_bits 1
    assert (cells >> 31).any() and not (cells >> 31).all()
    check_db(K, write_db(tmp_path / "vb31", cells, 31, TAXA13), cells, 31, 13)
    cells = make_cells(rng, np.ones(n, dtype=np.uint64), 1, 0.7)      # root only
    exp = check_db(K, write_db(tmp_path / "vb1", cells, 1, TAXA2), cells, 1, 2)
    assert exp[1] == (cells != 0).sum()


# ---- 8. bad values ---------------------------------------------------------------------------------------------------------------------
def test_bad_values_are_counted_and_nothing_else(K, tmp_path):
    from scrubby_amd import lib as S
    n, vb = 1 << 20, 6
    rng = np.random.default_rng(8)
    cells = make_cells(rng, rng.integers(1, 13, n), vb, 0.7)
    for at, value in ((5, 13), (300_001, 40), (n - 1, 63)):          # values outside the taxonomy of 13 nodes
        cells[at] = 7 << vb | value
    for at in (6, 900_000):                                          # occupied, value 0
        cells[at] = 9 << vb
    v = cells & np.uint32(63)
    good = (cells != 0) & (v != 0) & (v < 13)
    assert int(((cells != 0) & ~good).sum()) == 5
    exp = np.bincount(v[good], minlength=13).astype(np.uint64)
    path = write_db(tmp_path / "db", cells, vb, TAXA13)
    d = K.K2Db.open(path)
    try:
        counts, st = d.value_counts(return_stats=True)
    finally:
        d.close()
    assert st["n_bad_values"] == 5 and st["n_occupied"] == int((cells != 0).sum()) and st["n_cells"] == n
    assert np.array_equal(counts, exp) and int(counts.sum()) == st["n_occupied"] - 5
    with pytest.raises(S.ScrubbyHipError) as ei:
        K.inspect_database(path, output=tmp_path / "report.txt")
    assert ei.value.status == 7 and "5" in str(ei.value)          # SH_ERR_IO, naming the count
    assert not (tmp_path / "report.txt").exists()


# ---- 9. built databases ------------------------------------------------------------------------------------------------------------------
def test_built_databases(K, oracle, E, fixture_lib, fixture_parent, tmp_path):  # noqa: F811
    records, taxa = fixture_lib
    vb = E["value_bits"]
    keys, vals = expected_map(oracle, o_opts(oracle, vb), records, taxa, fixture_parent)
    res = build_fixture(K, tmp_path / "db", capacity=FIX_CAPACITY)
    d = K.K2Db.open(tmp_path / "db")
    try:
        counts, st = d.value_counts(return_stats=True)
        info = d.info()
    finally:
        d.close()
    assert np.array_equal(counts, np.bincount(vals, minlength=E["n_nodes"]).astype(np.uint64))
    assert int(counts.sum()) == info["size"] == st["n_occupied"] == res["size"] == len(keys) and st["n_bad_values"] == 0
    one = K.build_database([os.path.join(BUILD_GOLD, "library.fna")], tmp_path / "one", taxid=9606, name="Homo sapiens", capacity=FIX_CAPACITY)
    d = K.K2Db.open(tmp_path / "one")
    try:
        counts = d.value_counts()
        assert d.info()["n_nodes"] == 3
    finally:
        d.close()
    assert one["size"] > 1000 and counts.tolist() == [0, 0, one["size"]]


# ---- 10. a table changed in process ---------------------------------------------------------------------------------------------------------
def test_counts_follow_inserts(K):
    o = K.default_opts()
    o.value_bits = 4
    d = K.K2Db.create(o, 100_003, [t[3] for t in TAXA13], [t[2] for t in TAXA13], [t[0] for t in TAXA13], [t[1] for t in TAXA13])
    try:
        assert d.value_counts().tolist() == [0] * 13
        rng = np.random.default_rng(10)
        seen = []
        for n in (20_000, 30_000):
            d.insert(rng.integers(1, 1 << 62, n, dtype=np.uint64), rng.integers(1, 13, n).astype(np.uint32))
            cells = d.export()[0]
            counts, st = d.value_counts(return_stats=True)
            assert np.array_equal(counts, truth(cells, 4, 13)) and st["n_occupied"] == int((cells != 0).sum())
            seen.append(int(counts.sum()))
        assert 19_000 < seen[0] < seen[1]
    finally:
        d.close()


# ---- 11. the device form ------------------------------------------------------------------------------------------------------------------
def test_device_form(K, diverse13):
    import torch
    path, cells = diverse13
    exp = truth(cells, 6, 13)
    d = K.K2Db.open(path)
    try:
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            out = torch.full((13,), -1, dtype=torch.int64, device="cuda")
        assert d.value_counts_device(out, stream=s) is None          # no statistics: the call only enqueues
        assert d.value_counts_device(out, stream=s) is None          # overwrites, does not accumulate
        s.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint64), exp)
        st = d.value_counts_device(out, stream=s, stats=True)       # with statistics the call has waited
        assert np.array_equal(out.cpu().numpy().view(np.uint64), exp)
        assert (st["n_cells"], st["n_occupied"], st["n_bad_values"]) == (len(cells), int((cells != 0).sum()), 0) and st["ms"] > 0
        with torch.cuda.stream(s):                                    # stream=None: the current stream
            assert d.value_counts_device(out) is None
        s.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint64), exp)
    finally:
        d.close()


# ---- 12. sh_k2_inspect_run and the command line ------------------------------------------------------------------------------------------------
def test_run_and_cli(K, tmp_path):
    nodes, names, ranks = parse_taxo(os.path.join(PYDB, "taxo.k2d"))
    lists = taxonomy_lists(nodes, names, ranks)
    cells, size, vb = pydb_cells()
    exp_counts = truth(cells, vb, 13)
    d = K.K2Db.open(PYDB)
    try:
        header, counts = d.inspect_header(), d.value_counts()
    finally:
        d.close()
    assert header == header_lines(35, 31, SPACED, TOGGLE, 13, 736, 4099, 0) and np.array_equal(counts, exp_counts)
    for flags, kw in (([], {}), (["--report-zero-counts"], {"zero_counts": True}), (["--use-mpa-style"], {"mpa": True}),
                      (["--use-mpa-style", "--report-zero-counts"], {"mpa": True, "zero_counts": True})):
        res = K.inspect_database(PYDB, output=tmp_path / "lib.txt", report_zero_counts=kw.get("zero_counts", False), use_mpa_style=kw.get("mpa", False))
        from_lib = (tmp_path / "lib.txt").read_bytes()
        K.counts_report(nodes, names, ranks, counts, tmp_path / "direct.txt", header=header, **kw)
        assert from_lib == (tmp_path / "direct.txt").read_bytes()
        assert from_lib == expected_report(*lists, exp_counts, kw.get("zero_counts", False), kw.get("mpa", False), header=header)
        p = subprocess.run([EXE, "k2-inspect", "-d", PYDB] + flags, capture_output=True)
        assert p.returncode == 0, p.stderr
        assert p.stdout == from_lib
        assert (res["capacity"], res["size_header"], res["n_occupied"], res["n_bad_values"], res["n_nodes"]) == (4099, 736, 736, 0, 13)
        assert res["n_taxa_with_minimizers"] == int((exp_counts != 0).sum())
    assert len(from_lib.splitlines()) > 7
    p = subprocess.run([EXE, "k2-inspect", "-d", PYDB, "-o", str(tmp_path / "cli.txt")], capture_output=True)
    assert p.returncode == 0 and p.stdout == b""
    K.inspect_database(PYDB, output=tmp_path / "lib.txt")
    assert (tmp_path / "cli.txt").read_bytes() == (tmp_path / "lib.txt").read_bytes()
    p = subprocess.run([EXE, "k2-inspect", "-d", PYDB, "--skip-counts"], capture_output=True)
    assert p.returncode == 0 and p.stdout == header.encode()
    res = K.inspect_database(PYDB, output=tmp_path / "skip.txt", skip_counts=True)
    assert (tmp_path / "skip.txt").read_bytes() == header.encode() and res["n_occupied"] == 0 and res["s_count"] == 0
    p = subprocess.run([EXE, "k2-inspect", "-d", str(tmp_path / "no_such_db")], capture_output=True)
    assert p.returncode == 1 and p.stdout == b"" and b"no_such_db" in p.stderr


def test_header_size_that_differs_is_named_and_printed(K, tmp_path):
    """the header's `size` is taken on trust by sh_k2_open: inspection says so on stderr and prints the header's value, as Kraken 2 does"""
    rng = np.random.default_rng(12)
    cells = make_cells(rng, rng.integers(1, 13, 5000), 6, 0.7)
    occupied = int((cells != 0).sum())
    path = write_db(tmp_path / "db", cells, 6, TAXA13, size=occupied + 11, min_hash=1 << 60)
    p = subprocess.run([EXE, "k2-inspect", "-d", path], capture_output=True)
    assert p.returncode == 0
    assert p.stdout.startswith(header_lines(35, 31, SPACED, TOGGLE, 13, occupied + 11, 5000, 1 << 60).encode())
    assert p.stderr.decode().count("the header says %d cells are in use, the table holds %d" % (occupied + 11, occupied)) == 1
