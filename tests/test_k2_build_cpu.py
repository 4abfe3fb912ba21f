"""Database build, host side (no GPU): the NCBI taxonomy reduced to the taxa a library uses and laid out as taxo.k2d stores it,
the taxon of a FASTA header, and kraken2-build's --max-db-size arithmetic.  The fixture and its expectations come from
tests/golden/make_k2_build.py (its own breadth-first walk and header parsing, nothing from the product)."""
import json
import os
import subprocess
import sys

import pytest

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "k2_build")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def K():
    from scrubby_amd import k2
    return k2


@pytest.fixture(scope="module")
def E():
    with open(os.path.join(GOLD, "expected.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def tax(K):
    # the taxid of the library's kraken:taxid header is passed as a caller of the run would (it scans the headers first)
    return K.taxonomy_from_ncbi(os.path.join(GOLD, "nodes.dmp"), os.path.join(GOLD, "names.dmp"), os.path.join(GOLD, "seqid2taxid.map"), [1423])


def pool_str(pool, off):
    return pool[off: pool.index(b"\0", off)].decode()


def test_taxonomy_layout_equals_the_generators_walk(K, E, tax):
    info = tax.info()
    assert info["n_nodes"] == E["n_nodes"] and info["value_bits"] == E["value_bits"]
    assert info["n_map_entries"] == E["n_map_entries"] and info["n_missing_taxa"] == len(E["missing"])
    nodes, names, ranks = tax.arrays()
    assert len(names) == info["names_len"] and len(ranks) == info["ranks_len"]
    n0 = nodes[0]
    assert (n0.parent, n0.first_child, n0.child_count, n0.external_id, n0.godparent) == (0, 0, 0, 0, 0)
    for i, e in enumerate(E["nodes"]):
        n = nodes[i]
        assert (n.external_id, n.parent, n.first_child, n.child_count, n.godparent) == (e["external"], e["parent"], e["first_child"], e["child_count"], 0), i
        if i:
            assert pool_str(names, n.name_offset) == e["name"] and pool_str(ranks, n.rank_offset) == e["rank"], i
            assert tax.internal(e["external"]) == i
    # breadth-first: parents before children, the children of a node consecutive and in ascending external id
    for i in range(2, len(nodes)):
        assert nodes[i].parent < i
    for n in nodes:
        kids = [nodes[j].external_id for j in range(n.first_child, n.first_child + n.child_count)]
        assert kids == sorted(kids)


def test_unused_taxa_are_dropped_and_a_missing_taxid_is_skipped(K, E, tax):
    for t in E["dropped"] + E["missing"]:
        assert tax.internal(t) == 0
    ext = {n.external_id for n in tax.arrays()[0]}
    assert not ext & set(E["dropped"] + E["missing"])


def test_missing_taxid_is_named_once_on_stderr(E):
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from scrubby_amd import k2\n"
            "t = k2.taxonomy_from_ncbi(%r, %r, %r, [99999, 1423])\n"
            "print(t.info()['n_missing_taxa'])\n") % (ROOT, os.path.join(GOLD, "nodes.dmp"), os.path.join(GOLD, "names.dmp"), os.path.join(GOLD, "seqid2taxid.map"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, check=True)
    assert r.stdout.strip() == "1"
    lines = [ln for ln in r.stderr.splitlines() if "99999" in ln]
    assert len(lines) == 1 and "nodes.dmp" in lines[0] and "skipped" in lines[0]


def test_value_bits_more_but_never_fewer(K, E):
    args = (os.path.join(GOLD, "nodes.dmp"), os.path.join(GOLD, "names.dmp"), os.path.join(GOLD, "seqid2taxid.map"), [1423])
    assert K.taxonomy_from_ncbi(*args, value_bits=9).info()["value_bits"] == 9
    from scrubby_amd import lib as S
    with pytest.raises(S.ScrubbyHipError):
        K.taxonomy_from_ncbi(*args, value_bits=E["value_bits"] - 1)
    assert K.taxonomy_single(9606).info()["value_bits"] == 2          # 3 nodes


def test_header_to_taxon_for_every_record(K, E, tax):
    kinds = set()
    for r in E["records"]:
        assert tax.header_taxon(r["header"]) == r["internal"], r["header"]
        kinds.add("skip" if r["internal"] == 0 else "lca" if "\x01" in r["header"] else "tag" if "kraken:taxid|" in r["header"] else "map")
    assert kinds == {"skip", "lca", "tag", "map"}
    # without the header's taxid passed in, and without a map entry, 1423 is still there through seqC; a taxid nobody uses is not
    assert tax.header_taxon("kraken:taxid|564|x") == 0 and tax.header_taxon("kraken:taxid|10710|x") == 0
    # the LCA is of the taxa that are known: an unknown id beside a known one changes nothing
    assert tax.header_taxon("nobody\x01seqD") == tax.internal(9606)
    assert tax.header_taxon("seqA\x01seqD") == tax.internal(131567)
    assert tax.header_taxon("  seqA\tdescription") == tax.internal(562)
    assert tax.header_taxon("") == 0


def test_single_taxon_mode(K):
    t = K.taxonomy_single(9606)
    nodes, names, ranks = t.arrays()
    assert [(n.external_id, n.parent, n.first_child, n.child_count) for n in nodes] == [(0, 0, 0, 0), (1, 0, 2, 1), (9606, 1, 0, 0)]
    assert pool_str(names, nodes[2].name_offset) == "taxid 9606" and pool_str(ranks, nodes[2].rank_offset) == "species"
    assert pool_str(names, nodes[1].name_offset) == "root"
    assert t.header_taxon("chr1 anything at all") == 2 and t.header_taxon("") == 2
    t = K.taxonomy_single(9606, "Homo sapiens", "subspecies")
    nodes, names, ranks = t.arrays()
    assert pool_str(names, nodes[2].name_offset) == "Homo sapiens" and pool_str(ranks, nodes[2].rank_offset) == "subspecies"


def test_max_db_size_arithmetic(K):
    # 1000 cells needed, 2000 bytes allowed: 500 cells, half of the hash range kept: (1 - 2000 / 4000) * 2^64 = 2^63
    assert K.max_db_size(1000, 2000) == (500, 1 << 63)
    # 2^20 cells needed, 2^20 bytes allowed: 2^18 cells, a quarter kept: 0.75 * 2^64
    assert K.max_db_size(1 << 20, 1 << 20) == (1 << 18, 3 << 62)
    # 4 * 1000 = 4000 bytes fit exactly: nothing changes
    assert K.max_db_size(1000, 4000) == (1000, 0) and K.max_db_size(1000, 0) == (1000, 0)
    # through the estimate: 7 sampled -> 1792 -> ceil(1792 / 0.7) = 2560 cells; 5120 bytes hold 1280 = half of them
    assert K.capacity_plan(7) == (1792, 2560, 0)
    assert K.capacity_plan(7, 0.7, 5120) == (1792, 1280, 1 << 63)
    assert K.capacity_plan(7, 0.5) == (1792, 3584, 0)
