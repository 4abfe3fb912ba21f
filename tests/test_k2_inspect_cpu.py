"""Database inspection, the host half: sh_k2_counts_report (kraken2-inspect's report over any taxonomy and one count per node).

The expectation is a restatement, in plain Python, of the rules DESIGN.md §7 "Database inspection" gives (PARITY WITH kraken2-inspect
UNPINNED): a taxon's direct count is its own count, its clade count the sum over its subtree, the total the sum of all counts, no
`U` row; rows are `%6.2f`, clade, direct, rank code with depth suffix, external taxid, name indented two spaces per level; children by
descending clade count, ties by id; taxa with a clade count of 0 only with the zero-counts flag; MPA style prints, for every taxon
whose rank has a letter, the `|`-joined `x__Name` of its lettered ancestors and itself, a tab and the clade count, spaces in names as
`_`, and descends through the taxa that have no letter.  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "k2_build")
LETTER = {"superkingdom": "D", "kingdom": "K", "phylum": "P", "class": "C", "order": "O", "family": "F", "genus": "G", "species": "S"}
NEW_EXPORTS = ["sh_k2_value_counts_device", "sh_k2_value_counts", "sh_k2_counts_report", "sh_k2_inspect_header", "sh_k2_inspect_run"]


@pytest.fixture(scope="module")
def K():
    from scrubby_amd import k2
    return k2


def pool_str(pool, off):
    return pool[off: pool.index(b"\0", off)].decode()


def taxonomy_lists(nodes, names, ranks):
    """(parents, externals, names, ranks) per node from a K2TaxNode array and its two pools"""
    return ([int(n.parent) for n in nodes], [int(n.external_id) for n in nodes], [pool_str(names, n.name_offset) for n in nodes],
            [pool_str(ranks, n.rank_offset) for n in nodes])


def expected_report(parents, exts, names, ranks, counts, zero=False, mpa=False, header=""):
    n = len(parents)
    counts = [int(c) for c in counts]
    clade = list(counts)
    clade[0] = 0
    for i in range(n - 1, 1, -1):
        clade[parents[i]] += clade[i]
    total = sum(counts[1:]) or 1
    kids = {i: [j for j in range(2, n) if parents[j] == i] for i in range(n)}
    out = [header]

    def walk(i, depth, code, cd, path):
        if not (clade[i] or zero):
            return
        letter = LETTER.get(ranks[i])
        if i != 1:
            code, cd = (letter, 0) if letter else (code, cd + 1)
        if mpa:
            if letter:
                path = path + [letter.lower() + "__" + names[i].replace(" ", "_")]
                out.append("|".join(path) + "\t%d\n" % clade[i])
        else:
            out.append("%6.2f\t%d\t%d\t%s\t%d\t%s%s\n" % (100.0 * clade[i] / total, clade[i], counts[i], code + (str(cd) if cd else ""), exts[i],
                                                          "  " * depth, names[i]))
        for j in sorted(kids[i], key=lambda j: (-clade[j], j)):
            walk(j, depth + 1, code, cd, path)

    walk(1, 0, "R", 0, [])
    return "".join(out).encode()


def run_report(K, tax, counts, tmp_path, **kw):
    p = tmp_path / "report.txt"
    K.counts_report(*tax, counts, p, **kw)
    return p.read_bytes()


@pytest.fixture(scope="module")
def fixture_tax(K):
    t = K.taxonomy_from_ncbi(os.path.join(GOLD, "nodes.dmp"), os.path.join(GOLD, "names.dmp"), os.path.join(GOLD, "seqid2taxid.map"), [1423])
    return t.arrays()


@pytest.mark.parametrize("zero,mpa", [(False, False), (True, False), (False, True), (True, True)])
def test_report_over_the_fixture_taxonomy(K, fixture_tax, tmp_path, zero, mpa):
    lists = taxonomy_lists(*fixture_tax)
    n = len(lists[0])
    assert n >= 10 and len({r for r in lists[3] if r in LETTER}) >= 4 and any(r not in LETTER for r in lists[3][2:])
    for seed in (20261018, 7):
        rng = np.random.default_rng(seed)
        counts = rng.integers(0, 5000, n).astype(np.uint64)
        counts[rng.random(n) < 0.4] = 0          # whole subtrees without minimizers
        counts[0] = 0
        got = run_report(K, fixture_tax, counts, tmp_path, zero_counts=zero, mpa=mpa)
        exp = expected_report(*lists, counts, zero, mpa)
        assert got == exp
        assert len(exp.splitlines()) >= 3
    if zero and not mpa:
        assert len(got.splitlines()) == n - 1          # every taxon


def small_tax(K, parents, exts, names, ranks):
    return K.make_taxonomy(parents, exts, names, ranks), (parents, exts, names, ranks)


def test_all_counts_zero(K, fixture_tax, tmp_path):
    lists = taxonomy_lists(*fixture_tax)
    n = len(lists[0])
    z = np.zeros(n, dtype=np.uint64)
    assert run_report(K, fixture_tax, z, tmp_path) == b""
    assert run_report(K, fixture_tax, z, tmp_path, mpa=True) == b""
    got = run_report(K, fixture_tax, z, tmp_path, zero_counts=True)
    assert got == expected_report(*lists, z, True) and len(got.splitlines()) == n - 1
    assert all(ln.startswith(b"  0.00\t0\t0\t") for ln in got.splitlines())
    assert run_report(K, fixture_tax, z, tmp_path, zero_counts=True, mpa=True) == expected_report(*lists, z, True, True)


def test_root_only(K, tmp_path):
    tax, lists = small_tax(K, [0, 0], [0, 1], ["", "root"], ["", "no rank"])
    assert run_report(K, tax, [0, 5], tmp_path) == b"100.00\t5\t5\tR\t1\troot\n" == expected_report(*lists, [0, 5])
    assert run_report(K, tax, [0, 5], tmp_path, mpa=True) == b""
    assert run_report(K, tax, [0, 0], tmp_path, zero_counts=True) == b"  0.00\t0\t0\tR\t1\troot\n"


def test_names_with_spaces_ties_and_unlettered_ranks(K, tmp_path):
    # root -> cellular organisms (no rank) -> two genera with EQUAL clade counts -> species; a subspecies below one species
    parents = [0, 0, 1, 2, 2, 3, 3, 4, 5]
    exts = [0, 1, 131567, 561, 9605, 562, 564, 9606, 83333]
    names = ["", "root", "cellular organisms", "Escherichia", "Homo", "Escherichia coli", "Escherichia fergusonii", "Homo sapiens", "Escherichia coli K-12"]
    ranks = ["", "no rank", "no rank", "genus", "genus", "species", "species", "species", "strain"]
    tax, lists = small_tax(K, parents, exts, names, ranks)
    counts = [0, 1, 2, 3, 10, 4, 2, 0, 1]          # clade(Escherichia) = 3 + 4 + 2 + 1 = 10 = clade(Homo): id 3 comes before id 4
    plain = run_report(K, tax, counts, tmp_path)
    assert plain == expected_report(*lists, counts)
    rows = plain.decode().splitlines()
    assert [r.split("\t")[4] for r in rows] == ["1", "131567", "561", "562", "83333", "564", "9605"]
    assert [r.split("\t")[3] for r in rows] == ["R", "R1", "G", "S", "S1", "S", "G"]
    assert rows[4].endswith("\t        Escherichia coli K-12")
    mpa = run_report(K, tax, counts, tmp_path, mpa=True)
    assert mpa == expected_report(*lists, counts, mpa=True)
    assert mpa.decode().splitlines() == ["g__Escherichia\t10", "g__Escherichia|s__Escherichia_coli\t5", "g__Escherichia|s__Escherichia_fergusonii\t2", "g__Homo\t10"]
    mz = run_report(K, tax, counts, tmp_path, mpa=True, zero_counts=True)
    assert mz == expected_report(*lists, counts, True, True) and mz.decode().splitlines()[-1] == "g__Homo|s__Homo_sapiens\t0"


def test_header_is_written_verbatim(K, fixture_tax, tmp_path):
    lists = taxonomy_lists(*fixture_tax)
    counts = np.arange(len(lists[0]), dtype=np.uint64)
    h = "# anything at all\nno hash, two  spaces\t\x01\n# no newline at the end"
    assert run_report(K, fixture_tax, counts, tmp_path, header=h) == expected_report(*lists, counts, header=h)
    assert run_report(K, fixture_tax, counts, tmp_path, header=h, mpa=True) == expected_report(*lists, counts, mpa=True, header=h)


def test_errors(K, fixture_tax, tmp_path):
    from scrubby_amd import lib as S
    nodes, names, ranks = fixture_tax
    counts = np.ones(len(nodes), dtype=np.uint64)
    with pytest.raises(S.ScrubbyHipError) as ei:
        K.counts_report(nodes, names, ranks, counts, tmp_path / "no_such_directory" / "report.txt")
    assert ei.value.status == 7          # SH_ERR_IO
    L = S.load()
    args = [nodes, C.c_uint64(len(nodes)), names, C.c_uint64(len(names)), ranks, C.c_uint64(len(ranks)), C.c_void_p(counts.ctypes.data), 0, None,
            str(tmp_path / "x.txt").encode()]
    assert L.sh_k2_counts_report(*args) == 0
    for null_at in (0, 2, 4, 6):          # nodes, names, ranks, counts
        a = list(args)
        a[null_at] = None
        assert L.sh_k2_counts_report(*a) == 1, null_at          # SH_ERR_BAD_ARG
    assert L.sh_k2_inspect_header(None, None, C.c_uint64(0), None) == 1
    assert L.sh_k2_value_counts(None, None, None) == 1 and L.sh_k2_value_counts_device(None, None, None, None) == 1
    assert L.sh_k2_inspect_run(None, None) == 1


def test_version_and_exports():
    from scrubby_amd import lib as S
    L = S.load()
    assert L.sh_version() == 104
    for name in NEW_EXPORTS:
        assert name in S.EXPORTS and hasattr(L, name), name
