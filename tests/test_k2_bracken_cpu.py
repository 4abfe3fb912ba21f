"""Abundance re-estimation without a GPU: the ctypes mirrors against the C header (a tiny host program), the exports, and the
host-only entries (sh_k2_distrib_write / _read, sh_k2_bracken_estimate / _write, sh_k2_bracken_run) against tests/k2_bracken_ref.py
- the model written from the header's definitions - on the committed fixture tests/golden/k2_bracken/fixture.json
(tests/golden/make_k2_bracken.py).  PARITY WITH Bracken's own programs UNPINNED."""
import ctypes as C
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from tests import k2_bracken_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "k2_bracken")
EXE = os.path.join(ROOT, "scrubby_amd", "scrubby-hip")

PROG = r"""
#include <stdio.h>
#include <stddef.h>
#include "scrubby_hip.h"
#define S(t) printf("%zu ", sizeof(t))
#define O(t, f) printf("%zu ", offsetof(t, f))
int main(void)
{
    S(sh_k2_distrib_entry); O(sh_k2_distrib_entry, mapped); O(sh_k2_distrib_entry, windows);
    S(sh_k2_distrib_stats); O(sh_k2_distrib_stats, n_windows); O(sh_k2_distrib_stats, n_items); O(sh_k2_distrib_stats, n_big); O(sh_k2_distrib_stats, ms);
    S(sh_k2_bracken_row); O(sh_k2_bracken_row, assigned); O(sh_k2_bracken_row, new_est); O(sh_k2_bracken_row, added); O(sh_k2_bracken_row, fraction);
    S(sh_k2_bracken_summary); O(sh_k2_bracken_summary, reads_undistributed); O(sh_k2_bracken_summary, new_est_total);
    S(sh_k2_distrib_config); O(sh_k2_distrib_config, input); O(sh_k2_distrib_config, n_input); O(sh_k2_distrib_config, read_len);
    O(sh_k2_distrib_config, seqid2taxid); O(sh_k2_distrib_config, taxid); O(sh_k2_distrib_config, output); O(sh_k2_distrib_config, chunk_bytes);
    O(sh_k2_distrib_config, device);
    S(sh_k2_distrib_result); O(sh_k2_distrib_result, n_windows); O(sh_k2_distrib_result, n_entries); O(sh_k2_distrib_result, s_open); O(sh_k2_distrib_result, s_total);
    S(sh_k2_bracken_config); O(sh_k2_bracken_config, report); O(sh_k2_bracken_config, read_len); O(sh_k2_bracken_config, level); O(sh_k2_bracken_config, threshold);
    O(sh_k2_bracken_config, kmer_distrib); O(sh_k2_bracken_config, output);
    S(sh_k2_bracken_result); O(sh_k2_bracken_result, n_report_rows); O(sh_k2_bracken_result, n_unknown_taxa);
    printf("%d\n", SH_VERSION);
    return 0;
}
"""


@pytest.fixture(scope="module")
def K():
    from scrubby_amd import k2
    return k2


@pytest.fixture(scope="module")
def F():
    with open(os.path.join(GOLD, "fixture.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def tax(K, F):
    """(nodes, name pool, rank pool, parent, external, names, ranks) of the fixture's taxonomy"""
    cols = [[n[c] for n in F["nodes"]] for c in ("parent", "external", "name", "rank")]
    nodes, npool, rpool = K.make_taxonomy(*cols)
    return (nodes, npool, rpool, *cols)


def entries_array(K, entries):
    return np.array(sorted((g, m, w) for (g, m), w in entries.items()), dtype=K.DISTRIB_DTYPE) if entries else np.zeros(0, dtype=K.DISTRIB_DTYPE)


def fixture_maps(F):
    entries = {(g, m): w for g, m, w in F["entries"]}
    totals = {i: t for i, t in enumerate(F["totals"]) if t}
    return entries, totals


def test_ctypes_layouts_match_the_header(K, tmp_path):
    src, exe = tmp_path / "abi.c", tmp_path / "abi"
    src.write_text(PROG)
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    st, row, sm, dc, dr, bc, br = K.K2DistribStats, K.K2BrackenRow, K.K2BrackenSummary, K.K2DistribConfig, K.K2DistribResult, K.K2BrackenConfig, K.K2BrackenResult
    e = K.DISTRIB_DTYPE
    want = [e.itemsize, e.fields["mapped"][1], e.fields["windows"][1],
            C.sizeof(st), st.n_windows.offset, st.n_items.offset, st.n_big.offset, st.ms.offset,
            C.sizeof(row), row.assigned.offset, row.new_est.offset, row.added.offset, row.fraction.offset,
            C.sizeof(sm), sm.reads_undistributed.offset, sm.new_est_total.offset,
            C.sizeof(dc), dc.input.offset, dc.n_input.offset, dc.read_len.offset, dc.seqid2taxid.offset, dc.taxid.offset, dc.output.offset, dc.chunk_bytes.offset,
            dc.device.offset,
            C.sizeof(dr), dr.n_windows.offset, dr.n_entries.offset, dr.s_open.offset, dr.s_total.offset,
            C.sizeof(bc), bc.report.offset, bc.read_len.offset, bc.level.offset, bc.threshold.offset, bc.kmer_distrib.offset, bc.output.offset,
            C.sizeof(br), br.n_report_rows.offset, br.n_unknown_taxa.offset, 104]
    assert got == want
    assert e.itemsize == 16 and C.sizeof(st) == 40 and st.ms.offset == 32           # the layouts the issue fixes
    r = K.BRACKEN_ROW_DTYPE
    assert [r.itemsize] + [r.fields[n][1] for n in ("assigned", "new_est", "added", "fraction")] == want[8:13]


def test_exports(K):
    from scrubby_amd import lib
    L = lib.load()
    names = ["sh_k2_distrib_stretch", "sh_k2_distrib_create", "sh_k2_distrib_reset", "sh_k2_distrib_free", "sh_k2_distrib_add_device", "sh_k2_distrib_count",
             "sh_k2_distrib_copy", "sh_k2_distrib_write", "sh_k2_distrib_read", "sh_k2_bracken_estimate", "sh_k2_bracken_write", "sh_k2_distrib_run",
             "sh_k2_bracken_run"]
    for n in names:
        assert n in lib.EXPORTS and hasattr(L, n), n
    s = K.distrib_stretch()
    assert 16 <= s <= 32768
    for f in ("KmerDistrib", "write_kmer_distrib", "read_kmer_distrib", "bracken_estimate", "build_kmer_distrib", "bracken"):
        assert hasattr(K, f), f
    for m in ("add_library", "add_device", "entries", "totals", "reset", "close"):
        assert hasattr(K.KmerDistrib, m), m


def test_write_read_round_trip(K, F, tax, tmp_path):
    nodes, npool, rpool, parent, external, names, ranks = tax
    entries, totals = fixture_maps(F)
    p = tmp_path / "database100mers.kmer_distrib"
    K.write_kmer_distrib(entries_array(K, entries), F["totals"], external, F["read_len"], p)
    text = p.read_text()
    assert text == R.distrib_text(entries, totals, external) == F["distrib_text"]
    ent, tot = K.read_kmer_distrib(p, external)
    want_e, want_t = R.parse_distrib(text, external)
    assert {(int(g), int(m)): int(w) for g, m, w in ent} == want_e == {k: v for k, v in entries.items() if k[1] != 0}
    assert [tuple(x) for x in ent] == sorted((g, m, w) for (g, m), w in want_e.items())          # sorted by (genome, mapped)
    assert {i: int(t) for i, t in enumerate(tot) if t} == want_t == totals                        # the unclassified windows are still in the totals


def test_unknown_taxids_are_named_once_and_skipped(K, F, tax, tmp_path):
    nodes, npool, rpool, parent, external, names, ranks = tax
    p = tmp_path / "d.kmer_distrib"
    p.write_text(R.HEADER + "\n1\t564:10:980 777:5:50 83333:20:1010\n888\t564:1:980\n562\t777:2:50 83333:150:1010\n")
    code = ("import sys; sys.path.insert(0, %r); from scrubby_amd import k2; e, t = k2.read_kmer_distrib(%r, %r); "
            "print([tuple(int(v) for v in x) for x in e], [int(v) for v in t])" % (ROOT, str(p), external))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, check=True)
    assert r.stdout.strip() == str([(7, 1, 10), (9, 1, 20), (9, 6, 150)]) + " " + str([0, 0, 0, 0, 0, 0, 0, 980, 0, 1010])
    assert r.stderr.count("taxid 777 ") == 1 and r.stderr.count("taxid 888 ") == 1


@pytest.mark.parametrize("body,line", [
    ("1\t564:10\n", 2),                                  # two fields
    ("1\t564:10:980\n\n562\t564:1:980\n", 3),            # an empty line
    ("1\t564:10:980  83333:20:1010\n", 2),               # two spaces
    ("1\t564:10:980\nx62\t564:1:980\n", 3),              # not a number
    ("1 564:10:980\n", 2),                               # no tab
    ("1\t564:10:980 \n", 2),                             # a trailing space
    ("1\t564:10:980\n562\t564:1:981\n", 3),              # a second total for one genome
    ("1\t\n", 2),                                        # no entry
])
def test_malformed_lines_are_io_errors_naming_the_line(K, tax, tmp_path, body, line):
    from scrubby_amd import lib as S
    external = tax[4]
    p = tmp_path / "bad.kmer_distrib"
    p.write_text(R.HEADER + "\n" + body)
    with pytest.raises(S.ScrubbyHipError) as ei:
        K.read_kmer_distrib(p, external)
    assert ei.value.status == 7 and f"line {line} " in ei.value.message          # SH_ERR_IO
    p.write_text("mapped\tgenomes\n" + body)
    with pytest.raises(S.ScrubbyHipError) as ei:
        K.read_kmer_distrib(p, external)
    assert ei.value.status == 7 and "line 1 " in ei.value.message


def check_estimate(K, tax, direct, entries, totals, level, threshold, tmp_path):
    nodes, npool, rpool, parent, external, names, ranks = tax
    want = R.estimate(parent, ranks, external, names, direct, entries, totals, level, threshold)
    tot = [totals.get(i, 0) for i in range(len(parent))]
    rows, sm = K.bracken_estimate(nodes, rpool, direct, entries_array(K, entries), tot, level, threshold)
    assert [int(r["taxon"]) for r in rows] == [r[0] for r in want["rows"]]
    assert [(int(r["assigned"]), int(r["new_est"])) for r in rows] == [(r[1], r[3]) for r in want["rows"]]
    # the same operations in the same order: the doubles are equal bit for bit
    assert [struct.pack("<dd", r["added"], r["fraction"]) for r in rows] == [struct.pack("<dd", r[2], r[4]) for r in want["rows"]]
    assert sm["n_rows"] == len(want["rows"])
    for k in ("reads_total", "reads_at_level", "reads_below_threshold", "reads_distributed", "reads_undistributed", "new_est_total"):
        assert sm[k] == want[k], k
    out = tmp_path / f"t_{level}_{threshold}.bracken"
    K.write_bracken(nodes, npool, rows, level, out)
    assert out.read_text() == want["text"]
    return want


def test_estimate_on_the_golden_fixture(K, F, tax, tmp_path):
    entries, totals = fixture_maps(F)
    for c in F["cases"]:
        want = check_estimate(K, tax, F["direct"], entries, totals, c["level"], c["threshold"], tmp_path)
        assert want["text"] == c["text"]                # the recorded table
        assert [[r[0], r[1], r[3]] for r in want["rows"]] == [[r[0], r[1], r[3]] for r in c["rows"]]
        for k in ("reads_total", "reads_at_level", "reads_below_threshold", "reads_distributed", "reads_undistributed", "new_est_total"):
            assert want[k] == c[k], k
    s10 = F["cases"][0]
    assert (s10["level"], s10["threshold"]) == ("S", 10) and len(s10["rows"]) == 2
    assert s10["reads_undistributed"] == F["direct"][2] + F["direct"][5]         # nothing maps to the superkingdom or to the second genus
    assert s10["reads_below_threshold"] == F["direct"][8]                        # the third species
    assert s10["rows"][0][1] == F["direct"][6] + F["direct"][9]                  # the strain's reads are in its species' clade


def test_other_levels_and_empty_inputs(K, F, tax, tmp_path):
    from scrubby_amd import lib as S
    nodes, npool, rpool, parent, external, names, ranks = tax
    entries, totals = fixture_maps(F)
    for level in "DKPCOFGS":
        check_estimate(K, tax, F["direct"], entries, totals, level, 0, tmp_path)
    zero = [0] * len(parent)
    w = check_estimate(K, tax, zero, entries, totals, "S", 10, tmp_path)                     # no reads
    assert w["rows"] == [] and w["text"].count("\n") == 1
    w = check_estimate(K, tax, F["direct"], {}, {}, "S", 10, tmp_path)                      # no distribution: nothing can be distributed
    assert w["reads_distributed"] == 0 and all(r[1] == r[3] for r in w["rows"])
    with pytest.raises(S.ScrubbyHipError) as ei:
        K.bracken_estimate(nodes, rpool, F["direct"], entries_array(K, entries), F["totals"], "X", 10)
    assert ei.value.status == 1
    p = tmp_path / "empty.kmer_distrib"
    K.write_kmer_distrib(np.zeros(0, dtype=K.DISTRIB_DTYPE), zero, external, 100, p)
    assert p.read_text() == R.HEADER + "\n"
    ent, tot = K.read_kmer_distrib(p, external)
    assert len(ent) == 0 and not tot.any()


def save_taxonomy(dbdir, tax):
    """taxo.k2d alone: what sh_k2_bracken_run reads of a database"""
    nodes, npool, rpool = tax[:3]
    os.makedirs(dbdir, exist_ok=True)
    with open(os.path.join(dbdir, "taxo.k2d"), "wb") as f:
        f.write(b"K2TAXDAT" + struct.pack("<QQQ", len(nodes), len(npool), len(rpool)) + bytes(nodes) + npool + rpool)


def test_bracken_run_and_cli_without_a_gpu(K, F, tax, tmp_path):
    nodes, npool, rpool, parent, external, names, ranks = tax
    entries, totals = fixture_maps(F)
    db = tmp_path / "db"
    save_taxonomy(db, tax)
    (db / "database100mers.kmer_distrib").write_text(F["distrib_text"])
    direct = F["direct"]
    rep = [f"  0.31\t{direct[0]}\t{direct[0]}\tU\t0\tunclassified"]
    rep += [f" 10.00\t0\t{direct[i]}\tX\t{external[i]}\t{'  ' * i}{names[i]}" for i in range(1, len(parent)) if direct[i]]
    rep.append("  0.10\t6\t6\tS\t4242\tnot in the database")
    (tmp_path / "kraken.report").write_text("\n".join(rep) + "\n")
    want = R.estimate(parent, ranks, external, names, direct, *R.parse_distrib(F["distrib_text"], external), "S", 10)
    assert want["text"] == F["cases"][0]["text"]
    res = K.bracken(db, tmp_path / "kraken.report", tmp_path / "a.bracken", read_len=100)
    assert (tmp_path / "a.bracken").read_text() == want["text"]
    assert res["n_unknown_taxa"] == 1 and res["reads_undistributed"] == want["reads_undistributed"] + 6 and res["reads_total"] == want["reads_total"] + 6
    assert res["n_report_rows"] == len(rep)
    p = subprocess.run([EXE, "k2-bracken", "-d", str(db), "-r", str(tmp_path / "kraken.report"), "-l", "100", "-o", str(tmp_path / "b.bracken")],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "b.bracken").read_text() == want["text"] and p.stderr.count("taxid 4242 ") == 1
    g = R.estimate(parent, ranks, external, names, direct, entries, totals, "G", 1)
    p = subprocess.run([EXE, "k2-bracken", "-d", str(db), "-r", str(tmp_path / "kraken.report"), "-L", "G", "-t", "1", "-k", str(db / "database100mers.kmer_distrib"),
                        "-o", str(tmp_path / "g.bracken")], capture_output=True, text=True)
    assert p.returncode == 0 and (tmp_path / "g.bracken").read_text() == g["text"]
    for args in (["k2-bracken", "-d", str(db), "-r", str(tmp_path / "kraken.report"), "-l", "100"], ["k2-bracken-build", "-d", str(db), "-l", "100"],
                 ["k2-bracken", "-d", str(db), "-o"]):
        p = subprocess.run([EXE] + args, capture_output=True, text=True)
        assert p.returncode != 0 and ("k2-bracken" in p.stderr or "missing value" in p.stderr)
