"""Translated search without a GPU: the model (tests/k2_tx_ref.py) against hand answers, sh_k2_translate_host against the model,
the layouts of the two renamed struct fields against the C header, the exported symbols, and the committed fixtures against
their generator's rules."""
import ctypes as C
import json
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import k2_tx_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")

HAND_DNA = "ATGGCCATTGTAATGGGCCGCTGAAAGGGTGCCCGATAG"
HAND_AA = "MAIVMGR*KGAR*"

# the standard genetic code, written out codon by codon (NCBI translation table 1), independent of the model's packed string
STANDARD = {
    "TTT": "F", "TTC": "F", "TTA": "L", "TTG": "L", "CTT": "L", "CTC": "L", "CTA": "L", "CTG": "L",
    "ATT": "I", "ATC": "I", "ATA": "I", "ATG": "M", "GTT": "V", "GTC": "V", "GTA": "V", "GTG": "V",
    "TCT": "S", "TCC": "S", "TCA": "S", "TCG": "S", "CCT": "P", "CCC": "P", "CCA": "P", "CCG": "P",
    "ACT": "T", "ACC": "T", "ACA": "T", "ACG": "T", "GCT": "A", "GCC": "A", "GCA": "A", "GCG": "A",
    "TAT": "Y", "TAC": "Y", "TAA": "*", "TAG": "*", "CAT": "H", "CAC": "H", "CAA": "Q", "CAG": "Q",
    "AAT": "N", "AAC": "N", "AAA": "K", "AAG": "K", "GAT": "D", "GAC": "D", "GAA": "E", "GAG": "E",
    "TGT": "C", "TGC": "C", "TGA": "*", "TGG": "W", "CGT": "R", "CGC": "R", "CGA": "R", "CGG": "R",
    "AGT": "S", "AGC": "S", "AGA": "R", "AGG": "R", "GGT": "G", "GGC": "G", "GGA": "G", "GGG": "G",
}


def revcomp(s):
    return "".join({"A": "T", "C": "G", "G": "C", "T": "A", "a": "t", "c": "g", "g": "c", "t": "a"}.get(c, "N") for c in reversed(s))


# ---- the model against hand answers -----------------------------------------------------------------------------------------
def test_model_hand_translation():
    fr = M.translate(HAND_DNA)
    assert fr[2] == HAND_AA                           # the codons that start at base 0 land in frame 2
    assert [len(f) for f in fr] == [12, 12, 13, 12, 12, 13]
    rc = M.translate(revcomp(HAND_DNA))
    assert HAND_AA in rc[3:] and rc[5] == HAND_AA     # the reverse complement gives the same string in a reverse frame
    assert M.translate("AC") == [""] * 6 and M.translate("") == [""] * 6
    assert M.translate("ATG") == ["", "", "M", "", "", "H"]          # CAT


def test_model_code_table_codon_by_codon():
    assert len(STANDARD) == 64
    for codon, aa in STANDARD.items():
        assert M.translate(codon)[2] == aa, codon
        assert M.translate(codon.lower())[2] == aa
        assert M.translate(revcomp(codon))[5] == aa
    for bad in ("ANG", "NTG", "ATN", "AT-", "ATU", "ATR"):
        assert M.translate(bad)[2] == "X" and M.translate(bad)[5] == "X"


def test_model_alphabet_and_scanner():
    table = {"*": 0, "U": 0, "O": 0, "A": 1, "N": 2, "Q": 2, "S": 2, "C": 3, "D": 4, "E": 4, "F": 5, "G": 6, "H": 7, "I": 8, "L": 8, "K": 9,
             "P": 10, "R": 11, "M": 12, "V": 12, "T": 13, "W": 14, "Y": 15}
    for b in range(256):
        ch = chr(b)
        assert M.aa_code(ch) == table.get(ch.upper() if ch.isascii() and ch.isalpha() else ch), b
    assert M.aa_code("X") is None and M.aa_code("B") is None and M.aa_code("Z") is None and M.aa_code("J") is None
    # one k-mer of 15 residues: the minimum of its four 12-mers under the toggle mask
    s = "ACDEFGHIKLMNPQR"
    cands = []
    for i in range(4):
        v = 0
        for ch in s[i:i + 12]:
            v = v * 16 + table[ch]
        cands.append(v ^ M.TOGGLE)
    assert M.scan_aa(s) == [min(cands) ^ M.TOGGLE]
    assert M.scan_aa(s[:14]) == []
    # an X restarts the l-mer: the k-mers that have no whole 12-mer behind it are ambiguous, the first one that has one is not
    t = "ACDEFGHIKLMNPQRSTVWYACDEFGHIK"
    r = M.scan_aa(t[:16] + "X" + t[17:])
    assert len(r) == len(t) - 14 and r[0] is not None and r[1] is not None
    assert all(x is None for x in r[2:14]) and r[14] is not None
    # synonyms of the reduced alphabet give the same minimizers, either case
    assert M.scan_aa("ILMVNQSDE" * 3) == M.scan_aa("LIVMSNQED" * 3) == M.scan_aa(("ilmvnqsde" * 3))


def test_model_table_and_classify_s():
    parent = [0, 0, 1, 2, 2]
    t = M.Table(101, 3, parent)
    t.set(12345, 3)
    t.set(12345, 4)
    assert t.get(12345) == 2 and t.get(54321) == 0 and t.size() == 1           # LCA on a key already there
    prot = "ACDEFGHIKLMNPQRSTVWYACDEFGHIKLMNPQRSTVWY"
    t2 = M.Table(1009, 3, parent)
    t2.add_protein(prot, 3)
    dna = "".join({v: k for k, v in STANDARD.items()}[a] for a in prot)
    call, total, groups = M.classify(t2, [dna], 0.0, 1)
    assert call == 3 and total == 2 * (26 + 25 + 25) and groups >= 1
    # every k-mer of frame 2 counts for taxon 3: 26 of 152; S = 3 moves the threshold from ceil(c * 152) to ceil(c * 155)
    assert M.classify(t2, [dna], 25.9 / 155.0, 1)[0] == 3 and M.classify(t2, [dna], 26.5 / 155.0, 1)[0] == 0
    assert 26.5 / 155.0 * 152 <= 26                    # without S that confidence would still classify
    # a pair pools both mates and uses S = 6
    assert M.classify(t2, [dna, revcomp(dna)], 51.9 / 310.0, 1) == (3, 304, M.classify(t2, [dna, revcomp(dna)], 0, 1)[2])
    assert M.classify(t2, [dna, revcomp(dna)], 52.5 / 310.0, 1)[0] == 0


# ---- sh_k2_translate_host against the model ----------------------------------------------------------------------------------
def _records():
    rng = np.random.default_rng(20261019)
    recs = []
    for n in list(range(10)) + [44, 45, 46, 47, 150, 151, 152]:
        recs.append("".join("ACGT"[i] for i in rng.integers(0, 4, n)))
    base = recs[-3]
    recs.append("N" + base[1:])                            # an N at the first base
    recs.append(base[:-1] + "N")                           # at the last base
    for phase in range(3):
        recs.append(base[:60 + phase] + "N" + base[61 + phase:])       # at each codon phase
    recs.append(base.lower())
    recs.append(base[:50] + base[50:100].lower() + base[100:])
    return recs


def check_translation(got, off, recs, quals=None, min_qual=0, as_letters=False):
    exp, defined = M.frames_layout(recs, quals, min_qual, as_letters)
    assert len(got) == len(exp)
    d = np.frombuffer(bytes(defined), dtype=np.uint8).astype(bool)
    g, e = np.asarray(got), np.frombuffer(bytes(exp), dtype=np.uint8)
    bad = np.nonzero(d & (g != e))[0]
    assert len(bad) == 0, f"{len(bad)} bytes differ, first at {bad[:5]}"
    assert [int(x) for x in off] == [0] + list(np.cumsum([len(r) for r in recs]))


@pytest.mark.parametrize("as_letters", [False, True])
def test_translate_host_matches_the_model(as_letters):
    from scrubby_amd import k2
    recs = _records()
    out, off = k2.translate_host([r.encode() for r in recs], as_letters=as_letters)
    check_translation(out, off, recs, as_letters=as_letters)
    # the bytes between records are not written
    _, defined = M.frames_layout(recs)
    assert not out[~np.frombuffer(bytes(defined), dtype=np.uint8).astype(bool)].any()
    if as_letters:
        n0 = sum(len(r) for r in recs[:14])          # the 150-base record's frames
        assert bytes(out[2 * n0: 2 * n0 + 49]).decode() == M.translate(recs[14])[0]


def test_translate_host_quality_threshold_masks_one_base():
    from scrubby_amd import k2
    recs = _records()[14:17]
    quals = [bytes([ord("I")] * len(r)) for r in recs]
    q1 = bytearray(quals[1]); q1[70] = ord("!") + 9; quals[1] = bytes(q1)       # Phred 9 < 10
    q2 = bytearray(quals[2]); q2[5] = 0xff; quals[2] = bytes(q2)                # 0xFF is never masked
    for as_letters in (False, True):
        out, off = k2.translate_host([r.encode() for r in recs], quals=quals, min_qual=10, as_letters=as_letters)
        check_translation(out, off, recs, quals, 10, as_letters)
    assert "X" in M.translate(recs[1], quals[1], 10)[(70 % 3)] and "X" not in M.translate(recs[2], quals[2], 10)[2]
    # threshold 0: the qualities are not looked at
    out, off = k2.translate_host([r.encode() for r in recs], quals=quals, min_qual=0)
    check_translation(out, off, recs)


def test_hand_translation_through_the_library():
    from scrubby_amd import k2
    out, _ = k2.translate_host([HAND_DNA.encode()], as_letters=True)
    assert bytes(out[12 + 12: 12 + 12 + 13]).decode() == HAND_AA


# ---- layouts, symbols, defaults ------------------------------------------------------------------------------------------------
PROG = r"""
#include <stdio.h>
#include <stddef.h>
#include "scrubby_hip.h"
int main(void)
{
    printf("%zu %zu %zu %zu %zu %zu\n", sizeof(sh_k2_opts), offsetof(sh_k2_opts, protein), sizeof(sh_k2_stats), offsetof(sh_k2_stats, ms_translate),
           sizeof(sh_k2_build_config), offsetof(sh_k2_build_config, protein));
    return 0;
}
"""


def test_ctypes_layouts_match_the_header(tmp_path):
    from scrubby_amd import k2
    src, exe = tmp_path / "abi.c", tmp_path / "abi"
    src.write_text(PROG)
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    O, S, B = k2.K2Opts, k2.K2Stats, k2.K2BuildConfig
    assert got == [C.sizeof(O), O.protein.offset, C.sizeof(S), S.ms_translate.offset, C.sizeof(B), B.protein.offset]
    assert O.protein.offset == 60 and C.sizeof(O) == 64               # the field took the padding's place
    assert S.ms_translate.offset == 68 and C.sizeof(S) == 72
    assert "ms_translate" in k2._stats_dict(S())


def test_exported_symbols_and_defaults():
    from scrubby_amd import k2, lib
    L = lib.load()
    for name in ("sh_k2_default_protein_opts", "sh_k2_translate_device", "sh_k2_translate_host"):
        assert name in lib.EXPORTS and hasattr(L, name)
    d, p = k2.default_opts(), k2.default_protein_opts()
    assert (d.k, d.l, d.protein) == (35, 31, 0) and d.spaced_seed_mask != 0           # unchanged
    assert (p.k, p.l, p.spaced_seed_mask, p.protein) == (15, 12, 0, 1) and p.toggle_mask == d.toggle_mask == M.TOGGLE
    assert (p.min_hit_groups, p.confidence, p.value_bits) == (d.min_hit_groups, d.confidence, d.value_bits)


# ---- the committed fixtures ----------------------------------------------------------------------------------------------------
def test_committed_protein_database_is_what_the_model_says():
    exp = json.load(open(os.path.join(GOLD, "k2_protdb_expected.json")))
    raw = open(os.path.join(GOLD, "k2_protdb", "opts.k2d"), "rb").read()
    k, l, spaced, toggle, dna_db = struct.unpack_from("<QQQQB", raw)
    assert len(raw) == 64 and (k, l, spaced, toggle, dna_db) == (15, 12, 0, M.TOGGLE, 0)
    h = open(os.path.join(GOLD, "k2_protdb", "hash.k2d"), "rb").read()
    cap, size, kb, vb = struct.unpack_from("<QQQQ", h)
    assert (cap, size, kb + vb, vb) == (exp["capacity"], exp["size"], 32, exp["value_bits"]) and len(h) == 32 + 4 * cap < 16384
    t = M.Table(cap, vb, exp["parents"])
    t.cells = list(struct.unpack_from("<%dI" % cap, h, 32))
    species = [i for i, r in enumerate(exp["ranks"]) if r == "species"]
    genera = [i for i, r in enumerate(exp["ranks"]) if r == "genus"]
    assert len(species) >= 12 and len(genera) == 3 and all(len(exp["proteins"][str(s)]) == 120 for s in species)
    # every minimizer of a protein is in the table under the species or an ancestor of it
    for s in species:
        for m in M.scan_aa(exp["proteins"][str(s)]):
            assert t.is_ancestor(t.get(m), s)
    # the expected answers are the model's, the overflow unit needs more taxa than the in-LDS list holds, and S decides one call
    for u in exp["units"]:
        for r in u["results"]:
            assert M.classify(t, u["mates"], r["confidence"], r["min_hit_groups"]) == (r["call"], r["total_kmers"], r["hit_groups"])
    assert max(u["n_taxa"] for u in exp["units"]) > 8
    by_what = {u["what"][:8]: u for u in exp["units"]}
    assert by_what["44 bases"]["results"][0]["total_kmers"] == 0 and by_what["45 bases"]["results"][0]["total_kmers"] == 2
    assert by_what["47 bases"]["results"][0]["total_kmers"] == 6
    sd = exp["s_decides"]
    assert M.classify(t, sd["mates"], sd["confidence"], sd["min_hit_groups"])[0] == sd["call"] != sd["call_without_s"]
