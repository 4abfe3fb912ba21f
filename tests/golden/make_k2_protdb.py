#!/usr/bin/env python3
"""A small Kraken 2 PROTEIN database written byte by byte in plain Python, what translated search over it must give, and a
small protein library for the build.

Nothing of the product takes part: the three files are packed with `struct` from the published layouts (see make_k2_pydb.py;
here dna_db = 0, k = 15, l = 12, no spaced seed), and every expected value comes from tests/k2_tx_ref.py, the longhand model of
DESIGN.md §7 "Translated search" (PARITY UNPINNED: the rules are recalled, no Kraken 2 binary has seen these files).

Writes  tests/golden/k2_protdb/{opts,taxo,hash}.k2d, tests/golden/k2_protdb_expected.json
        tests/golden/k2_prot_build/{library.faa, seqid2taxid.map, nodes.dmp, names.dmp}
Tests   tests/test_k2_tx_cpu.py, tests/test_k2_tx_gpu.py

Run: python tests/golden/make_k2_protdb.py
"""
import json
import os
import random
import struct
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import k2_tx_ref as M      # noqa: E402

SEED = 20261019
K, L = M.K_AA, M.L_AA
CAPACITY, VALUE_BITS = 2503, 5
HCAP = 8                    # taxa a unit may count for before the kernel's overflow pass takes it

# name, rank, external id, parent (index; breadth-first, children in ascending external id: the order the build gives them too)
TAXA = [("", "", 0, 0), ("root", "no rank", 1, 0), ("Viruses", "superkingdom", 10239, 1),
        ("Alphavirus", "genus", 100, 2), ("Betavirus", "genus", 200, 2), ("Gammavirus", "genus", 300, 2)]
for g, (gname, gid) in enumerate((("Alphavirus", 100), ("Betavirus", 200), ("Gammavirus", 300))):
    for s in range(4):
        TAXA.append((f"{gname} sp{s + 1}", "species", gid + s + 1, 3 + g))
PARENT = [t[3] for t in TAXA]
SPECIES = list(range(6, 18))
AMINO = "ACDEFGHIKLMNPQRSTVWY"


def rand_protein(rng, n):
    return "".join(rng.choice(AMINO) for _ in range(n))


def back_translate(rng, residues):
    """a codon of the standard code for every residue, picked at random among its codons"""
    out = []
    for r in residues:
        codons = [i for i, a in enumerate(M.CODE_TABLE) if a == r]
        c = rng.choice(codons)
        out.append("ACGT"[c >> 4] + "ACGT"[(c >> 2) & 3] + "ACGT"[c & 3])
    return "".join(out)


def revcomp(s):
    return "".join({"A": "T", "C": "G", "G": "C", "T": "A"}.get(c, "N") for c in reversed(s))


def rand_dna(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def main():
    rng = random.Random(SEED)
    # proteins of 120 residues: [0, 40) shared inside the genus, [40, 80) the species' own, [80, 120) own too, except that the
    # first species of Alphavirus and of Betavirus share it (LCA = Viruses)
    prot = {}
    cross = rand_protein(rng, 40)
    for g in range(3):
        shared = rand_protein(rng, 40)
        for s in range(4):
            t = 6 + 4 * g + s
            tail = cross if (g in (0, 1) and s == 0) else rand_protein(rng, 40)
            prot[t] = shared + rand_protein(rng, 40) + tail
    table = M.Table(CAPACITY, VALUE_BITS, PARENT)
    for t in SPECIES:
        table.add_protein(prot[t], t)
    size = table.size()

    out = os.path.join(HERE, "k2_protdb")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "opts.k2d"), "wb") as f:       # dna_db = 0
        f.write(struct.pack("<QQQQB7xQiii4x", K, L, 0, M.TOGGLE, 0, 0, 1, 0, 0))
    names = b"".join(t[0].encode() + b"\0" for t in TAXA)
    rank_list = []
    for t in TAXA:
        if t[1] not in rank_list:
            rank_list.append(t[1])
    ranks = b"".join(r.encode() + b"\0" for r in rank_list)
    with open(os.path.join(out, "taxo.k2d"), "wb") as f:
        f.write(b"K2TAXDAT" + struct.pack("<QQQ", len(TAXA), len(names), len(ranks)))
        name_off = 0
        for i, t in enumerate(TAXA):
            kids = [j for j in range(2, len(TAXA)) if PARENT[j] == i] if i else []
            rank_off = sum(len(r) + 1 for r in rank_list[:rank_list.index(t[1])])
            f.write(struct.pack("<7Q", PARENT[i], kids[0] if kids else 0, len(kids), name_off, rank_off, t[2], 0))
            name_off += len(t[0]) + 1
        f.write(names + ranks)
    with open(os.path.join(out, "hash.k2d"), "wb") as f:
        f.write(struct.pack("<QQQQ", CAPACITY, size, 32 - VALUE_BITS, VALUE_BITS))
        f.write(struct.pack("<%dI" % CAPACITY, *table.cells))

    a1, a2, a3, b1, b2, c1 = 6, 7, 8, 10, 11, 14
    own = back_translate(rng, prot[a2][40:80])                 # 120 bases, Alphavirus sp2's own stretch
    units = []
    for phase in range(3):
        read = rand_dna(rng, phase) + own
        units.append(([read], f"back-translated read, {phase} base(s) in front"))
        units.append(([revcomp(read)], f"its reverse complement ({phase})"))
    units.append(([own[:57] + "TAA" + own[60:]], "a stop codon inside"))
    units.append(([own[:61] + "N" + own[62:]], "an N inside: the codons over it are X"))
    units.append(([own[:44]], "44 bases: no k-mer in any frame"))
    units.append(([own[:45]], "45 bases: one k-mer in frame 2 and one in its reverse frame"))
    units.append(([own[:47]], "47 bases: one k-mer in every frame"))
    units.append(([back_translate(rng, prot[a3][0:40])], "a stretch shared inside the genus -> Alphavirus"))
    units.append(([back_translate(rng, prot[a3][20:60])], "across the border of shared and own"))
    units.append(([back_translate(rng, prot[a1][82:118])], "shared by two genera -> Viruses"))
    units.append(([rand_dna(rng, 150)], "random: unclassified"))
    units.append(([back_translate(rng, prot[b2][40:80]), revcomp(back_translate(rng, prot[b2][70:110]))], "concordant pair"))
    units.append(([back_translate(rng, prot[b2][40:80]), revcomp(back_translate(rng, prot[c1][40:80]))], "pair whose mates disagree"))
    units.append((["N" * 100, back_translate(rng, prot[c1][45:85])], "pair with one mate all N"))
    pieces = "".join(prot[t][44 + (i % 3):60 + (i % 3)] for i, t in enumerate(SPECIES[:10]))
    big = back_translate(rng, pieces + rand_protein(rng, 40))
    assert len(big) == 600 and M.n_taxa(table, [big]) > HCAP, "the 600-base read must need the overflow pass"
    units.append(([big], "600 bases, 16-residue pieces of ten species: more taxa than the in-LDS list holds"))
    units.append(([big, revcomp(own)], "pair: the 600-base read and a short mate"))

    # a confidence at which S decides: the call with ceil(c * (total + S)) differs from the call with ceil(c * total)
    s_conf = None
    for i in range(1, 1000):
        c = i / 1000.0
        with_s = M.classify(table, [own], c, 1)
        saved = M.S_READ
        M.S_READ = 0
        without = M.classify(table, [own], c, 1)
        M.S_READ = saved
        if with_s[0] != without[0]:
            s_conf = (c, with_s[0], without[0])
            break
    assert s_conf, "no confidence separates S = 3 from S = 0 on this read"

    exp = {"k": K, "l": L, "capacity": CAPACITY, "value_bits": VALUE_BITS, "size": size, "toggle": str(M.TOGGLE), "seed": SEED,
           "parents": PARENT, "external": [t[2] for t in TAXA], "names": [t[0] for t in TAXA], "ranks": [t[1] for t in TAXA],
           "proteins": {str(t): prot[t] for t in SPECIES},
           "s_decides": {"mates": [own], "confidence": s_conf[0], "min_hit_groups": 1, "call": s_conf[1], "call_without_s": s_conf[2]},
           "units": []}
    thresholds = [(c, g) for c in (0.0, 0.5, 1.0) for g in (1, 2, 3)]
    for mates, what in units:
        res = []
        for conf, mhg in thresholds:
            call, total, groups = M.classify(table, mates, conf, mhg)
            res.append({"confidence": conf, "min_hit_groups": mhg, "call": call, "taxid": TAXA[call][2], "total_kmers": total, "hit_groups": groups})
        exp["units"].append({"mates": mates, "what": what, "n_taxa": M.n_taxa(table, mates), "results": res})
    with open(os.path.join(HERE, "k2_protdb_expected.json"), "w") as f:
        json.dump(exp, f, indent=0)
        f.write("\n")

    # ---- the build fixture: the same taxonomy NCBI-style, the twelve proteins as an amino-acid FASTA library with U, O, X, *
    # and lower case in it, and a thirteenth record that is skipped
    bd = os.path.join(HERE, "k2_prot_build")
    os.makedirs(bd, exist_ok=True)
    with open(os.path.join(bd, "nodes.dmp"), "w") as f:
        for i in range(1, len(TAXA)):
            t = TAXA[i]
            f.write(f"{t[2]}\t|\t{TAXA[PARENT[i]][2] if i > 1 else 1}\t|\t{t[1]}\t|\t\t|\t0\t|\t0\t|\t11\t|\t0\t|\t0\t|\t0\t|\t0\t|\t0\t|\t\t|\n")
    with open(os.path.join(bd, "names.dmp"), "w") as f:
        for i in range(1, len(TAXA)):
            f.write(f"{TAXA[i][2]}\t|\t{TAXA[i][0]}\t|\t\t|\tscientific name\t|\n")
    lib = []
    for n, t in enumerate(SPECIES):
        p = prot[t]
        if n == 1:
            p = p[:50] + "U" + p[51:]                       # selenocysteine: code 0, like '*'
        if n == 2:
            p = p[:60] + "O" + p[61:]                       # pyrrolysine: code 0
        if n == 3:
            p = p[:55] + "X" + p[56:]                       # ambiguous: restarts the l-mer
        if n == 4:
            p = p[:70] + "*" + p[71:]                       # a stop inside
        if n == 5:
            p = p[:30] + p[30:90].lower() + p[90:]          # lower case
        lib.append((f"prot{n + 1}", TAXA[t][2], p))
    with open(os.path.join(bd, "seqid2taxid.map"), "w") as f:
        for sid, taxid, _ in lib[:10]:
            f.write(f"{sid}\t{taxid}\n")
    with open(os.path.join(bd, "library.faa"), "w") as f:
        for n, (sid, taxid, p) in enumerate(lib):
            f.write(f">{sid if n < 10 else f'kraken:taxid|{taxid}|{sid}'} protein {n + 1}\n")
            width = 60 if n % 2 == 0 else 47
            for q in range(0, len(p), width):
                f.write(p[q:q + width] + "\n")
        f.write(">orphan not in the map\n" + rand_protein(rng, 80) + "\n")
    print("cells used", size, "of", CAPACITY, "| S decides at confidence", s_conf)
    print("calls at (0, 2):", [TAXA[u["results"][1]["call"]][0] or "-" for u in exp["units"]])


if __name__ == "__main__":
    main()
