#!/usr/bin/env python3
"""Writes tests/golden/k2_build/: a small NCBI-style taxonomy, an id map, a FASTA library and expected.json for the database
build (tests/test_k2_build_cpu.py, tests/test_k2_build_gpu.py).  Plain Python, nothing from the product or the oracle: the
expected taxonomy comes from this file's own breadth-first walk, the expected taxon of a header from its own parsing.

    python tests/golden/make_k2_build.py        # rewrites the directory; SEED below is the fixture's seed

SEED = 20261016 was the first seed tried; tests/test_k2_build_gpu.py asserts (on the CPU, before any GPU work) that with it no two
distinct minimizers of the library that share a truncated key fall into one occupied run of the table it builds."""
import json
import os
import random

SEED = 20261016
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "k2_build")

# (taxid, parent, rank, scientific name), in the order the rows are written: siblings are NOT in ascending taxid order
NODES = [
    (1, 1, "no rank", "root"),
    (10239, 1, "superkingdom", "Viruses"),                # not used by the map: dropped, with its child
    (131567, 1, "no rank", "cellular organisms"),
    (2759, 131567, "superkingdom", "Eukaryota"),          # written before its smaller sibling 2
    (2, 131567, "superkingdom", "Bacteria"),
    (9606, 2759, "species", "Homo sapiens"),
    (1239, 2, "phylum", "Bacillota"),                     # written before its smaller sibling 1224
    (1224, 2, "phylum", "Pseudomonadota"),
    (543, 1224, "family", "Enterobacteriaceae"),
    (590, 543, "genus", "Salmonella"),                    # written before its smaller sibling 561
    (561, 543, "genus", "Escherichia"),
    (28901, 590, "species", "Salmonella enterica"),
    (564, 561, "species", "Escherichia fergusonii"),      # not used: dropped
    (562, 561, "species", "Escherichia coli"),
    (1386, 1239, "genus", "Bacillus"),
    (1423, 1386, "species", "Bacillus subtilis"),
    (10710, 10239, "species", "Lambdavirus lambda"),      # not used: dropped
]
OTHER_NAMES = [(562, "E. coli", "common name"), (562, "Bacterium coli", "synonym"), (9606, "human", "genbank common name"),
               (1, "all", "synonym"), (2, "eubacteria", "genbank common name")]
# sequence id -> taxid; 99999 is not in nodes.dmp (reported once, its sequences skipped)
MAP = [("seqA", 562), ("seqB", 28901), ("seqC", 1423), ("seqD", 9606), ("seqE", 562), ("seqF", 99999), ("multi1", 562), ("multi2", 28901)]
MISSING = [99999]
DROPPED = [10239, 10710, 564]


def rand_seq(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def main():
    rng = random.Random(SEED)
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "nodes.dmp"), "w") as f:
        for t, p, r, _ in NODES:
            f.write(f"{t}\t|\t{p}\t|\t{r}\t|\t\t|\t0\t|\t0\t|\t11\t|\t0\t|\t0\t|\t0\t|\t0\t|\t0\t|\t\t|\n")
    with open(os.path.join(OUT, "names.dmp"), "w") as f:
        rows = [(t, n, "scientific name") for t, _, _, n in NODES] + OTHER_NAMES
        rows.sort(key=lambda x: (x[0], x[2] == "scientific name"))        # the scientific name is not the first row of its taxon
        for t, n, c in rows:
            f.write(f"{t}\t|\t{n}\t|\t\t|\t{c}\t|\n")
    with open(os.path.join(OUT, "seqid2taxid.map"), "w") as f:
        for i, (s, t) in enumerate(MAP):
            f.write(f"{s}{' ' if i % 3 == 2 else chr(9)}{t}\n")            # tab- or space-separated

    # the library: two species share a 600-base stretch, so minimizers with an LCA above the species really occur
    shared = rand_seq(rng, 600)
    a = rand_seq(rng, 4000) + shared + rand_seq(rng, 4400)
    a = a[:1500] + a[1500:1900].lower() + a[1900:]                        # a lower-case stretch (still ACGT)
    b = rand_seq(rng, 2500) + shared + rand_seq(rng, 4900)
    c = rand_seq(rng, 3000) + "N" * 50 + rand_seq(rng, 3950)              # an N run
    c = c[:5000] + "R" + c[5001:]                                         # and one IUPAC code
    records = [
        ("seqA Escherichia coli, with a lower-case stretch", a, 562),
        ("seqB Salmonella enterica, shares 600 bases with seqA", b, 28901),
        ("seqC Bacillus subtilis, with an N run", c, 1423),
        ("seqD Homo sapiens", rand_seq(rng, 6000), 9606),
        ("seqE shorter than k", rand_seq(rng, 20), 562),
        ("seqF its taxid is not in nodes.dmp", rand_seq(rng, 1000), 0),
        ("orphan1 not in the map", rand_seq(rng, 1000), 0),
        ("kraken:taxid|1423|seqK no map entry needed", rand_seq(rng, 3000), 1423),
        ("multi1 first of two ids\x01multi2 second id", rand_seq(rng, 3000), 543),      # LCA(562, 28901), checked below
    ]
    with open(os.path.join(OUT, "library.fna"), "w") as f:
        for i, (h, s, _) in enumerate(records):
            f.write(">" + h + "\n")
            width = 70 if i % 2 == 0 else 61
            for p in range(0, len(s), width):
                f.write(s[p: p + width] + "\n")

    # expected taxonomy: this file's own walk
    parent = {t: p for t, p, _, _ in NODES}
    rank = {t: r for t, _, r, _ in NODES}
    name = {t: n for t, _, _, n in NODES}
    used = {t for _, t in MAP if t in parent} | {1423}                    # 1423 also through the kraken:taxid header
    keep = {1}
    for t in used:
        while t not in keep:
            keep.add(t)
            t = parent[t]
    kids = {}
    for t in keep:
        if t != 1:
            kids.setdefault(parent[t], []).append(t)
    order = [None, 1]
    nodes = [dict(external=0, parent=0, first_child=0, child_count=0, name="", rank=""), None]
    internal = {1: 1}
    i = 1
    while i < len(order):
        t = order[i]
        ch = sorted(kids.get(t, []))
        nodes[i] = dict(external=t, parent=internal[parent[t]] if t != 1 else 0, first_child=len(order) if ch else 0, child_count=len(ch), name=name[t], rank=rank[t])
        for k in ch:
            internal[k] = len(order)
            order.append(k)
            nodes.append(None)
        i += 1
    assert sorted(keep) == sorted(internal) and not (set(DROPPED) & keep)
    value_bits = 1
    while (1 << value_bits) < len(nodes):
        value_bits += 1

    def lca(x, y):
        anc = set()
        while True:
            anc.add(x)
            if x == 1:
                break
            x = parent[x]
        while y not in anc:
            y = parent[y]
        return y
    assert lca(562, 28901) == 543
    expected = dict(seed=SEED, n_nodes=len(nodes), value_bits=value_bits, nodes=nodes, dropped=DROPPED, missing=MISSING,
                    n_map_entries=sum(1 for _, t in MAP if t in parent),
                    records=[dict(header=h, length=len(s), taxid=t, internal=internal.get(t, 0)) for h, s, t in records])
    with open(os.path.join(OUT, "expected.json"), "w") as f:
        json.dump(expected, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
