"""Writes tests/golden/k2_bracken/fixture.json: a small taxonomy, one sample's direct reads, a k-mer distribution, and what
tests/k2_bracken_ref.py (the model written from the definitions) makes of them: the kmer_distrib file and the Bracken tables.

The taxonomy has two species under one genus, a strain below one of them, and a third species (under a second genus) whose
clade stays below the threshold.  Reads sit at the root, the superkingdom, the family, both genera, the species and the strain.
Nothing maps to the superkingdom or to the second genus, so their reads are undistributed at level S.

A condition on the fixture, asserted here: no clade + added lies within 1e-6 of a half, so the rounding rule never hangs on
floating-point luck.

    python tests/golden/make_k2_bracken.py
"""
import json
import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import k2_bracken_ref as R  # noqa: E402

NODES = [   # (parent, external taxid, name, rank); ids breadth-first, children consecutive
    (0, 0, "", ""),
    (0, 1, "root", "no rank"),
    (1, 2, "Bacteria", "superkingdom"),
    (2, 543, "Enterobacteriaceae", "family"),
    (3, 561, "Escherichia", "genus"),
    (3, 590, "Salmonella", "genus"),
    (4, 562, "Escherichia coli", "species"),
    (4, 564, "Escherichia fergusonii", "species"),
    (5, 28901, "Salmonella enterica", "species"),
    (6, 83333, "Escherichia coli K-12", "strain"),
]
DIRECT = [3, 37, 5, 23, 111, 13, 400, 300, 4, 57]       # [0]: unclassified reads
ENTRIES = [     # (genome, mapped, windows); mapped 0 = unclassified windows
    (9, 0, 10), (9, 1, 20), (9, 3, 30), (9, 4, 100), (9, 6, 150), (9, 9, 700),
    (7, 1, 10), (7, 3, 50), (7, 4, 120), (7, 7, 800),
    (8, 0, 20), (8, 3, 40), (8, 8, 500),
]
CASES = [("S", 10), ("G", 1), ("S", 1), ("F", 10), ("K", 10)]
READ_LEN = 100


def main():
    parent = [n[0] for n in NODES]
    external = [n[1] for n in NODES]
    names = [n[2] for n in NODES]
    ranks = [n[3] for n in NODES]
    entries = {(g, m): w for g, m, w in ENTRIES}
    totals = {}
    for g, _, w in ENTRIES:
        totals[g] = totals.get(g, 0) + w
    cases = []
    for level, threshold in CASES:
        e = R.estimate(parent, ranks, external, names, DIRECT, entries, totals, level, threshold)
        for s, assigned, added, new_est, _ in e["rows"]:
            frac = (assigned + added) - math.floor(assigned + added)
            assert abs(frac - 0.5) > 1e-6, (level, threshold, s, assigned + added)
        cases.append({"level": level, "threshold": threshold, "rows": [[s, a, ad, ne, f] for s, a, ad, ne, f in e["rows"]],
                      **{k: e[k] for k in ("reads_total", "reads_at_level", "reads_below_threshold", "reads_distributed", "reads_undistributed", "new_est_total", "text")}})
    s10 = cases[0]
    assert s10["reads_undistributed"] == DIRECT[2] + DIRECT[5] and s10["reads_below_threshold"] == DIRECT[8] and len(s10["rows"]) == 2
    out = {"nodes": [{"parent": p, "external": x, "name": nm, "rank": rk} for p, x, nm, rk in NODES], "direct": DIRECT,
           "entries": [list(e) for e in ENTRIES], "totals": [totals.get(i, 0) for i in range(len(NODES))], "read_len": READ_LEN,
           "distrib_text": R.distrib_text(entries, totals, external), "cases": cases}
    os.makedirs(os.path.join(HERE, "k2_bracken"), exist_ok=True)
    with open(os.path.join(HERE, "k2_bracken", "fixture.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
