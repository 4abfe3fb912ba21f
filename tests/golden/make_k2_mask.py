"""Generator of tests/golden/k2_mask/: a small FASTA library that mixes ordinary and low-complexity sequence, and the masked
intervals the brute force (tests/k2_mask_ref.py) finds in it for each (window, threshold) the tests use.

    python tests/golden/make_k2_mask.py

Families (seed 20261016): uniformly random ACGT, homopolymers, tandem repeats of 2..7-mers with a few percent of substitutions,
two-letter stretches, runs of N, lower-case stretches, and records of 0..3 bases."""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import k2_mask_ref as R  # noqa: E402

PARAMS = [(64, 20), (32, 20), (64, 30), (16, 12)]
SEED = 20261016


def rand_seq(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def tandem(rng, unit_len, n, sub_pct):
    unit = rand_seq(rng, unit_len)
    s = list((unit * (n // unit_len + 1))[:n])
    for i in range(n):
        if rng.random() * 100 < sub_pct:
            s[i] = rng.choice("ACGT")
    return "".join(s)


def family_piece(rng):
    """one stretch of a random family"""
    f = rng.randrange(8)
    if f == 0:
        return rand_seq(rng, rng.randrange(30, 400))
    if f == 1:
        return rng.choice("ACGT") * rng.randrange(4, 90)
    if f == 2:
        return tandem(rng, rng.randrange(2, 8), rng.randrange(10, 300), rng.choice([0, 2, 4, 6]))
    if f == 3:
        return rand_seq(rng, rng.randrange(10, 200), alphabet=rng.sample("ACGT", 2))
    if f == 4:
        return "N" * rng.randrange(1, 70)
    if f == 5:
        return tandem(rng, rng.randrange(2, 8), rng.randrange(10, 200), 3).lower()
    if f == 6:
        return rand_seq(rng, rng.randrange(1, 12))          # short runs between other things
    return rng.choice("ACGT") * rng.randrange(5, 9) + rng.choice("NRYn-") + rand_seq(rng, rng.randrange(0, 6))


def make_records(rng, n_records, pieces):
    recs = []
    for i in range(n_records):
        recs.append("".join(family_piece(rng) for _ in range(rng.randrange(*pieces))))
    return recs


def library():
    rng = random.Random(SEED)
    recs = make_records(rng, 24, (8, 24))
    recs += ["", "A", "AC", "ACG", "ACGT"]                          # records of 0..4 bases
    recs += [rand_seq(rng, 4097), rand_seq(rng, 300) + "A" * 40]      # one default tile plus one base; a stretch at a record's end
    recs += ["T" * 40 + rand_seq(rng, 200)]                            # ... and at the start of the next one
    return [(f"m{i} family mix {i}", s) for i, s in enumerate(recs)]


def main():
    out = os.path.join(HERE, "k2_mask")
    os.makedirs(out, exist_ok=True)
    recs = library()
    with open(os.path.join(out, "library.fa"), "w") as f:
        for h, s in recs:
            f.write(f">{h}\n")
            for p in range(0, len(s), 70):
                f.write(s[p: p + 70] + "\n")
    exp = {"seed": SEED, "n_bases": sum(len(s) for _, s in recs), "records": [{"header": h, "length": len(s)} for h, s in recs], "masked": {}}
    for W, T in PARAMS:
        iv = [R.intervals(R.mask_flags(s.encode(), W, T)) for _, s in recs]
        n = sum(b - a for r in iv for a, b in r)
        exp["masked"][f"{W},{T}"] = {"n_masked": n, "intervals": iv}
        print(f"W={W} T={T}: {n} of {exp['n_bases']} bases masked ({100.0 * n / exp['n_bases']:.1f} %)")
    with open(os.path.join(out, "expected.json"), "w") as f:
        json.dump(exp, f, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()
