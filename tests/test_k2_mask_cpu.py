"""Low-complexity masking, CPU side: the brute force of the rule (tests/k2_mask_ref.py) against known answers worked out by hand,
sanity bounds on the rule itself, and sh_k2_mask_host (the streaming mirror in the library) against the brute force, byte for byte.

Known answers, from the rule (score r / l of an interval of triplets, masked when 10 r > 20 l, i.e. score > 2):
* a homopolymer of n bases has m = n - 2 equal triplets: r = m (m - 1) / 2, l = m - 1, score m / 2 > 2 from m = 5: A x 6 unmasked,
  A x 7 masked whole.
* (AC) x h: 2h - 2 triplets, h - 1 ACA and h - 1 CAC: r = (h - 1)(h - 2), l = 2h - 3; h = 5: 12 / 7 < 2, h = 6: 20 / 9 > 2.
* (ACG) x n has period 3 in its triplets (ACG, CGA, GAC).  A stretch of b bases has b - 2 triplets spread as evenly as can be over
  the three codes.  b = 16: counts 5, 5, 4: r = 10 + 10 + 6 = 26, l = 13: exactly 2, not above it.  b = 17: counts 5, 5, 5: r = 30,
  l = 14: 15 / 7 > 2.  Shorter stretches score less, so 17 bases is the shortest masked length, and those 17 are masked whole
  (every interval inside scores at most what the whole does).
"""
import json
import os
import random
import sys

import numpy as np
import pytest

from tests import k2_mask_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "k2_mask")
sys.path.insert(0, os.path.dirname(GOLD))
import make_k2_mask as G  # noqa: E402  (the fixture's generator: its families make the seeded inputs too)

PARAMS = [(64, 20), (32, 20), (64, 30), (16, 12)]


@pytest.fixture(scope="module")
def K():
    from scrubby_amd import k2
    return k2


def read_fixture():
    recs, h, parts = [], None, []
    with open(os.path.join(GOLD, "library.fa"), "rb") as f:
        for ln in f:
            ln = ln.rstrip(b"\n")
            if ln.startswith(b">"):
                if h is not None:
                    recs.append((h, b"".join(parts)))
                h, parts = ln[1:].decode(), []
            else:
                parts.append(ln)
    recs.append((h, b"".join(parts)))
    return recs


@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(GOLD, "expected.json")) as f:
        E = json.load(f)
    recs = read_fixture()
    assert [h for h, _ in recs] == [r["header"] for r in E["records"]] and [len(s) for _, s in recs] == [r["length"] for r in E["records"]]
    return [s for _, s in recs], E


def seeded_records(seed):
    """the fixture's families under another seed, plus short records"""
    rng = random.Random(seed)
    return [s.encode() for s in G.make_records(rng, 4, (3, 14))] + [b"", b"AC", b"ACGTTTTTTTTTT"]


def flags_of(masked, original):
    return bytearray(int(a != b) for a, b in zip(masked, original))


# ---- the brute force itself ---------------------------------------------------------------------------------------------------
KNOWN = [
    (b"G" + b"A" * 6 + b"C", None),                            # A x 6 between other bases
    (b"A" * 7, [[0, 7]]),
    (b"G" + b"A" * 7 + b"C", [[1, 8]]),
    (b"AC" * 5, None),
    (b"AC" * 6, [[0, 12]]),
    ((b"ACG" * 6)[:16], None),
    ((b"ACG" * 6)[:17], [[0, 17]]),
    (b"GATTACA" + b"N" + b"T" * 9 + b"N" + b"CATGCAT", [[8, 17]]),          # a masked stretch between two N
    (b"a" * 7, [[0, 7]]), (b"cagtg" + b"acacacacacac" + b"gtcag", [[5, 17]]),   # lower case is ACGT
    (b"", None), (b"A", None), (b"AA", None), (b"AAA", None),
]


@pytest.mark.parametrize("seq,want", KNOWN)
def test_known_answers_brute_force(seq, want):
    got = R.intervals(R.mask_flags(seq))
    assert got == (want or [])
    assert R.mask_flags(seq) == R.by_enumeration(seq)


def test_brute_force_recurrence_equals_plain_enumeration():
    rng = random.Random(3)
    for it in range(80):
        s = "".join(rng.choice("AC" if it % 2 else "ACGT") for _ in range(rng.randrange(4, 44))).encode()
        for W, T in ((64, 20), (16, 12), (8, 5)):
            assert R.mask_flags(s, W, T) == R.by_enumeration(s, W, T), (s, W, T)


def test_rule_sanity_bounds(fixture):
    """taken on the brute force itself: ordinary sequence is left alone, the fixture's mix is neither ignored nor wiped out"""
    rng = random.Random(20261016)
    s = "".join(rng.choice("ACGT") for _ in range(100_000)).encode()
    frac = sum(R.mask_flags(s)) / len(s)
    print(f"uniformly random ACGT: {100 * frac:.3f} % masked")
    assert frac < 0.01
    recs, E = fixture
    n = sum(sum(R.mask_flags(r)) for r in recs)
    frac = n / E["n_bases"]
    print(f"fixture: {100 * frac:.1f} % masked")
    assert 0.20 <= frac <= 0.80


def test_fixture_expectation_is_the_brute_force(fixture):
    recs, E = fixture
    for W, T in PARAMS:
        e = E["masked"][f"{W},{T}"]
        iv = [R.intervals(R.mask_flags(r, W, T)) for r in recs]
        assert iv == e["intervals"] and sum(b - a for r in iv for a, b in r) == e["n_masked"]


# ---- the library's host mirror ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seq,want", KNOWN)
def test_known_answers_host(K, seq, want):
    (m,), st = K.mask_low_complexity_host([seq], return_stats=True)
    assert m == R.mask_records([seq])[0]
    assert st["n_masked"] == sum(R.mask_flags(seq)) and st["n_bases"] == len(seq)
    (soft,) = K.mask_low_complexity_host([seq], replacement=None)
    assert soft == R.mask_records([seq], replacement=None)[0] and soft.upper() == seq.upper()


def test_two_records_are_not_masked_across(K):
    """AAAA | AAAA: one record of 8 would be masked whole, two records of 4 hold 2 triplets each and score 1 / 1"""
    assert R.intervals(R.mask_flags(b"A" * 8)) == [[0, 8]]
    assert K.mask_low_complexity_host([b"A" * 8]) == [b"x" * 8]
    assert K.mask_low_complexity_host([b"A" * 4, b"A" * 4]) == [b"A" * 4, b"A" * 4]
    a, b = b"GATC" + b"AC" * 3, b"AC" * 3 + b"GGAT"          # (AC) x 6 across the border
    assert R.intervals(R.mask_flags(a + b)) != []
    assert K.mask_low_complexity_host([a, b]) == [a, b] == R.mask_records([a, b])


@pytest.mark.parametrize("W,T", PARAMS)
def test_host_equals_brute_force_on_the_fixture(K, fixture, W, T):
    recs, E = fixture
    e = E["masked"][f"{W},{T}"]
    for rep in (b"x", None):
        got, st = K.mask_low_complexity_host(recs, W, T, rep, return_stats=True)
        assert got == R.mask_records(recs, W, T, rep)
        assert [R.intervals(flags_of(g, r)) for g, r in zip(got, recs)] == e["intervals"] if rep else True
        assert st["n_masked"] == e["n_masked"] and st["n_bases"] == E["n_bases"]


@pytest.mark.parametrize("W,T", PARAMS)
def test_host_equals_brute_force_on_seeded_families(K, W, T):
    for seed in range(100, 112):
        recs = seeded_records(seed)
        assert K.mask_low_complexity_host(recs, W, T) == R.mask_records(recs, W, T), seed
        assert K.mask_low_complexity_host(recs, W, T, None) == R.mask_records(recs, W, T, None), seed


def test_defaults_and_refused_parameters(K):
    from scrubby_amd import lib as S
    seq = [b"ACGT" * 3 + b"A" * 30 + b"GATTACA"]
    assert K.mask_low_complexity_host(seq, 0, 0) == K.mask_low_complexity_host(seq, 64, 20)
    for W, T, word in ((7, 20, "window"), (65, 20, "window"), (64, -1, "threshold")):
        with pytest.raises(S.ScrubbyHipError) as ei:
            K.mask_low_complexity_host(seq, W, T)
        assert word in ei.value.message


def test_new_names_are_exported():
    from scrubby_amd import lib as S
    L = S.load()
    assert L.sh_version() == 104
    for name in ("sh_k2_mask_device", "sh_k2_mask_host", "sh_k2_mask_run"):
        assert name in S.EXPORTS and hasattr(L, name)
