"""Column 5 of kraken.reads: Kraken 2's hit list, formatted on the host by sh_k2_format_hits from one unit's (code, count)
entries, the taxonomy's external ids and the --quick flag.  No GPU needed.  `rle` restates how the entries come from the
per-k-mer taxa that oracle/k2_oracle.c lists (tests/test_k2_hitlist_gpu.py compares the kernel with it)."""
import numpy as np
import pytest

A, B = 0xFFFFFFFF, 0xFFFFFFFE           # the oracle's ambiguous k-mer and mate border (SH_K2_HIT_AMBIGUOUS / _BORDER)
EXT = np.array([0, 1, 131567, 9606, 9605, 562, 4294967295 - 7], dtype=np.uint32)       # external ids by internal id


def rle(taxa):
    """entries of the per-k-mer taxa sequence: runs of one code merge, the border never does and counts 0"""
    out = []
    for t in (int(x) for x in taxa):
        if t == B:
            out.append((B, 0))
        elif out and out[-1][0] == t and t != B:
            out[-1] = (t, out[-1][1] + 1)
        else:
            out.append((t, 1))
    return out


def col5(entries, external=EXT):
    """the same column restated in Python"""
    if not entries:
        return "0:0"
    return " ".join("|:|" if c == B else f"A:{n}" if c == A else f"{int(external[c])}:{n}" for c, n in entries)


@pytest.fixture(scope="module")
def K():
    from scrubby_amd import k2
    return k2


def test_merged_runs_and_unclassified_runs(K):
    taxa = [3, 3, 3, 4, 4, 0, 0, 0, 3, 3, 5]
    assert rle(taxa) == [(3, 3), (4, 2), (0, 3), (3, 2), (5, 1)]
    assert K.format_hits(rle(taxa), EXT) == "9606:3 9605:2 0:3 9606:2 562:1"
    # two runs of different minimizers with one taxon are one entry; so are adjacent entries the caller did not merge
    assert K.format_hits(rle([3] * 5 + [3] * 7), EXT) == "9606:12"
    assert K.format_hits([(0, 116)], EXT) == "0:116"


@pytest.mark.parametrize("taxa, want", [
    ([A, A, 3, 3, 3], "A:2 9606:3"),                 # start
    ([3, 3, A, A, A, 3, 4], "9606:2 A:3 9606:1 9605:1"),   # middle: a run resumed after the span is a new entry
    ([5, 5, 0, A], "562:2 0:1 A:1"),                 # end
    ([A] * 9, "A:9"),
])
def test_ambiguous_spans(K, taxa, want):
    assert K.format_hits(rle(taxa), EXT) == want == col5(rle(taxa))


@pytest.mark.parametrize("taxa, want", [
    ([B, 3, 3], "|:| 9606:2"),                       # mate 1 without k-mers
    ([3, 3, B, 3, 3], "9606:2 |:| 9606:2"),          # the border never merges
    ([A, 4, B, A, A], "A:1 9605:1 |:| A:2"),
    ([3, B], "9606:1 |:|"),                          # mate 2 without k-mers
    ([B], "|:|"),                                    # both mates shorter than k
])
def test_mate_border(K, taxa, want):
    assert K.format_hits(rle(taxa), EXT) == want == col5(rle(taxa))


def test_empty_single_read_and_quick_mode(K):
    assert K.format_hits([], EXT) == "0:0"
    assert K.format_hits(np.zeros(0, dtype=K.HIT_DTYPE), EXT) == "0:0"
    assert K.format_hits([], EXT, quick=True, quick_taxid=9606) == "9606:Q"
    assert K.format_hits([], EXT, quick=True, quick_taxid=0) == "0:Q"
    assert K.format_hits([(3, 10), (B, 0)], EXT, quick=True, quick_taxid=562) == "562:Q"     # entries ignored


def test_external_ids_no_trailing_space_and_bad_codes(K):
    s = K.format_hits([(6, 4294967), (2, 1), (1, 2), (B, 0), (A, 4000000000)], EXT)
    assert s == "4294967288:4294967 131567:1 1:2 |:| A:4000000000"
    assert not s.endswith(" ") and "  " not in s
    other = np.arange(100, 107, dtype=np.uint32)
    assert K.format_hits([(3, 1), (0, 2)], other) == "103:1 100:2"
    from scrubby_amd.lib import ScrubbyHipError
    with pytest.raises(ScrubbyHipError, match="outside the taxonomy"):
        K.format_hits([(7, 1)], EXT)


def test_long_list_round_trip(K):
    rng = np.random.default_rng(5)
    taxa = []
    for _ in range(400):
        taxa += [int(rng.choice([0, 1, 2, 3, 4, 5, 6, A]))] * int(rng.integers(1, 20))
        if rng.random() < 0.01:
            taxa.append(B)
    e = rle(taxa)
    s = K.format_hits(np.array(e, dtype=K.HIT_DTYPE), EXT)
    assert s == col5(e)
    assert sum(int(x.split(":")[1]) for x in s.split() if x != "|:|") == sum(1 for t in taxa if t != B)
