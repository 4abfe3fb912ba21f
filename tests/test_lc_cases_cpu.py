"""The case table of k_local_cluster (tests/lc_cases.py) and its model (tests/lc_model.py), held against the CPU oracle before the device is
asked anything: every edge of the kernel's premises occurs in the table on both sides, and - the lemma itself - a read the model calls
decided is a read the oracle maps.  No GPU."""
import collections

import numpy as np
import pytest

from tests import lc_cases as C
from tests import lc_model as M


@pytest.fixture(scope="module")
def T(oracle):
    return C.cases(oracle)


@pytest.mark.parametrize("rc_", (0, 1), ids=("forward", "reverse"))
def test_every_edge_occurs_on_both_sides(T, rc_):
    missing = C.missing_edges(T, rc_)
    assert not missing, f"the table lacks: {missing} (choose another TABLE_SEED)"


def test_what_the_model_decides_the_oracle_maps(T):
    """steps 1 to 3 of the kernel's argument, on the CPU: K's top chain out-scores U_out and passes chain_lemma or the middle check => flag 1"""
    decided = [i for i, m in enumerate(T.model) if m.outcome in (M.DECIDED, M.DECIDED_FILTERED)]
    bad = [(i, T.reads[i].family, T.reads[i].sweep, T.reads[i].step, T.reads[i].rc) for i in decided if T.flag[i] != 1]
    assert len(decided) > 1000 and not bad, f"{len(bad)} reads decided by the model that the oracle does not map, first {bad[:5]}"
    # The other direction does not hold and the table shows it: the oracle maps hundreds of reads the model leaves alone.  Reads it does NOT
    # map are few under the sr preset - a chain of two anchors already aligns to 40 and more - and all of them have a K of fewer than two
    # anchors: what keeps the kernel from deciding too eagerly is the comparison of its decisions with the model's, read by read.
    assert sum(T.flag[i] == 1 and T.model[i].outcome in (M.MARGIN, M.LEMMA, M.WINDOW) for i in range(len(T.reads))) > 100
    assert all(T.model[i].outcome in (M.NOT_LISTED, M.N_SEED, M.NO_SINGLETON, M.K_SIZE, M.LEMMA) for i in np.where(T.flag == 0)[0]) and int((T.flag == 0).sum()) >= 8


def test_score_ties_are_rare(T):
    general = sum("n_chain" in m.detail for m in T.model)
    ties = sum(m.outcome == M.SCORE_TIE for m in T.model)
    assert general > 1000 and ties <= 0.02 * general, (ties, general)


def test_size_and_buckets(T):
    hist = collections.Counter(m.outcome for m in T.model)
    print(len(T.reads), "reads:", {o: hist[o] for o in M.OUTCOMES + (M.SCORE_TIE,)})
    assert len(T.reads) <= 6000
    assert all(hist[o] >= 8 for o in M.OUTCOMES), hist
    # every read is there in both orientations, next to each other
    assert all(a.seq == C.rc(b.seq) and (a.rc, b.rc) == (0, 1) for a, b in zip(T.reads[0::2], T.reads[1::2]))
    assert {r.ctx for r in T.reads} == {0, 1} and max(len(r.seq) for r in T.reads) <= 512


def test_both_orientations_end_alike(T):
    """a read and its reverse complement have the same seeds at mirrored places: the model's outcome may differ only where a tie of minimizers
    or of chains is broken by position"""
    diff = [(a.family, a.sweep, a.step) for a, b, ma, mb in zip(T.reads[0::2], T.reads[1::2], T.model[0::2], T.model[1::2]) if ma.outcome != mb.outcome]
    assert len(diff) <= 0.01 * len(T.reads), diff[:10]


def test_the_models_pieces_on_known_answers(oracle):
    o = oracle.preset("sr")
    assert M.lemma_premises(o) == (True, True)
    assert (M.max_dist_x(o, 150), M.max_dist_x(o, 400), M.max_dist_x(o, 750), M.max_dist_y(o, 150), M.max_dist_y(o, 60)) == (650, 400, 100, 150, 100)
    assert C.MDX == M.max_dist_x(o, C.QLEN) and o.zdrop // o.b == 12 and (o.k, o.w, o.mid_occ, o.min_chain_score) == (C.K, C.W, 1000, 25)
    # anchors: same strand, and opposite strands (the query position is mirrored, bit 63 set)
    assert M.anchor(7 << 32 | 500 << 1 | 1, 90 << 1 | 1, 150, 21) == (7 << 32 | 500, 90)
    assert M.anchor(7 << 32 | 500 << 1, 90 << 1 | 1, 150, 21) == (1 << 63 | 7 << 32 | 500, 150 - (90 + 1 - 21) - 1)
    # the middle check: +2 a match, -8 a mismatch; the drop is measured from the best score so far
    ref = [np.frombuffer(b"ACGTACGTACGTACGTACGT", np.uint8)]
    assert M.middle_max_drop(o, ref, b"ACGTACGTACGTACGTACGT", 0, 0, 0, 20, 0) == 0
    assert M.middle_max_drop(o, ref, b"ACGTTTTTACGTACGTACGT", 0, 0, 0, 20, 0) == 3 * 8             # T against A, C and G, then a match
    assert M.middle_max_drop(o, ref, C.rc(b"ACGTACGTACGTACGTACGT"), 0, 1, 0, 20, 0) == 0
    assert M.middle_max_drop(o, ref, b"ACGTACGTACNTACGTACGT", 0, 0, 0, 20, 0) == 1                   # sc_ambi
    # chain_lemma: one co-diagonal run of three anchors 10 apart: covered 41, span 20 < k; four: span 30
    x, q = [100, 110, 120, 130], [20, 30, 40, 50]
    assert M.chain_lemma(o, 12, x, q, [-1, 0, 1, 2], 2, -1)[0] == 0 and M.chain_lemma(o, 12, x, q, [-1, 0, 1, 2], 3, -1) == (1, (20, 50, 100))
    # two runs (an insertion between anchors 1 and 2): the later run wins with equal cover only if it is the earlier one walked, i.e. >=
    x, q = [100, 121, 143, 164], [20, 41, 62, 83]
    assert M.chain_lemma(o, 12, x, q, [-1, 0, 1, 2], 3, -1) == (1, (20, 41, 100))
    # bases outside the k-mers: a gap of 21 + 13 takes the middle check, 21 + 12 does not
    assert M.chain_lemma(o, 12, [100, 134], [20, 54], [-1, 0], 1, -1)[0] == 2 and M.chain_lemma(o, 12, [100, 133], [20, 53], [-1, 0], 1, -1)[0] == 1
    assert C.first_round_pivots(13) == [1, 3, 5, 7, 9, 11] and C.first_round_pivots(513)[:2] == [64, 129] and C.first_round_pivots(64) == [7, 15, 23, 31, 39, 47, 55]
