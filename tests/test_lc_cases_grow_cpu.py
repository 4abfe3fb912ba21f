"""The second case table of k_local_cluster (tests/lc_cases_grow.py: what the window's later rounds admit) under the unchanged model
(tests/lc_model.py), held against the CPU oracle before the device is asked anything: every growth edge occurs in the table on both sides,
and a read the model calls decided is a read the oracle maps.  No GPU."""
import collections

import pytest

from tests import lc_cases_grow as G
from tests import lc_model as M


@pytest.fixture(scope="module")
def T(oracle):
    return G.cases(oracle)


@pytest.mark.parametrize("rc_", (0, 1), ids=("forward", "reverse"))
def test_every_growth_edge_occurs_on_both_sides(oracle, T, rc_):
    missing = G.missing_edges(oracle, T, rc_)
    assert not missing, f"the table lacks: {missing} (choose another TABLE_SEED)"


def test_what_the_model_decides_the_oracle_maps(T):
    decided = [i for i, m in enumerate(T.model) if m.outcome in (M.DECIDED, M.DECIDED_FILTERED)]
    bad = [(T.reads[i].family, T.reads[i].sweep, T.reads[i].step, T.reads[i].rc) for i in decided if T.flag[i] != 1]
    assert len(decided) >= 60 and not bad, f"{len(bad)} reads decided by the model that the oracle does not map, first {bad[:5]}"


def test_size_and_shape(T):
    hist = collections.Counter((r.family, m.outcome) for r, m in zip(T.reads, T.model))
    print(len(T.reads), "reads:", dict(hist))
    assert 150 <= len(T.reads) <= 400 and sum(len(c) for c in T.contigs[0]) <= 800_000
    assert all(len(r.seq) == G.QLEN for r in T.reads)
    assert all(a.seq == G.rc(b.seq) and (a.rc, b.rc) == (0, 1) for a, b in zip(T.reads[0::2], T.reads[1::2]))
    assert all(m.outcome != M.NOT_LISTED for m in T.model), "a read of the table is not on the repeat list"
    assert {r.family for r in T.reads} == {"above", "both", "tandem", "cumcap", "k2nd", "contig"}
    # the rounds the table walks: every count of 2 to 4, ended by a break and by the refusal
    assert {m.rounds for m in T.model} >= {2, 3, 4}
