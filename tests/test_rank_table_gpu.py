"""The rank table of the parallel fills (pf_rank_sort in csrc/sh_chain.h: the mask of query positions, its 16-word prefix `qpre`, the
`start[]` prefix over the ranks), through the par-fill variants of sh_dbg_chain: par_fill_block and par_fill_tiled, four and eight lanes.

tests/chain_cases.py reaches the caps with workload-like shapes; these cases sit on the table's own edges: a read whose anchors share one
query position (one rank), exactly PF_MAX_RANK distinct positions (each once, and each twice), PF_MAX_RANK + 1 (the fill must decline and
leave the read to the sequential code), and positions in the first and last bit of a mask word and of the table (0, 63, 64, 1023), alone
and together with every multiple of 64.  Compared the way tests/test_chain_gpu.py compares: f and p of every clean cluster against the
oracle's arrays, the return value and the dirty marks against the model.  Integers only."""
import numpy as np
import pytest

from tests import chain_cases as K
from tests import chain_ref as R
from tests.test_chain_gpu import Batch, _clusters, _ints, _marked

pytestmark = pytest.mark.gpu
VARIANTS = (("pf_block", {}), ("pf_tiled", {}), ("pf_tiled8", {"g_min": 1}))


def _diag_q(qs, r0=1000):
    """one anchor per query position on one diagonal, in clusters of 20 that lie 6000 apart (beyond max_dist_x): no anchor has more than
    max_skip valid predecessors, so every cluster comes out clean and its f / p show what the rank table held"""
    return [(r0 + q + 6000 * (t // 20), q) for t, q in enumerate(qs)]


def cases():
    T = []
    add = T.append
    o = K.SRW      # max_dist_x = 5000, max_dist_y = qlen: a diagonal across the whole table is one cluster
    add(K._case("rank_one", "rank", o, 1024, [(1000 + 5 * t, 500) for t in range(40)]))
    add(K._case("rank_one_anchor", "rank", o, 1024, [(1000, 0)]))
    for n_rank in (2, K.PF_MAX_RANK - 1, K.PF_MAX_RANK, K.PF_MAX_RANK + 1):
        qs = [3 + 7 * t for t in range(n_rank)]      # 3 .. 899: every mask word
        add(K._case(f"rank_{n_rank}", "rank", o, 1024, _diag_q(qs)))
        twice = sorted(_diag_q(qs) + _diag_q(qs, r0=1400))      # a second diagonal 400 off (beyond bw) in the same clusters: same ranks, two anchors each
        add(K._case(f"rank_{n_rank}_twice", "rank", o, 1024, twice))
    for q in (0, 63, 64, 1023):
        add(K._case(f"q_{q}", "rank", o, 1024, _diag_q([q]) + [(3000 + t, q) for t in range(3)]))
    add(K._case("q_edges", "rank", o, 1024, _diag_q([0, 63, 64, 1023])))
    words = sorted(set([64 * w for w in range(16)] + [64 * w + 63 for w in range(16)]))      # both ends of all 16 mask words: 32 ranks
    add(K._case("q_word_ends", "rank", o, 1024, _diag_q(words)))
    add(K._case("q_last_word_full", "rank", o, 1024, _diag_q(range(960, 1024))))             # 64 ranks in qpre's last word
    return T


@pytest.fixture(scope="module")
def ran(oracle):
    """one launch per variant over every case: (case, the oracle's f / p, the model's verdict, what each variant returned)"""
    T = cases()
    B, idx = Batch(), {}
    for c in T:
        off = B.anchors(c["x"], _marked(c))
        for v, kw in VARIANTS:
            idx[c["name"], v] = B.add(off, len(c["x"]), c["qlen"], c["o"], dp=v.rstrip("8"), **kw)
    out = B.run()
    rows = []
    for c in T:
        f, p, _ = K.oracle_case(oracle, c)
        ev = K.model_case(oracle, c).events
        rows.append((c, f, p, R.par_fill_model(c["o"], c["qlen"], _ints(c["x"]), _ints(c["q"]), ev), {v: out[idx[c["name"], v]] for v, _ in VARIANTS}))
    return rows


def test_the_cases_reach_the_edges_of_the_table():
    n_rank = {c["name"]: len(set(_ints(c["q"]))) for c in cases()}
    assert n_rank["rank_one"] == 1 and n_rank[f"rank_{K.PF_MAX_RANK}"] == n_rank[f"rank_{K.PF_MAX_RANK}_twice"] == K.PF_MAX_RANK == 128
    assert n_rank[f"rank_{K.PF_MAX_RANK + 1}"] == n_rank[f"rank_{K.PF_MAX_RANK + 1}_twice"] == 129
    seen = set()
    for c in cases():
        seen |= set(_ints(c["q"]))
    assert {0, 63, 64, 1023} <= seen and max(seen) == K.PF_MAX_Q - 1


@pytest.mark.parametrize("variant", [v for v, _ in VARIANTS])
def test_rank_table_edges(variant, ran):
    bad, n_true, n_declined, n_cmp = [], 0, 0, 0
    for c, f, p, (applies, dirty, starts), got in ran:
        g = got[variant]
        n_rank = len(set(_ints(c["q"])))
        assert applies == (n_rank <= K.PF_MAX_RANK), c["name"]      # nothing else in these cases makes a fill decline
        if bool(g["ret"]) != applies:
            bad.append(c["name"] + ":ret")
        if not g["ret"]:
            n_declined += 1
            continue
        n_true += 1
        marked = {a for a, _ in _clusters(starts) if g["t"][a] == K.PF_DIRTY}
        if marked != dirty or set(np.unique(g["t"]).tolist()) - {0, K.PF_DIRTY}:
            bad.append(c["name"] + ":dirty")
        for a, b in _clusters(starts):
            if a not in marked:
                n_cmp += b - a
                if not (np.array_equal(g["f"][a:b], f[a:b]) and np.array_equal(g["p"][a:b], p[a:b])):
                    bad.append(f"{c['name']}:{a}")
    assert not bad and n_declined == 2 and n_true == len(ran) - 2 and n_cmp >= 900, (variant, n_true, n_declined, n_cmp, bad)
