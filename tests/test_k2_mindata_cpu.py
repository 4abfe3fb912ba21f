"""kraken2 --report-minimizer-data, the host side: the HyperLogLog estimator (sh_k2_hll_estimate), the register merge, the
8-column report writer, and the self-check of the model (tests/k2_mindata_ref.py) the GPU tests compare against.  No GPU."""
import math
import os

import numpy as np
import pytest

from tests import k2_mindata_ref as R
from tests.test_k2_options_cpu import _batch, _reads, _toy

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "k2_mindata")
STD_ERR = 1.04 / math.sqrt(R.M)         # of an HLL with m registers: 1.625 %


@pytest.fixture(scope="module")
def K():
    from scrubby_amd import k2
    return k2


def _random_values(n, seed):
    return np.random.default_rng(seed).integers(0, 1 << 64, n, dtype=np.uint64)


def _close(K, regs):
    got, want = K.hll_estimate(regs), R.estimate(regs)
    if math.isinf(want):
        assert math.isinf(got)
        return got
    assert abs(got - want) <= 1e-12 * max(abs(want), 1e-300), (got, want)
    assert R.rounded(got) == R.rounded(want)
    return got


def test_register_rules():
    assert R.fmix64(0) == 0 and R.register_of(0) == (0, 53)              # w == 0: rank 53
    v = _random_values(2000, 1)
    assert np.array_equal(R.registers_np(v), R.registers(v.tolist()))
    h = R.fmix64(int(v[0]))
    assert R.register_of(int(v[0]))[0] == h >> 52


def test_estimator_edge_inputs(K):
    assert _close(K, np.zeros(R.M, np.uint8)) == 0.0
    one = np.zeros(R.M, np.uint8); one[77] = 3
    e = _close(K, one)
    assert R.rounded(e) == 1
    _close(K, np.full(R.M, 53, np.uint8))
    from scrubby_amd.lib import ScrubbyHipError
    with pytest.raises(ScrubbyHipError, match="register"):
        K.hll_estimate(np.full(R.M, 54, np.uint8))


@pytest.mark.parametrize("n, seed", [(1, 101), (10, 102), (1000, 103), (50_000, 104), (2_000_000, 105)])
def test_estimator_against_the_true_count(K, n, seed):
    regs = R.registers_np(_random_values(n, seed))
    want = R.estimate(regs)
    # a condition on the inputs: the Python estimator itself is within 5 standard errors on this seed
    assert abs(want - n) <= max(1.0, 5 * STD_ERR * n), (want, n)
    got = _close(K, regs)
    assert abs(got - n) <= max(1.0, 5 * STD_ERR * n)


def test_merge_host(K):
    rng = np.random.default_rng(7)
    a, b = rng.integers(0, 54, 3 * R.M).astype(np.uint8), rng.integers(0, 54, 3 * R.M).astype(np.uint8)
    want = np.maximum(a, b)
    got = K.hll_merge(a.copy(), b)
    assert np.array_equal(got, want)
    # the merge of two sketches is the sketch of the union
    x, y = _random_values(3000, 8), _random_values(3000, 9)
    u = K.hll_merge(R.registers_np(x), R.registers_np(y))
    assert np.array_equal(u, R.registers_np(np.concatenate([x, y])))


# a hand-made taxonomy of 7 nodes: 1 root - 2 Bacteria (superkingdom) - {3 Proteobacteria (phylum) - {5 E. coli, 6 S. enterica},
# 4 Firmicutes (phylum) - nothing below}; breadth-first ids, children consecutive
PARENTS = [0, 0, 1, 2, 2, 3, 3]
EXTERNALS = [0, 1, 2, 1224, 1239, 562, 28901]
NAMES = ["", "root", "Bacteria", "Proteobacteria", "Firmicutes", "Escherichia coli", "Salmonella enterica"]
RANKS = ["", "no rank", "superkingdom", "phylum", "phylum", "species", "species"]
DIRECT = [0, 2, 0, 5, 40, 100, 13]
CLADE_MIN = [0, 9000, 8990, 7000, 1990, 6000, 900]
CLADE_DISTINCT = [0, 4100, 4090, 3300, 60, 3000, 410]


def _clade(direct):
    c = list(direct)
    for i in range(len(c) - 1, 1, -1):
        c[PARENTS[i]] += c[i]
    return c


def test_report_writer_against_the_hand_written_file(K, tmp_path):
    nodes, npool, rpool = K.make_taxonomy(PARENTS, EXTERNALS, NAMES, RANKS)
    total = sum(DIRECT) + 40                                # 40 unclassified units
    K.write_minimizer_report(nodes, npool, rpool, _clade(DIRECT), DIRECT, CLADE_MIN, CLADE_DISTINCT, total, tmp_path / "r.txt")
    got = open(tmp_path / "r.txt").read()
    assert got == open(os.path.join(GOLDEN, "report7.txt")).read()
    assert all(len(l.split("\t")) == 8 for l in got.splitlines())
    # and the model's writer, which the GPU tests use, says the same
    fc = [nodes[i].first_child for i in range(7)]; cc = [nodes[i].child_count for i in range(7)]
    assert R.report_text(PARENTS, fc, cc, NAMES, RANKS, EXTERNALS, DIRECT, CLADE_MIN, CLADE_DISTINCT, total) == got


def test_report_without_the_two_columns_is_the_six_column_layout(K, tmp_path):
    nodes, npool, rpool = K.make_taxonomy(PARENTS, EXTERNALS, NAMES, RANKS)
    total = sum(DIRECT)                                     # every unit classified: the counts report has no unclassified row
    K.write_minimizer_report(nodes, npool, rpool, _clade(DIRECT), DIRECT, CLADE_MIN, CLADE_DISTINCT, total, tmp_path / "r8.txt")
    K.counts_report(nodes, npool, rpool, DIRECT, tmp_path / "r6.txt")
    six = ["\t".join(c for i, c in enumerate(l.split("\t")) if i not in (3, 4)) for l in open(tmp_path / "r8.txt").read().splitlines()]
    assert six == open(tmp_path / "r6.txt").read().splitlines() and len(six) == 6


def test_report_writer_refuses_bad_input(K, tmp_path):
    from scrubby_amd.lib import ScrubbyHipError
    nodes, npool, rpool = K.make_taxonomy(PARENTS, EXTERNALS, NAMES, RANKS)
    with pytest.raises(ScrubbyHipError, match="classified"):
        K.write_minimizer_report(nodes, npool, rpool, _clade(DIRECT), DIRECT, CLADE_MIN, CLADE_DISTINCT, 3, tmp_path / "x.txt")


def test_model_self_check_on_a_small_table(oracle):
    """events == hit_groups and lookups == n_probes for every unit (asserted inside Model.events), single and paired, plain and
    down-sampled; --quick keeps the first min_hit_groups events"""
    t, o, seqs = _toy(oracle)
    assert all(R.fmix64(m) == oracle.lib().k2o_hash(m) for m in (0, 1, 0xdeadbeef, (1 << 64) - 1))
    rng = np.random.default_rng(21)
    recs = _reads(seqs, 120, rng)
    recs[3] = recs[3][:20]                                  # shorter than k
    recs[4] = recs[5][-40:] + recs[5][-40:]
    bases, off = _batch(recs)
    m = R.Model(oracle, t, o)
    for paired in (False, True):
        ev = m.events(bases, off, paired)
        assert sum(len(e) for e in ev) > 200 and (paired or any(not e for e in ev))       # single: a random read, the short one
        for mhg in (1, 2):
            q = m.events(bases, off, paired, quick=True, min_hit_groups=mhg)
            assert all(len(a) == min(len(b), mhg) if len(b) >= mhg else a == b for a, b in zip(q, ev))
            assert all(a == b[:len(a)] for a, b in zip(q, ev))
    e = R.Expected(t.parent).add(m.events(bases, off, False))
    assert int(e.count.sum()) == sum(len(x) for x in m.events(bases, off, False))
    assert all(len(s) <= int(c) for s, c in zip(e.sets, e.count))
    # clade values: sums and unions up the tree
    cc, cs, cr = e.clade_count(), e.clade_sets(), e.clade_regs()
    assert int(cc[1]) == int(e.count.sum()) and cs[1] == set().union(*e.sets)
    assert np.array_equal(cr[1], R.registers(cs[1]))
    # down-sampled: fewer lookups, still the oracle's numbers
    o2 = oracle.k2_default_opts(); o2.value_bits = o.value_bits; o2.min_acceptable_hash = 1 << 63
    ev2 = R.Model(oracle, t, o2).events(bases, off, True)
    assert 0 < sum(len(x) for x in ev2) < sum(len(x) for x in m.events(bases, off, True))
