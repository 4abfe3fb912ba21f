"""k_local_cluster alone (sh_dbg_repeat_shortcuts, the kernel's counting instance) on the growth table of tests/lc_cases_grow.py: what the
window's second to fourth round admit - on either side of a list, through more than one group of eight entries, up to the cap of 16 and up
to a K of 64, and never an entry of another contig - against the plain model of tests/lc_model.py and the CPU oracle's flags.  The checks
are those of tests/test_local_cluster_gpu.py (whose helpers are used): soundness, the partition of the list, lc_why per predicted outcome,
table order and a shuffled order, and the pair pass in front (mask 1, then both bits).  Integers only, no tolerance."""
import numpy as np
import pytest

from tests import lc_cases_grow as G_
from tests import lc_model as M
from tests.test_local_cluster_gpu import check_partition, model_hist, shortcuts

pytestmark = pytest.mark.gpu
DECIDED = (M.DECIDED, M.DECIDED_FILTERED)


@pytest.fixture(scope="module")
def S():
    from scrubby_amd import lib
    lib.require_gpu()
    return lib


@pytest.fixture(scope="module")
def T(oracle):
    return G_.cases(oracle)


@pytest.fixture(scope="module")
def ctx(S, T):
    mp = pytest.MonkeyPatch()
    mp.setenv("SCRUBBY_HIP_ARENA_MB", "96")       # the chain arena is not what these tests are about
    idx = S.Index.build([c.tobytes() for c in T.contigs[0]], S.preset("sr"))
    c = S.Context(idx, 1000, 400_000, 512)
    mp.undo()
    yield c
    c.close()
    idx.close()


@pytest.fixture(scope="module")
def grouped(S, T, ctx):
    """mask 2 over the reads of each predicted outcome, one call each -> per read its flag and whether it was listed, the calls' lc_why"""
    flag, listed_all, why = np.zeros(len(T.reads), np.uint8), np.zeros(len(T.reads), bool), {}
    for outcome in M.OUTCOMES + (M.SCORE_TIE,):
        sel = [i for i in T.of(0) if T.outcome(i) == outcome]
        if not sel:
            continue
        rc, out = shortcuts(S, ctx, [T.reads[i].seq for i in sel], 2)
        S.check(rc)
        listed, flagged, left = check_partition(out, len(sel))
        print(outcome, len(sel), "lc_why", out["lc_why"].tolist(), "flagged", int(flagged.sum()))
        flag[sel], listed_all[sel], why[outcome] = flagged, listed, out["lc_why"]
    return flag, listed_all, why


def test_soundness_and_the_decided_set(grouped, T):
    flag, listed, why = grouped
    name = lambda i: (T.reads[i].family, T.reads[i].sweep, T.reads[i].step, T.reads[i].rc)
    bad = [name(i) for i in np.where(flag == 1)[0] if T.flag[i] != 1]
    assert not bad, f"flagged reads the oracle does not map: {bad[:5]}"
    assert listed.all(), f"reads off the repeat list: {[name(i) for i in np.where(~listed)[0]][:5]}"
    odd = [name(i) for i, m in enumerate(T.model) if m.outcome != M.SCORE_TIE and (flag[i] == 1) != (m.outcome in DECIDED)]
    assert not odd, f"the kernel decides otherwise than the model: {len(odd)} reads, first {odd[:5]}"
    assert int(flag.sum()) >= 60, "the kernel decides next to nothing"


@pytest.mark.parametrize("outcome", (M.WINDOW, M.K_SIZE, M.DECIDED))
def test_reasons(grouped, T, outcome):
    """the reads of one predicted outcome in one call: lc_why is the model's histogram - a window that stopped growing a round early or took
    an entry too many shows here as a read counted under another reason"""
    flag, listed, why = grouped
    sel = [i for i in T.of(0) if T.outcome(i) == outcome]
    assert len(sel) >= 8
    assert np.array_equal(why[outcome], model_hist([T.model[i] for i in sel])), (outcome, len(sel), why[outcome].tolist())


def test_every_predicted_outcome_was_asked(grouped, T):
    flag, listed, why = grouped
    assert set(why) == {T.outcome(i) for i in T.of(0)}
    for outcome, h in why.items():
        if outcome != M.SCORE_TIE:
            assert np.array_equal(h, model_hist([T.model[i] for i in T.of(0) if T.outcome(i) == outcome])), (outcome, h.tolist())


@pytest.mark.parametrize("order", ("table", "shuffled"))
def test_order_independence(S, T, ctx, grouped, order):
    flag, listed, why = grouped
    sel = np.array(T.of(0))
    if order == "shuffled":
        sel = sel[np.random.default_rng(11).permutation(len(sel))]
    rc, out = shortcuts(S, ctx, [T.reads[i].seq for i in sel], 2)
    S.check(rc)
    l, f, _ = check_partition(out, len(sel))
    assert np.array_equal(l, listed[sel]) and np.array_equal(f, flag[sel] == 1), int((f != (flag[sel] == 1)).sum())
    assert np.array_equal(out["lc_why"].astype(np.uint64), sum(h.astype(np.uint64) for h in why.values()))


def test_pair_pass_in_front(S, T, ctx, grouped):
    """mask 1, then mask 3: k_local_cluster sees what the pair pass leaves, decides of it what it decides alone, and the union is sound"""
    flag, listed, _ = grouped
    sel = np.array(T.of(0))
    seqs = [T.reads[i].seq for i in sel]
    rc, p = shortcuts(S, ctx, seqs, 1)
    S.check(rc)
    l1, f1, left1 = check_partition(p, len(sel), lc_ran=False)
    assert p["info"][2] == 1 and p["info"][3] == 0 and not p["lc_why"].any()
    rc, b = shortcuts(S, ctx, seqs, 3)
    S.check(rc)
    l3, f3, left3 = check_partition(b, len(sel), lc_ran=False)
    assert b["info"][2] == 1 and b["info"][3] == 1 and np.array_equal(l3, l1) and np.array_equal(l1, listed[sel])
    assert int(b["lc_why"][0]) + int(b["lc_why"][-1]) == int(left1.sum()), "k_local_cluster did not walk the pair pass's leftover"
    assert np.array_equal(f3, f1 | ((flag[sel] == 1) & left1))
    assert not [i for i, x in zip(sel, f3) if x and T.flag[i] != 1]
