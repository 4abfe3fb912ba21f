"""k_local_cluster alone (sh_dbg_repeat_shortcuts: front end, then the repeat list's shortcuts under a mask, the kernel's counting instance)
on the case table of tests/lc_cases.py, against the plain model of tests/lc_model.py and the CPU oracle's flags.  The table walks every
premise of the kernel across its edge; test_lc_cases_cpu.py has checked that both sides of each are there.  Integers only, no tolerance:

  soundness   a read the kernel flags is a read the oracle maps
  partition   flagged + leftover = the repeat list, disjoint, nothing twice, reads off the list untouched, lc_why adds up to the list
  reasons     the reads of one predicted outcome in one call: lc_why is the model's histogram, the flagged reads are the model's decided reads
  order       the whole table in one call, in table order and shuffled: the same decisions, the counters the sum of the grouped calls'
so that a kernel that decides too eagerly, or that silently decides nothing (full-path flags would still be right), fails here."""
import collections
import ctypes as C

import numpy as np
import pytest

from tests import lc_cases as T_
from tests import lc_model as M

pytestmark = pytest.mark.gpu
BAD_ARG = 1
LISTED, LEFT, TWICE = 1, 2, 0x80
DECIDED = (M.DECIDED, M.DECIDED_FILTERED)
MAX_READS, MAX_BASES, MAX_LEN = 6000, 2_000_000, 512


@pytest.fixture(scope="module")
def S():
    from scrubby_amd import lib
    lib.require_gpu()
    return lib


@pytest.fixture(scope="module")
def T(oracle):
    return T_.cases(oracle)


def gpu_opts(S, ctx):
    o = S.preset("sr")
    if ctx == 1:
        o.mid_occ, o.max_occ, o.q_occ_frac = T_.HIGH_MID_OCC, T_.HIGH_MAX_OCC, 0.0
    return o


@pytest.fixture(scope="module")
def G(S, T):
    """per context of the table: the GPU index and an sh_ctx on it"""
    mp = pytest.MonkeyPatch()
    mp.setenv("SCRUBBY_HIP_ARENA_MB", "96")       # the chain arena is not what these tests are about
    idx = [S.Index.build([c.tobytes() for c in T.contigs[i]], gpu_opts(S, i)) for i in (0, 1)]
    ctx = [S.Context(ix, MAX_READS, MAX_BASES, MAX_LEN) for ix in idx]
    mp.undo()
    yield idx, ctx
    for c in ctx:
        c.close()
    for ix in idx:
        ix.close()


def shortcuts(S, ctx, seqs, mask, trace=None):
    """sh_dbg_repeat_shortcuts on the reads `seqs` -> (status, dict of what it copies out)"""
    import torch
    L = S.require_gpu()
    n = len(seqs)
    bases, offs = T_.batch(seqs)
    d_b = torch.from_numpy(np.concatenate([bases, np.frombuffer(b"ACGTTGCA" * 8, np.uint8)])).cuda()
    d_o = torch.from_numpy(offs.astype(np.int64)).cuda()
    torch.cuda.synchronize()
    out = {"k1info": np.zeros(max(n, 1), np.uint32), "route": np.full(max(n, 1), 0xEE, np.uint8), "flags": np.full(max(n, 1), 0xEE, np.uint8),
           "lc_why": np.zeros(len(M.LC_WHY), np.uint32), "pair_mid": np.zeros(4, np.uint32), "info": np.full(4, -1, np.int32)}
    rc = L.sh_dbg_repeat_shortcuts(ctx.h, C.c_void_p(d_b.data_ptr()), C.c_void_p(d_o.data_ptr()), n, len(bases), trace, mask,
                                   *(out[k].ctypes.data for k in ("k1info", "route", "flags", "lc_why", "pair_mid", "info")))
    return rc, out


def check_partition(out, n, lc_ran=True):
    """what holds for every call: -> (listed, flagged, leftover) as boolean arrays"""
    route, flags, info = out["route"][:n], out["flags"][:n], out["info"]
    assert not (route & TWICE).any() and not (route & ~np.uint8(LISTED | LEFT | TWICE)).any(), "a list names a read twice"
    assert set(np.unique(flags)) <= {0, 1}
    listed, left, flagged = (route & LISTED) != 0, (route & LEFT) != 0, flags == 1
    assert not (flagged & left).any(), "a read is flagged and left over"
    assert np.array_equal(flagged | left, listed), "flagged + leftover is not the repeat list (reads off the list must stay untouched)"
    assert info[0] == int(listed.sum()) and info[1] == int(left.sum())
    if lc_ran:
        why = out["lc_why"]
        assert info[3] == 1 and int(why[0]) + int(why[M.LC_WHY.index(M.N_SEED)]) == int(listed.sum()), (why, int(listed.sum()))
        assert int(why[1:-1].sum()) == int(why[0]), why
        assert int(why[M.LC_WHY.index(M.DECIDED)]) + int(why[M.LC_WHY.index(M.DECIDED_FILTERED)]) == int(flagged.sum())
    return listed, flagged, left


def model_hist(models):
    h = np.zeros(len(M.LC_WHY), np.uint32)
    for m in models:
        assert m.outcome != M.SCORE_TIE
        if m.outcome != M.NOT_LISTED:
            h[M.LC_WHY.index(m.outcome)] += 1
            h[0] += m.outcome != M.N_SEED
    return h


@pytest.fixture(scope="module")
def grouped(S, T, G):
    """mask 2 (k_local_cluster alone) over the reads of each (context, predicted outcome), one call each -> per read its flag and whether it
    was listed, per context the sum of the calls' lc_why, per (context, outcome) the call's lc_why; the partition is checked here"""
    idx, ctx = G
    flag, listed_all = np.zeros(len(T.reads), np.uint8), np.zeros(len(T.reads), bool)
    why_sum = [np.zeros(len(M.LC_WHY), np.uint64), np.zeros(len(M.LC_WHY), np.uint64)]
    why = {}
    for c in (0, 1):
        for outcome in M.OUTCOMES + (M.SCORE_TIE,):
            sel = [i for i in T.of(c) if T.outcome(i) == outcome]
            if not sel:
                continue
            rc, out = shortcuts(S, ctx[c], [T.reads[i].seq for i in sel], 2)
            S.check(rc)
            listed, flagged, left = check_partition(out, len(sel))
            print(c, outcome, len(sel), "lc_why", out["lc_why"].tolist(), "flagged", int(flagged.sum()))
            flag[sel], listed_all[sel] = flagged, listed
            why_sum[c] += out["lc_why"]
            why[(c, outcome)] = out["lc_why"]
    return flag, listed_all, why_sum, why


def test_index_is_the_one_the_model_read(oracle, T, G):
    idx, ctx = G
    for c in (0, 1):
        got = oracle.Index.wrap(*idx[c].export(), T_.W, T_.K).dump()
        want = T.cidx[c].dump()
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        grp = np.repeat(np.arange(len(got[0])), got[1].astype(np.int64))
        assert np.array_equal(got[2], got[2][np.lexsort((got[2], grp))]), "an occurrence list of the GPU index is not ascending"
        assert np.array_equal(got[2], want[2][np.lexsort((want[2], grp))])


def test_soundness_routing_and_the_decided_set(grouped, T):
    flag, listed, why_sum, why = grouped
    name = lambda i: (T.reads[i].family, T.reads[i].sweep, T.reads[i].step, T.reads[i].rc)
    bad = [name(i) for i in np.where(flag == 1)[0] if T.flag[i] != 1]
    assert not bad, f"flagged reads the oracle does not map: {bad[:5]}"
    odd = [name(i) for i, m in enumerate(T.model) if listed[i] != (m.outcome != M.NOT_LISTED)]
    assert not odd, f"the front end routes reads otherwise than the model: {odd[:5]}"
    # (who wins a tie hangs on a hash: only soundness and the partition are asked of those reads)
    odd = [name(i) for i, m in enumerate(T.model) if m.outcome != M.SCORE_TIE and (flag[i] == 1) != (m.outcome in DECIDED)]
    assert not odd, f"the kernel decides otherwise than the model: {len(odd)} reads, first {odd[:5]}"
    assert int(flag.sum()) > 1000, "the kernel decides next to nothing"


@pytest.mark.parametrize("outcome", M.OUTCOMES)
def test_reasons(grouped, T, outcome):
    """the reads of one predicted outcome in one call: lc_why is the model's histogram.  (MARGIN is the case that found the co-diagonal branch
    dead on the device: 11 reads whose K is one co-diagonal run covering 24 < min_chain_score bases and no more than U_out are counted under
    MARGIN only by that branch - the general path finds no chain and leaves them under LEMMA.)"""
    flag, listed, why_sum, why = grouped
    n = 0
    for c in (0, 1):
        sel = [i for i in T.of(c) if T.outcome(i) == outcome]
        if sel:
            assert np.array_equal(why[(c, outcome)], model_hist([T.model[i] for i in sel])), (c, outcome, len(sel), why[(c, outcome)].tolist())
            n += len(sel)
    assert n >= 8


@pytest.mark.parametrize("order", ("table", "shuffled"))
def test_order_independence(S, T, G, grouped, order):
    idx, ctx = G
    flag, listed, why_sum, _ = grouped
    for c in (0, 1):
        sel = np.array(T.of(c))
        if order == "shuffled":
            sel = sel[np.random.default_rng(7 + c).permutation(len(sel))]
        rc, out = shortcuts(S, ctx[c], [T.reads[i].seq for i in sel], 2)
        S.check(rc)
        l, f, _ = check_partition(out, len(sel))
        assert np.array_equal(l, listed[sel]) and np.array_equal(f, flag[sel] == 1), (c, int((f != (flag[sel] == 1)).sum()))
        assert np.array_equal(out["lc_why"].astype(np.uint64), why_sum[c]), (out["lc_why"].tolist(), why_sum[c].tolist())
        assert not [i for i, x in zip(sel, f) if x and T.flag[i] != 1]


def test_pair_pass_in_front(S, T, G, grouped):
    """mask 1, then mask 3: k_local_cluster sees what the pair pass leaves, decides of it what it decides alone, and the union is sound"""
    idx, ctx = G
    flag, listed, _, _ = grouped
    for c in (0, 1):
        sel = np.array(T.of(c))
        seqs = [T.reads[i].seq for i in sel]
        rc, p = shortcuts(S, ctx[c], seqs, 1)
        S.check(rc)
        l1, f1, left1 = check_partition(p, len(sel), lc_ran=False)
        assert p["info"][2] == 1 and p["info"][3] == 0 and not p["lc_why"].any()
        rc, b = shortcuts(S, ctx[c], seqs, 3)
        S.check(rc)
        l3, f3, left3 = check_partition(b, len(sel), lc_ran=False)
        assert b["info"][2] == 1 and b["info"][3] == 1 and np.array_equal(l3, l1) and np.array_equal(l1, listed[sel])
        why = b["lc_why"]
        assert int(why[0]) + int(why[-1]) == int(left1.sum()), "k_local_cluster did not walk the pair pass's leftover"
        assert np.array_equal(f3, f1 | ((flag[sel] == 1) & left1))
        assert np.array_equal(p["pair_mid"], b["pair_mid"]) and not p["pair_mid"][:2].any()
        print(c, "pair pass decides", int(f1.sum()), "of", int(l1.sum()), "then k_local_cluster", int((f3 & ~f1).sum()), "pair_mid", p["pair_mid"].tolist())
        assert not [i for i, x in zip(sel, f3) if x and T.flag[i] != 1]


@pytest.mark.parametrize("n_list", (0, 1, 3, 4, 5, 8, 9, 1000))
def test_batch_geometry(S, T, G, grouped, n_list):
    """the ticket draws four reads at a time: lists of every length around that, built by repeating table reads, with reads off the list between"""
    idx, ctx = G
    flag, listed, _, _ = grouped
    rng = np.random.default_rng(n_list)
    on = [i for i in T.of(0) if listed[i] and T.outcome(i) != M.SCORE_TIE]
    off = [i for i in T.of(0) if not listed[i]]
    pick = list(rng.choice(on, n_list)) + list(rng.choice(off, 1 + n_list // 7))
    pick = [pick[j] for j in rng.permutation(len(pick))]
    rc, out = shortcuts(S, ctx[0], [T.reads[i].seq for i in pick], 2)
    S.check(rc)
    l, f, _ = check_partition(out, len(pick))
    assert int(l.sum()) == n_list and np.array_equal(l, listed[pick]) and np.array_equal(f, flag[pick] == 1)
    assert np.array_equal(out["lc_why"], model_hist([T.model[i] for i in pick]))


MODES = {"plain": {}, "no_lemma": {"SCRUBBY_HIP_NO_LEMMA": "1"}, "no_local_cluster": {"SCRUBBY_HIP_DBG": "256"}, "stats": {"SCRUBBY_HIP_DBG": "16"}}


@pytest.mark.parametrize("mode", list(MODES))
def test_classify_level(S, T, G, mode, monkeypatch):
    """the table through the whole classify path: the oracle's flags whatever the switches; with the statistics on, the reads decided although
    a seed of theirs is filtered are counted, and are the model's"""
    idx, ctx = G
    for name, v in MODES[mode].items():
        monkeypatch.setenv(name, v)
    for c in (0, 1):
        sel = T.of(c)
        bases, offs = T_.batch([T.reads[i].seq for i in sel])
        gf, _, st, rc = idx[c].classify(bases, offs, want_trace=False)
        print(mode, c, {k: st[k] for k in ("n_chain_small", "n_chain_large", "n_pair_decided", "n_ext_shortcut", "n_lc_filtered", "n_ext_reads")})
        assert rc == 0
        bad = np.where(gf != T.flag[sel])[0]
        assert len(bad) == 0, f"{mode}: {len(bad)} flags differ from the oracle's, first {[(T.reads[sel[j]].family, T.reads[sel[j]].sweep, T.reads[sel[j]].step) for j in bad[:5]]}"
        if mode == "stats":
            assert st["n_lc_filtered"] == sum(T.outcome(i) == M.DECIDED_FILTERED for i in sel)
        else:
            assert st["n_lc_filtered"] == 0


def test_refusals(S, T, G, monkeypatch):
    idx, ctx = G
    seqs = [T.reads[i].seq for i in T.of(0)[:64]]
    untouched = lambda out: (out["route"] == 0xEE).all() and (out["flags"] == 0xEE).all() and (out["info"] == -1).all()
    for mask in (-1, 4):
        rc, out = shortcuts(S, ctx[0], seqs, mask)
        assert rc == BAD_ARG and untouched(out)
    rc, out = shortcuts(S, ctx[0], seqs, 2, trace=C.c_void_p(64))      # trace mode has no shortcuts: refused before anything is read
    assert rc == BAD_ARG and untouched(out)
    rc, out = shortcuts(S, ctx[0], [], 2)
    assert rc == BAD_ARG and untouched(out)
    rc, out = shortcuts(S, ctx[0], [b"A" * (MAX_LEN + 1)] + seqs, 2)
    assert rc == BAD_ARG and untouched(out)
    monkeypatch.setenv("SCRUBBY_HIP_ARENA_MB", "96")
    # no extension stage; premises of ext_lemma not met (a * k < min_dp_max); a long-read context
    plain, weak = gpu_opts(S, 0), gpu_opts(S, 0)
    plain.flags = 0
    weak.min_dp_max = 1000
    for o in (plain, weak):
        idx[0].opts, keep = o, idx[0].opts
        try:
            c2 = S.Context(idx[0], 256, 100_000, MAX_LEN)
        finally:
            idx[0].opts = keep
        rc, out = shortcuts(S, c2, seqs, 2)
        c2.close()
        assert rc == BAD_ARG and untouched(out)
    lo = S.preset("map-ont")
    lidx = S.Index.build([T.contigs[1][0][:50_000].tobytes()], lo)
    c3 = S.Context(lidx, 256, 100_000, MAX_LEN)
    rc, out = shortcuts(S, c3, seqs, 2)
    c3.close(); lidx.close()
    assert rc == BAD_ARG and untouched(out)
    # ext_lemma off by switch: taken, the mask's bit 1 finds no kernel to run, the list is left over whole
    monkeypatch.setenv("SCRUBBY_HIP_NO_LEMMA", "1")
    c4 = S.Context(idx[0], 256, 100_000, MAX_LEN)
    monkeypatch.delenv("SCRUBBY_HIP_NO_LEMMA")
    rc, out = shortcuts(S, c4, seqs, 2)
    c4.close()
    S.check(rc)
    l, f, left = check_partition(out, len(seqs), lc_ran=False)
    assert out["info"][3] == 0 and not f.any() and np.array_equal(left, l) and l.any() and not out["lc_why"].any()
