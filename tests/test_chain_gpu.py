"""The chaining DP and backtrack variants of csrc/sh_chain.h, called directly (sh_dbg_chain, csrc/sh_dbg_chain.hip) on the case table of
tests/chain_cases.py: seven implementations of mg_lchain_dp and six ways to run mg_chain_backtrack against the oracle's arrays
(mmo_chain_arrays), and - where a variant may decline or leave work to the sequential code - against what the plain model
(tests/chain_ref.py) says it must do.  Integers only: there is no tolerance anywhere.  Two launches' worth of cases are shared by all tests."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests import chain_cases as K
from tests import chain_ref as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
G_MIN = 32768      # the product's threshold for eight lanes an anchor (K3Args::pft_gmin)


class ChainCase(C.Structure):
    _fields_ = [("off", C.c_uint64)] + [(n, C.c_int32) for n in
                ("n", "qlen", "dp", "bt", "g_min", "first_only", "top_cap", "pad", "k", "is_sr", "min_cnt", "min_sc", "max_gap", "max_gap_ref",
                 "max_frag_len", "bw", "max_skip", "max_iter")] + [("chain_gap_scale", C.c_float), ("chain_skip_scale", C.c_float)]


class ChainResult(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("ret", "bt_ret", "n_u", "best", "n_emit", "pad")]


def _ints(a):
    return [int(v) for v in a]


class Batch:
    """cases for one call of sh_dbg_chain"""

    def __init__(self):
        self.x, self.q, self.n_total, self.entries = [], [], 0, []

    def anchors(self, x, q):
        off = self.n_total
        self.x.append(np.asarray(x, np.uint64)); self.q.append(np.asarray(q, np.uint32)); self.n_total += len(x)
        return off

    def add(self, off, n, qlen, o, dp="none", bt="none", f_in=None, p_in=None, g_min=G_MIN, first_only=False, top_cap=K.TOPBT_MAX):
        self.entries.append((off, n, qlen, o, K.DP_CODE[dp], K.BT_CODE[bt], f_in, p_in, g_min, int(first_only), top_cap))
        return len(self.entries) - 1

    def call(self):
        from scrubby_amd import lib as S
        L = S.require_gpu()
        x, q = np.concatenate(self.x), np.concatenate(self.q)
        arr = (ChainCase * len(self.entries))()
        outs, tot = [], 0
        for i, (off, n, qlen, o, dp, bt, f_in, p_in, g_min, first_only, top_cap) in enumerate(self.entries):
            c = arr[i]
            c.off, c.n, c.qlen, c.dp, c.bt, c.g_min, c.first_only, c.top_cap = off, n, qlen, dp, bt, g_min, first_only, top_cap
            c.k, c.is_sr, c.min_cnt, c.min_sc, c.max_gap, c.max_gap_ref, c.max_frag_len = o.k, o.is_sr, o.min_cnt, o.min_sc, o.max_gap, o.max_gap_ref, o.max_frag_len
            c.bw, c.max_skip, c.max_iter, c.chain_gap_scale, c.chain_skip_scale = o.bw, o.max_skip, o.max_iter, o.gap_scale, o.skip_scale
            outs.append(tot); tot += n
        f_in, p_in = np.zeros(tot, np.int32), np.full(tot, -1, np.int32)
        for at, e in zip(outs, self.entries):
            if e[6] is not None:
                f_in[at:at + e[1]] = e[6]; p_in[at:at + e[1]] = e[7]
        res = (ChainResult * len(self.entries))()
        f, p, t, ch = np.zeros(tot, np.int32), np.zeros(tot, np.int32), np.zeros(tot, np.int32), np.zeros(5 * tot, np.int32)
        rc = L.sh_dbg_chain(0, x.ctypes.data, q.ctypes.data, len(x), C.cast(arr, C.c_void_p), len(self.entries), f_in.ctypes.data, p_in.ctypes.data,
                            C.cast(res, C.c_void_p), f.ctypes.data, p.ctypes.data, t.ctypes.data, ch.ctypes.data)
        return rc, outs, res, f, p, t, ch

    def run(self):
        from scrubby_amd import lib as S
        rc, outs, res, f, p, t, ch = self.call()
        S.check(rc)
        out = []
        for at, e, r in zip(outs, self.entries, res):
            n = e[1]
            assert 0 <= r.n_emit <= n
            out.append({"ret": int(r.ret), "bt_ret": int(r.bt_ret), "n_u": int(r.n_u), "best": int(r.best), "f": f[at:at + n], "p": p[at:at + n], "t": t[at:at + n],
                        "chains": [tuple(int(v) for v in ch[5 * at + 5 * c:5 * at + 5 * c + 5]) for c in range(r.n_emit)]})
        return out


def _marked(c):
    starts = R.cluster_starts(c["o"], c["qlen"], _ints(c["x"]))
    return c["q"] | (np.array(starts, np.uint32) << np.uint32(31))


# ---- the references, once ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def want(oracle):
    """per case: the oracle's (f, p, chains)"""
    return {c["name"]: K.oracle_case(oracle, c) for c in K.table()}


@pytest.fixture(scope="module")
def models(oracle):
    return {c["name"]: K.model_case(oracle, c) for c in K.table()}


@pytest.fixture(scope="module")
def states(oracle, want):
    """every DP state the backtracks run over: (name, options, f, p, the oracle's chains), from the table and by hand"""
    S = [(c["name"], c["o"], want[c["name"]][0], want[c["name"]][1], want[c["name"]][2]) for c in K.table()]
    S += [(b["name"], b["o"], b["f"], b["p"], oracle.backtrack_arrays(K.oracle_opts(oracle, b["o"]), b["f"], b["p"])) for b in K.bt_table()]
    return S


@pytest.fixture(scope="module")
def visits(states):
    """the model's backtrack over every state: (chains, t, visits)"""
    return {name: R.backtrack(o, _ints(f), _ints(p)) for name, o, f, p, _ in states}


# ---- launch 1: every DP variant on every case it takes ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dp_device():
    B, idx = Batch(), {}
    for c in K.table():
        n = len(c["x"])
        off = B.anchors(c["x"], _marked(c))
        for v in K.DP_VARIANTS:
            if not K.takes(v, n, c["qlen"], c["o"], c["groups"]):
                continue
            if v == "small":
                order = K.shuffled(c)
                idx[c["name"], v] = B.add(B.anchors(c["x"][order], c["q"][order]), n, c["qlen"], c["o"], dp=v)
            elif v == "pf_tiled":
                idx[c["name"], v] = B.add(off, n, c["qlen"], c["o"], dp=v)
                idx[c["name"], "pf_tiled8"] = B.add(off, n, c["qlen"], c["o"], dp=v, g_min=1)
            else:
                idx[c["name"], v] = B.add(off, n, c["qlen"], c["o"], dp=v)
    out = B.run()
    return {key: out[i] for key, i in idx.items()}


@pytest.mark.parametrize("variant", ["seq", "mask", "small", "wave", "ring"])
def test_dp_variant_is_identical_to_the_oracle(variant, dp_device, want, oracle):
    bad, n_cases = [], 0
    for c in K.table():
        got = dp_device.get((c["name"], variant))
        if got is None:
            continue
        n_cases += 1
        f, p, _ = want[c["name"]]
        if not (np.array_equal(got["f"], f) and np.array_equal(got["p"], p)) or got["ret"] != 0:
            bad.append(c["name"])
            continue
        t, n = got["t"], len(f)
        if variant == "seq":          # the sequential code leaves mg_lchain_dp's own marks: t[j] = the last anchor whose scan marked j
            _, _, _, marks = R.chain_dp(oracle.lib(), c["o"], c["qlen"], _ints(c["x"]), _ints(c["q"])) if n <= 600 else (0, 0, 0, None)
            ok = marks is None or _ints(t) == marks
        elif variant == "wave":       # a mark may be one the sequential scan would not have set (a lane past the break point), but it is always a true one:
            ok = all(t[j] == 0 or (j < t[j] < n and any(p[jj] == j for jj in range(j + 1, int(t[j])))) for j in range(n) if n <= 600)      # j precedes an anchor before t[j]
        elif variant in ("mask", "ring"):      # marks in a register / in LDS: t in memory stays as it was handed over, zero
            ok = not t.any()
        else:
            ok = True                 # SmallStore: the t byte holds what sorting left there and nothing reads it
        if not ok:
            bad.append(c["name"] + ":t")
    assert not bad and n_cases >= 70, (variant, n_cases, bad)


def _clusters(starts):
    where = [i for i, s in enumerate(starts) if s] + [len(starts)]
    return list(zip(where[:-1], where[1:]))


def test_par_fill_block(dp_device, want, models):
    bad, n_true, n_cmp = [], 0, 0
    for c in K.table():
        got, (f, p, _) = dp_device[c["name"], "pf_block"], want[c["name"]]
        applies, dirty, starts = R.par_fill_model(c["o"], c["qlen"], _ints(c["x"]), _ints(c["q"]), models[c["name"]].events)
        if bool(got["ret"]) != applies:
            bad.append(c["name"] + ":ret")
        if not (applies and got["ret"]):
            continue      # nothing usable was written
        n_true += 1
        if {a for a, _ in _clusters(starts) if got["t"][a] == K.PF_DIRTY} != dirty or set(np.unique(got["t"]).tolist()) - {0, K.PF_DIRTY}:
            bad.append(c["name"] + ":dirty")
        for a, b in _clusters(starts):
            if a not in dirty:
                n_cmp += b - a
                if not (np.array_equal(got["f"][a:b], f[a:b]) and np.array_equal(got["p"][a:b], p[a:b])):
                    bad.append(f"{c['name']}:{a}")
    assert not bad and n_true >= 100 and n_cmp >= 20000, (n_true, n_cmp, bad)


@pytest.mark.parametrize("lanes", ["pf_tiled", "pf_tiled8"])
def test_par_fill_tiled(lanes, dp_device, want, models):
    bad, n_true, n_cmp, n_must, n_low = [], 0, 0, 0, 0
    for c in K.table():
        got = dp_device.get((c["name"], lanes))
        if got is None:
            continue
        f, p, _ = want[c["name"]]
        if c["o"].max_iter < K.PFT_H:      # the halo stands in for the max_iter cut: below PFT_H the tiled fill declines, whatever the read
            n_low += 1
            if got["ret"]:
                bad.append(c["name"] + ":max_iter")
            continue
        ev = models[c["name"]].events
        applies, dirty, starts = R.par_fill_model(c["o"], c["qlen"], _ints(c["x"]), _ints(c["q"]), ev)
        # the tiled fill also leaves to the sequential code an anchor with PFT_H anchors or more in its window, and one whose scan runs out of
        # the halo; the caps are the block fill's, counted per tile.  So only a read of one tile whose windows all stay below PFT_H (and
        # tile_bounds, built so) must behave exactly as the model says.
        exact = (len(f) <= K.PFT_T and max(i - e.st for i, e in enumerate(ev)) < K.PFT_H) or c["name"] == "tile_bounds"
        if exact and bool(got["ret"]) != applies:
            bad.append(c["name"] + ":ret")
        if not got["ret"]:
            continue
        n_true += 1
        marked = {a for a, _ in _clusters(starts) if got["t"][a] == K.PF_DIRTY}
        if not dirty <= marked or set(np.unique(got["t"]).tolist()) - {0, K.PF_DIRTY}:
            bad.append(c["name"] + ":dirty")
        if exact and marked != dirty:      # among them the families built clean: nothing dirty
            bad.append(c["name"] + ":clean")
        if exact:
            n_must += sum(b - a for a, b in _clusters(starts) if a not in dirty)
        for a, b in _clusters(starts):
            if a not in marked:
                n_cmp += b - a
                if not (np.array_equal(got["f"][a:b], f[a:b]) and np.array_equal(got["p"][a:b], p[a:b])):
                    bad.append(f"{c['name']}:{a}")
    # n_must: the anchors of the clusters the model says must come out clean, in the reads where the tiled fill has no reason of its own to
    # mark more (tile_bounds' 12611 among them); all of them are compared with the oracle
    assert not bad and n_true >= 100 and n_cmp >= n_must >= 15000 and n_low == 6, (lanes, n_true, n_cmp, n_must, n_low, bad)


# ---- launch 2: every backtrack over the oracle's f / p and over its own DP's ------------------------------------------------------------------
OWN_DP = {"small": "seq", "mask": "mask", "heap": "ring", "wave_top": "wave", "quick": "ring", "block_top": "pf_block"}


@pytest.fixture(scope="module")
def bt_device(states, models):
    B, idx = Batch(), {}
    table = {c["name"]: c for c in K.table()}
    for name, o, f, p, _ in states:
        n = len(f)
        c = table.get(name)
        if c is not None:
            off, qlen = B.anchors(c["x"], _marked(c)), c["qlen"]
        else:      # a state by hand: the backtracks read no anchors
            off, qlen = B.anchors(np.arange(n, dtype=np.uint64) + 1000, np.zeros(n, np.uint32) | np.uint32(1 << 31)), 1024
        for v in K.BT_VARIANTS:
            if not K.bt_takes(v, n):
                continue
            idx[name, v, "oracle"] = B.add(off, n, qlen, o, bt=v, f_in=f, p_in=p)
            if v in ("small", "mask", "heap"):
                idx[name, v, "first"] = B.add(off, n, qlen, o, bt=v, f_in=f, p_in=p, first_only=True)
            if c is None:
                continue
            dp = OWN_DP[v]
            if not K.takes(dp, n, qlen, o, c["groups"]):
                continue
            if dp == "pf_block":      # only where the fill leaves nothing to the sequential code
                applies, dirty, _ = R.par_fill_model(o, qlen, _ints(c["x"]), _ints(c["q"]), models[name].events)
                if not applies or dirty:
                    continue
            idx[name, v, "own"] = B.add(off, n, qlen, o, dp=dp, bt=v)
        if c is not None and K.takes("small", n, qlen, o, c["groups"]):      # k_chain_small's pair: the SmallStore's DP, backtrack_mask over it
            order = K.shuffled(c)
            idx[name, "mask", "small"] = B.add(B.anchors(c["x"][order], c["q"][order]), n, qlen, o, dp="small", bt="mask")
        if K.bt_takes("block_top", n):      # a cap of its own: one candidate, and as many as the first chain's score admits less one
            idx[name, "block_top", "cap1"] = B.add(off, n, qlen, o, bt="block_top", f_in=f, p_in=p, top_cap=1)
    out = B.run()
    return {key: out[i] for key, i in idx.items()}


@pytest.mark.parametrize("variant", ["small", "mask", "heap", "wave_top"])
def test_backtrack_gives_the_oracles_chains(variant, bt_device, states, visits):
    bad, n_run = [], 0
    for name, o, f, p, chains in states:
        for src in ("oracle", "own", "small"):
            got = bt_device.get((name, variant, src))
            if got is None:
                continue
            n_run += 1
            best = max([c[2] for c in chains], default=0)
            ok = got["n_u"] == len(chains) and got["best"] == best and np.array_equal(got["f"], f) and np.array_equal(got["p"], p)
            if variant != "small":      # backtrack_small takes no emitter
                ok = ok and got["chains"] == chains
            if variant != "mask":       # t = 1 on every anchor a walk took, kept or not (the mask variant keeps them in a register)
                ok = ok and _ints(got["t"]) == visits[name][1]
            if not ok:
                bad.append((name, src))
    assert not bad and n_run >= 150, (variant, n_run, bad)


@pytest.mark.parametrize("variant", ["small", "mask", "heap"])
def test_first_only_gives_the_first_accepted_chain(variant, bt_device, states):
    bad, n_run = [], 0
    for name, o, f, p, chains in states:
        got = bt_device.get((name, variant, "first"))
        if got is None:
            continue
        n_run += 1
        ok = got["n_u"] == min(1, len(chains)) and got["best"] == (chains[0][2] if chains else 0)
        if variant != "small":
            ok = ok and got["chains"] == chains[:1]
        if not ok:
            bad.append(name)
    assert not bad and n_run >= 100, (variant, n_run, bad)


def _block_top_wanted(o, f, chains, vis, cap):
    """(returns, chains): false when the first candidate's chain is rejected or more than cap anchors have f at or above its score"""
    if not vis:
        return True, []
    zi, accepted, _, _, score, _ = vis[0]
    if not accepted:
        return False, None
    if sum(int(v) >= score for v in f) > cap:
        return False, None
    return True, [c for c in chains if c[4] >= score]


def test_backtrack_block_top(bt_device, states, visits):
    bad, n_run, n_false, n_true = [], 0, 0, 0
    for name, o, f, p, chains in states:
        for src, cap in (("oracle", K.TOPBT_MAX), ("own", K.TOPBT_MAX), ("cap1", 1)):
            got = bt_device.get((name, "block_top", src))
            if got is None:
                continue
            n_run += 1
            ret, kept = _block_top_wanted(o, f, chains, visits[name][2], cap)
            n_false += not ret; n_true += ret
            if bool(got["bt_ret"]) != ret:
                bad.append((name, src, "ret"))
            elif ret and (got["chains"] != kept or got["n_u"] != len(kept) or got["best"] != max([c[2] for c in kept], default=0)):
                bad.append((name, src))
            elif not ret and (got["chains"] or got["t"].any()):      # nothing marked or handed over
                bad.append((name, src, "touched"))
    # both outcomes, each for each of its reasons (the counts only guard against a loop that has gone empty)
    B = {(name, src): bool(bt_device[name, "block_top", src]["bt_ret"]) for name, *_ in states for src in ("oracle", "cap1")}
    assert not B["first_rejected", "oracle"] and not B["top_65", "oracle"] and not B["top_70", "oracle"] and B["top_64", "oracle"] and B["none", "oracle"]
    assert not B["top_3", "cap1"] and B["cnt_2", "cap1"]
    assert not bad and n_run >= 400 and n_false >= 20 and n_true >= 200, (n_run, n_false, n_true, bad)


def test_first_chain_quick(bt_device, states, visits):
    bad, seen = [], set()
    for name, o, f, p, chains in states:
        for src in ("oracle", "own"):
            got = bt_device.get((name, "quick", src))
            if got is None:
                continue
            vis = visits[name][2]
            wanted = 0 if not vis else (1 if vis[0][1] else -1)
            seen.add(wanted)
            if got["bt_ret"] != wanted:
                bad.append((name, src, got["bt_ret"], wanted))
    assert not bad and seen == {0, 1, -1}, (seen, bad)


# ---- refusals and known answers ------------------------------------------------------------------------------------------------------------------
def test_what_a_variant_cannot_take_is_refused_before_any_launch():
    from scrubby_amd import lib as S
    S.require_gpu()
    def rc(n, qlen, o, q_hi=0, f_hi=None, **kw):
        B = Batch()
        x = np.arange(n, dtype=np.uint64) + 1000
        q = np.arange(n, dtype=np.uint32) % 1000
        q[-1] = max(q[-1], q_hi); q[0] |= np.uint32(1 << 31)
        f = np.full(n, 21, np.int32) if f_hi is None else np.full(n, f_hi, np.int32)
        B.add(B.anchors(x, q), n, qlen, o, f_in=f, p_in=np.full(n, -1, np.int32), **kw)
        return B.call()[0]
    BAD = 1
    assert S.STATUS_NAMES[BAD] == "SH_ERR_BAD_ARG"
    assert rc(64, 1024, K.SRW, dp="mask") == 0 and rc(65, 1024, K.SRW, dp="mask") == BAD and rc(65, 1024, K.SRW, bt="mask") == BAD
    assert rc(32, 1024, K.SRW, dp="small") == 0 and rc(33, 1024, K.SRW, dp="small") == BAD
    assert rc(8, 70000, K.SRW, q_hi=65535, dp="small") == 0 and rc(8, 70000, K.SRW, q_hi=65536, dp="small") == BAD
    assert rc(32, 1024, K.SRW._replace(k=2047), dp="small") == 0 and rc(32, 1024, K.SRW._replace(k=2048), dp="small") == BAD      # f <= k * n: beyond 16 bits
    assert rc(100, 1024, K.SRW._replace(max_iter=K.RING_TMAX_ITER), dp="ring") == 0 and rc(100, 1024, K.SRW._replace(max_iter=K.RING_TMAX_ITER + 1), dp="ring") == BAD
    assert rc(10, 1024, K.SRW, dp="wave", bt="block_top") == BAD and rc(10, 1024, K.SRW, dp="pf_block", bt="heap") == BAD and rc(10, 1024, K.SRW, dp="small", bt="heap") == BAD


def test_known_answers_on_the_device(dp_device, bt_device):
    kat = json.load(open(os.path.join(HERE, "golden", "chain_dp_kat.json")))["cases"]
    n_dp = n_bt = 0
    for e in kat:
        for v in ("seq", "mask", "small", "wave", "ring"):
            got = dp_device.get((e["name"], v))
            if got is not None:
                n_dp += 1
                assert _ints(got["f"]) == e["f"] and _ints(got["p"]) == e["p"], (e["name"], v)
        for v, src in (("mask", "own"), ("mask", "small"), ("heap", "own"), ("wave_top", "own")):
            got = bt_device.get((e["name"], v, src))
            if got is not None:
                n_bt += 1
                assert [list(c) for c in got["chains"]] == e["chains"], (e["name"], v, src)
    assert n_dp >= 90 and n_bt >= 60
