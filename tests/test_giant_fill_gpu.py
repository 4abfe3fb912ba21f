"""par_fill_tiled (csrc/sh_chain.h) where its tile holds q and f in 16 bits each, keeps the eight-lane split's cluster distances in p's slots
and takes a scan's predecessors B = 4 at a time: the shapes at which exactly those three can go wrong, through sh_dbg_chain against the
oracle's f and p the way tests/test_chain_gpu.py does it.  Integers only, no tolerance.

A scan of the tiled fill walks back from anchor i over the entries j with x_i - x_j <= min(max_dist_x, q_i + bw) and ends at the first
entry beyond that (`dist`), at a cluster start after taking it (`mark`), at the valid predecessor number max_skip + 1 (`skip`), or at index 0
of tile + halo (`out`).  scan_shape() below says which, after how many entries and with how many valid ones; the first test holds every
constructed case against it on the CPU, with the oracle's score alone, before the device is asked anything.
"""
import functools

import numpy as np
import pytest

from tests import chain_cases as K
from tests import chain_ref as R
from tests.test_chain_gpu import Batch, _clusters, _ints, _marked

B = 4                              # PFT_B: predecessors loaded per batch
SR = K.SR                          # k = 21, bw = 100, max_skip = 25
QLEN = 400                         # max_dist_x = max_dist_y = 400 under sr
R0, Q0 = 5000, 150                 # the anchor whose scan is built, in most cases: limit = min(400, Q0 + bw) = 250
Q_OFF = 300                        # a query position no anchor on the diagonal of (R0, Q0) links to or from: dq <= 0 or dd > bw


def scan_shape(L, o, qlen, x, q, starts, i):
    """(entries taken, valid among them, how the scan ended) for the tiled fill's scan of anchor i inside the first tile"""
    sc = R.Scorer(L, o, qlen)
    lim = min(sc.mdx, q[i] + o.bw)
    if starts[i]:
        return 0, 0, "start"
    taken = valid = 0
    for j in range(i - 1, -1, -1):
        if (x[i] & 0xffffffff) - (x[j] & 0xffffffff) > lim:
            return taken, valid, "dist"
        taken += 1
        if sc(x[i], q[i], x[j], q[j]) != R.NONE:
            valid += 1
            if valid > o.max_skip:
                return taken, valid, "skip"
        if starts[j]:
            return taken, valid, "mark"
    return taken, valid, "out"


def _entries(kinds, r0=R0, q0=Q0, q_off=Q_OFF):
    """the anchors at scan positions 1, 2, ... behind (r0, q0): 'v' on its diagonal (valid), 'i' one it cannot link to"""
    return [(r0 - s, q0 - s if kd == "v" else q_off) for s, kd in enumerate(kinds, 1)][::-1]


def _case(name, rq, want, qlen=QLEN, o=SR, group=None, at=-1, g_min=None, exact=True):
    """want: (entries, valid, end) of anchor `at`'s scan"""
    c = K._case(name, "giant_fill", o, qlen, rq, group)
    c.update(want=want, at=at % len(rq), g_min=g_min, exact=exact)
    return c


def _saw_read(n, spans, dense_at=None):
    """n anchors in clusters of short windows (chain_cases._saw): one cluster over each [a, b) of spans, clusters of 23 and a shorter one
    between them; at dense_at a dense diagonal of 30 (more than max_skip valid predecessors: dirty)"""
    rq, r = [], 1000
    def put(m, dense=False):
        nonlocal r
        rq.extend(K._diag(m, 1, r, 100) if dense else K._saw(m, r))
        r += 20 * m + 20000
    for a, b in sorted(spans + ([(dense_at, dense_at + 30)] if dense_at is not None else []) + [(n, n)]):
        a, b = min(a, n), min(b, n)
        while len(rq) < a:
            put(min(23, a - len(rq)))
        if b > a:
            put(b - a, a == dense_at)
    assert len(rq) == n
    return rq


W2 = K.SRW._replace(max_gap_ref=1000)      # max_dist_x = 1000: the model's windows stay short over these long reads


@functools.lru_cache(maxsize=None)
def table():
    T = []
    far = [(R0 - 251, Q_OFF)]      # one past the limit of (R0, Q0), within max_dist_x of what follows: the same cluster
    # windows of V valid predecessors, moved along the batch by s entries that are not
    for V in (0, 1, 3, 4, 5, 9):
        for s in range(B):
            T.append(_case(f"win_{V}_{s}", far + _entries("i" * s + "v" * V) + [(R0, Q0)], (s + V, V, "dist")))
    # the distance limit on entry e of a batch, and behind it four anchors on the diagonal that score if they are taken: q_i = 390, so the
    # limit is max_dist_x = 400 and an anchor 401 .. 404 back with dq 380 .. 383 is within the band
    for e in range(1, B + 1):
        for full in (1, 2):
            m = B * full + e - 1
            beyond = [(R0 - 404 + t, 7 + t) for t in range(4)]
            T.append(_case(f"dist_{e}_{full}", beyond + _entries("vi" * 6, q0=390, q_off=395)[12 - m:] + [(R0, 390)], (m, (m + 1) // 2, "dist")))
    # a cluster start on entry e of a batch; before it, on another strand, anchors of the same diagonal a few bases back: loaded, never taken
    for e in range(1, B + 1):
        for full in (0, 1):
            m = B * full + e
            other = [(R0 - m - 6 + t, Q0 - m - 6 + t) for t in range(6)]
            T.append(_case(f"mark_{e}_{full}", other + _entries("v" * m) + [(R0, Q0)], (m, m, "mark"), group=[0] * 6 + [1] * (m + 1)))
    # valid predecessor 25, 26 and 27 on each entry of a batch: 26 makes the cluster dirty
    for V in (24, 25, 26, 27):
        for s in range(B):
            got = (s + min(V, 26), min(V, 26), "skip" if V >= 26 else "dist")
            T.append(_case(f"skip_{V}_{s}", far + _entries("i" * s + "v" * V) + [(R0, Q0)], got))
    # a window that ends at index 0 of the first tile
    for n in range(1, 10):
        T.append(_case(f"first_{n}", K._diag(n, 1, 1000, 100), (n - 1, n - 1, "mark" if n > 1 else "start")))
    # 16 bits of q and f: qlen = 1024, q = 1023 with and without the mark, and f = k + 1023 at the end of one chain over the whole query
    # (128 ranks: a first step of 15, then 126 of 8)
    W = K.SRW
    whole = [(1000, 0)] + [(1015 + 8 * t, 15 + 8 * t) for t in range(127)]
    T.append(_case("q1023", [(1000, 1023), (9000, 1015), (9008, 1023)], (1, 1, "mark"), qlen=1024, o=W))
    T.append(_case("whole_query", whole, (127, 127, "mark"), qlen=1024, o=W._replace(max_skip=200)))
    T.append(_case("k_fits", whole, (127, 127, "mark"), qlen=1024, o=W._replace(k=65535 - 1024, max_skip=200)))
    T.append(_case("k_declines", whole, (127, 127, "mark"), qlen=1024, o=W._replace(k=65535 - 1023, max_skip=200)))
    # dcs in p's slots (eight lanes per anchor): clusters that start at a tile's first anchor (4096), inside its halo (3840 .. 4095) and before
    # it, each running on into the tile where it can; a dirty cluster in every read
    for n, spans in ((4097, [(3900, 4096), (4096, 4097)]), (4352, [(3950, 4352)]), (4353, [(3700, 4353)]), (8193, [(3950, 4300), (7800, 8193)])):
        T.append(_case(f"dcs_{n}", _saw_read(n, spans, dense_at=3000), None, qlen=1024, o=W2, g_min=1, exact=False))
    # a cluster that starts exactly at index 0 of the second tile's halo (3840), and one an anchor before it, 4096 + 256 + 1 .. 9 anchors
    for m in range(1, 10):
        for s0 in (3840, 3839):
            rq = _saw_read(4352 + m, [(s0, 4352 + m)])
            for g_min in (None, 1):
                T.append(_case(f"halo_{m}_{s0}_{g_min or 0}", rq, None, qlen=1024, o=W2, g_min=g_min, exact=False))
    return T


_MODEL = {}


def _want_fp(oracle, c):
    """the oracle's f and p.  Its anchors carry k in 8 bits, so for k_fits they are written down instead: every link of `whole` has dd = 0 and
    dg = dq <= 15 <= k, which scores dq without a penalty, so f_i = k + q_i from every predecessor alike and p_i is the nearest one"""
    if c["name"] == "k_fits":
        return c["o"].k + c["q"].astype(np.int32), np.arange(len(c["q"]), dtype=np.int32) - 1
    f, p, _ = K.oracle_case(oracle, c)
    return f, p


def _model(oracle, c):
    if c["name"] not in _MODEL:
        x, q = _ints(c["x"]), _ints(c["q"])
        f, p, ev, _ = R.chain_dp(oracle.lib(), c["o"], c["qlen"], x, q)
        _MODEL[c["name"]] = (x, q, ev, R.par_fill_model(c["o"], c["qlen"], x, q, ev))
    return _MODEL[c["name"]]


def test_the_cases_are_what_they_are_meant_to_be(oracle):
    L = oracle.lib()
    seen = set()
    for c in table():
        x, q, ev, (applies, dirty, starts) = _model(oracle, c)
        assert applies, c["name"]
        if c["want"] is not None:
            got = scan_shape(L, c["o"], c["qlen"], x, q, starts, c["at"])
            assert got == c["want"], (c["name"], got)
            seen.add((got[2], got[0] % B))
            if c["name"].startswith(("win_", "skip_")):      # what the model counts over the whole window agrees
                assert min(ev[c["at"]].n_valid, 26) == got[1], c["name"]
        name = c["name"]
        if name.startswith("skip_"):
            assert bool(dirty) == (int(name.split("_")[1]) >= 26), name
        elif name.startswith("dcs_"):
            assert dirty == {3000}, name
        elif name.startswith("halo_"):
            assert not dirty and starts[int(name.split("_")[2])] and not any(starts[int(name.split("_")[2]) + 1:]), name
        else:
            assert not dirty, name
    # every exit on every entry of a batch
    assert {(end, e) for end in ("dist", "mark", "skip") for e in range(B)} <= seen
    f, _, _ = K.oracle_case(oracle, next(c for c in table() if c["name"] == "whole_query"))
    assert int(f.max()) == 21 + 1023
    f, _ = _want_fp(oracle, next(c for c in table() if c["name"] == "k_fits"))
    assert int(f.max()) == 65534


@pytest.fixture(scope="module")
def device():
    bt, idx = Batch(), {}
    for c in table():
        off = bt.anchors(c["x"], _marked(c))
        idx[c["name"]] = bt.add(off, len(c["x"]), c["qlen"], c["o"], dp="pf_tiled", **({} if c["g_min"] is None else {"g_min": c["g_min"]}))
        if c["want"] is not None:      # the small cases also with eight lanes per anchor
            idx[c["name"], 8] = bt.add(off, len(c["x"]), c["qlen"], c["o"], dp="pf_tiled", g_min=1)
    out = bt.run()
    return {key: out[i] for key, i in idx.items()}


def _check(oracle, device, names):
    bad, n_cmp = [], 0
    for c in table():
        if not c["name"].startswith(names):
            continue
        f, p = _want_fp(oracle, c)
        _, _, _, (applies, dirty, starts) = _model(oracle, c)
        for key in (c["name"], (c["name"], 8)):
            got = device.get(key)
            if got is None:
                continue
            if not got["ret"]:
                bad.append((key, "declined"))
                continue
            marked = {a for a, _ in _clusters(starts) if got["t"][a] == K.PF_DIRTY}
            if not dirty <= marked or set(np.unique(got["t"]).tolist()) - {0, K.PF_DIRTY}:
                bad.append((key, "dirty"))
            if c["exact"] and marked != dirty:
                bad.append((key, "clean"))
            for a, b in _clusters(starts):
                if a not in marked:
                    n_cmp += b - a
                    if not (np.array_equal(got["f"][a:b], f[a:b]) and np.array_equal(got["p"][a:b], p[a:b])):
                        bad.append((key, a))
    assert not bad, bad
    return n_cmp


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["win_", "dist_", "mark_", "skip_", "first_"])
def test_batch_edges(family, oracle, device):
    assert _check(oracle, device, (family,)) >= 40


@pytest.mark.gpu
def test_sixteen_bit_fields(oracle, device):
    assert _check(oracle, device, ("q1023", "whole_query", "k_fits")) >= 2 * (3 + 128 + 128)
    assert device["k_fits"]["ret"] == 1 and int(device["k_fits"]["f"].max()) == 65534
    assert device["k_declines"]["ret"] == 0 and device["k_declines", 8]["ret"] == 0      # nothing to compare: nothing usable was written


@pytest.mark.gpu
def test_cluster_distances_in_the_slots_of_p(oracle, device):
    assert _check(oracle, device, ("dcs_",)) >= 4097 + 4352 + 4353 + 8193 - 4 * 200


@pytest.mark.gpu
def test_clusters_at_the_first_index_of_the_halo(oracle, device):
    n_cmp = _check(oracle, device, ("halo_",))
    # a cluster that starts at the halo's first index is seen whole; one that starts an anchor earlier is not, and may be left to the
    # sequential code - but only that one
    for c in table():
        if c["name"].startswith("halo_"):
            got, s0 = device[c["name"]], int(c["name"].split("_")[2])
            marked = {a for a in range(len(c["x"])) if got["t"][a] == K.PF_DIRTY}
            assert marked <= ({s0} if s0 == 3839 else set()), c["name"]
    assert n_cmp >= 36 * 3800
