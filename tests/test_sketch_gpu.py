"""The front of the pipeline, seen directly: the three minimizer state machines of csrc/sh_sketch.h (sh_dbg_sketch) and the real front-end
kernels - k_sketch_probe, k_long_sketch / k_long_probe - run alone on a context (sh_dbg_front_end), on the case table of
tests/sketch_cases.py, against the oracle's mmo_sketch and a numpy lookup in the exported index.  The reference sketch's segment seams go
through the index dump.  Integers only, bit for bit: there is no tolerance anywhere."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests import sketch_cases as K

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
STATE, PACKED, DYN = 0, 1, 2
FORM_NAME = {STATE: "SketchState", PACKED: "SketchPacked", DYN: "SketchStateDyn"}
ROUTE_NONE, ROUTE_SMALL, ROUTE_BIG, ROUTE_RESKETCH = 0, 1, 2, 4
K2_CAP = 32              # anchors a read may give and still be chained in LDS (work_small)
SLOT_EMPTY, SLOT_MULTI, SLOT_KEYMASK, SLOT_NMASK = (1 << 64) - 1, 1 << 63, (1 << 56) - 1, (1 << 28) - 1
BAD_ARG = 1


# ---- sh_dbg_sketch ------------------------------------------------------------------------------------------------------------------------
def dbg_sketch(seqs, w, k, form):
    """-> (status, hash, y, count, at): the pushes of sequence i are hash / y [at[i] : at[i] + count[i]] (room for len + 1)"""
    from scrubby_amd import lib as S
    L = S.require_gpu()
    lens = np.array([len(s) for s in seqs], np.uint64)
    off = np.concatenate(([0], np.cumsum(lens))).astype(np.uint64)
    bases = np.frombuffer(b"".join(seqs) + b"\0", np.uint8).copy()
    n_out = int(off[-1]) + len(seqs)
    h, y, cnt = np.full(n_out, 0xA5A5A5A5A5A5A5A5, np.uint64), np.full(n_out, 0xA5A5A5A5, np.uint32), np.full(len(seqs), -7, np.int32)
    rc = L.sh_dbg_sketch(0, bases.ctypes.data, off.ctypes.data, len(seqs), w, k, form, h.ctypes.data, y.ctypes.data, cnt.ctypes.data)
    return rc, h, y, cnt, off[:-1].astype(np.int64) + np.arange(len(seqs))


def check_against(seqs, names, want, w, k, form):
    """one launch of one form over seqs; want[i] = the oracle's (hash, y)"""
    from scrubby_amd import lib as S
    rc, h, y, cnt, at = dbg_sketch(seqs, w, k, form)
    S.check(rc)
    got = []
    for i, (wh, wy) in enumerate(want):
        n = int(cnt[i])
        assert 0 <= n <= len(seqs[i]) + 1, (FORM_NAME[form], w, k, names[i], n)
        gh, gy = h[at[i]:at[i] + n], y[at[i]:at[i] + n]
        if n != len(wh) or not np.array_equal(gh, wh) or not np.array_equal(gy, wy):
            d = next((j for j in range(min(n, len(wh))) if gh[j] != wh[j] or gy[j] != wy[j]), min(n, len(wh)))
            pytest.fail(f"{FORM_NAME[form]} w={w} k={k} {names[i]}: {n} minimizers, the oracle has {len(wh)}; first difference at {d}: "
                        f"{[(int(a), int(b) >> 1, int(b) & 1) for a, b in zip(gh[d:d + 3], gy[d:d + 3])]} != "
                        f"{[(int(a), int(b) >> 1, int(b) & 1) for a, b in zip(wh[d:d + 3], wy[d:d + 3])]}")
        got.append((gh, gy))
    return got


@pytest.mark.parametrize("w", K.WS)
def test_every_form_equals_the_oracle_on_the_table(oracle, w):
    for k in K.KS + (K.K_WIDE,):
        cases = K.sequences(w, k) + K.seam_reads(w, k)
        names, seqs = [n for n, _ in cases], [s for _, s in cases]
        want = [K.oracle_sketch(oracle, s, w, k) for s in seqs]
        got = {f: check_against(seqs, names, want, w, k, f) for f in ((STATE, DYN) if k > 23 else (STATE, PACKED, DYN))}
        # the forms then equal each other; said directly, so that a failure names the odd one out
        for f in got:
            for i, name in enumerate(names):
                assert np.array_equal(got[f][i][0], got[STATE][i][0]) and np.array_equal(got[f][i][1], got[STATE][i][1]), (FORM_NAME[f], w, k, name)


def test_known_answers_on_the_device(oracle):
    kat = json.load(open(os.path.join(HERE, "golden", "sketch_kat.json")))["cases"]
    cases = [(c["seq"].encode(), c["w"], c["k"], [tuple(m) for m in c["minimizers"]]) for c in kat]
    cases.append((K.KAT_SEQ, K.KAT_W, K.KAT_K, K.KAT_MINIMIZERS))
    for seq, w, k, want in cases:
        for form in (STATE, PACKED, DYN):
            rc, h, y, cnt, at = dbg_sketch([seq], w, k, form)
            assert rc == 0
            got = [(int(a), int(b) >> 1, int(b) & 1) for a, b in zip(h[:cnt[0]], y[:cnt[0]])]
            assert got == want, (FORM_NAME[form], w, k, seq)


@pytest.mark.parametrize("w", K.WS)
def test_position_independence(oracle, w):
    """A tie cluster and an N behind 0 .. W + 1 extra leading bases: every event moves through every ring slot, and the minimizers at positions
    from w + k on of the original, shifted back, do not depend on the prefix."""
    for k in (7, 21):
        rng = np.random.default_rng([31, w, k])
        core = (K.rand_seq(rng, w + k + 3) + K.tandem(rng, 3, w + k + 5) + K.rand_seq(rng, 4) + b"N" + K.tandem(rng, 2, w + k + 4, 1)
                + K.rand_seq(rng, w + k) + K.tandem(rng, w - 1, 3 * w + k) + K.rand_seq(rng, 11))
        assert K.has_window_tie(core, w, k)
        pre = K.rand_seq(rng, w + 1)
        seqs = [pre[len(pre) - p:] + core for p in range(w + 2)]
        names = [f"prefix_{p}" for p in range(w + 2)]
        want = [K.oracle_sketch(oracle, s, w, k) for s in seqs]
        for form in (STATE, PACKED, DYN):
            got = check_against(seqs, names, want, w, k, form)
            tails = []
            for p, (h, y) in enumerate(got):
                keep = (y >> np.uint32(1)) >= p + w + k
                tails.append((h[keep].tolist(), (y[keep] - np.uint32(2 * p)).tolist()))
            assert len(tails[0][0]) > 6
            for p in range(1, w + 2):
                assert tails[p] == tails[0], (FORM_NAME[form], w, k, p)


def test_what_a_form_cannot_take_is_refused_before_any_launch():
    seq = b"ACGTTGCAAGGCTTAACGGATCGATTACGCGATATCGGCTAGCTAGGATC"
    bad = [(7, 15, STATE), (0, 15, DYN), (20, 15, PACKED),           # not an instantiated window
           (10, 16, STATE), (10, 14, PACKED), (11, 20, DYN),         # even k
           (10, 25, PACKED), (10, 29, STATE), (19, 29, DYN), (10, 0, STATE), (10, -1, DYN),
           (10, 15, 3), (10, 15, -1)]                                # no such form
    for w, k, form in bad:
        rc, h, y, cnt, _ = dbg_sketch([seq, seq], w, k, form)
        assert rc == BAD_ARG, (w, k, form)
        assert np.all(h == 0xA5A5A5A5A5A5A5A5) and np.all(y == 0xA5A5A5A5) and np.all(cnt == -7), (w, k, form)
    rc, h, y, cnt, _ = dbg_sketch([seq, b"A" * 1025], 10, 15, PACKED)       # the packed form holds positions of reads of at most 1024
    assert rc == BAD_ARG and np.all(cnt == -7)
    for form in (STATE, PACKED, DYN):
        assert dbg_sketch([seq, b"A" * 1024], 10, 15, form)[0] == 0
    assert dbg_sketch([seq, b"A" * 1025], 10, 27, STATE)[0] == 0


# ---- sh_dbg_front_end -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_arena():
    mp = pytest.MonkeyPatch()
    mp.setenv("SCRUBBY_HIP_ARENA_MB", "96")       # the chain arena is not what these tests are about
    yield
    mp.undo()


def make_opts(preset, w, k, mid_occ, q_occ_frac=None):
    from scrubby_amd import lib as S
    o = S.preset(preset)
    o.w, o.k, o.mid_occ, o.flags = w, k, mid_occ, 0      # flags: no extension stage, whose buffers the front end does not touch
    if q_occ_frac is not None:
        o.q_occ_frac = q_occ_frac
    return o


class Lookup:
    """the exported table as numpy: hash -> (payload word w1, occurrences)"""

    def __init__(self, oracle, idx, w, k):
        slots, pos = idx.export()
        w0, w1 = slots[0::2], slots[1::2]
        used = w0 != np.uint64(SLOT_EMPTY)
        key = w0[used] & np.uint64(SLOT_KEYMASK)
        order = np.argsort(key)
        self.key, self.w1 = key[order], w1[used][order]
        assert len(np.unique(self.key)) == len(self.key)
        multi = (w0[used][order] & np.uint64(SLOT_MULTI)) != 0
        in_table = np.where(multi, self.w1 & np.uint64(SLOT_NMASK), np.uint64(1))
        # the occurrence count of each hash as the oracle reads the same table
        dk, dc, _ = oracle.Index.wrap(slots, pos, w, k).dump()
        o2 = np.argsort(dk)
        assert np.array_equal(dk[o2], self.key) and np.array_equal(dc[o2].astype(np.uint64), in_table)
        self.occ = dc[o2].astype(np.uint32)

    def find(self, h):
        if len(self.key) == 0 or len(h) == 0:
            return np.zeros(len(h), bool), np.zeros(len(h), np.int64)
        i = np.minimum(np.searchsorted(self.key, h), len(self.key) - 1)
        return self.key[i] == h, i

    def records(self, h, y):
        """-> (hit mask, the seed records of the hits in order: x, y = payload, z = occurrences | PREV_SAME, w = qpos << 1 | strand)"""
        hit, i = self.find(h)
        same = np.concatenate(([False], h[1:] == h[:-1])) if len(h) else np.zeros(0, bool)
        rec = np.zeros((int(hit.sum()), 4), np.uint32)
        w1 = self.w1[i[hit]]
        rec[:, 0], rec[:, 1] = (w1 & np.uint64(0xffffffff)).astype(np.uint32), (w1 >> np.uint64(32)).astype(np.uint32)
        rec[:, 2] = self.occ[i[hit]] | (same[hit].astype(np.uint32) << np.uint32(30))
        rec[:, 3] = y[hit]
        return hit, rec, same


def front_end(ctx, reads, ptr_off=0, lead=5):
    """sh_dbg_front_end on `reads`: the base pointer sits ptr_off bytes past a 256-byte boundary, offsets[0] = lead, the last read ends
    exactly at n_bases, and what lies outside the reads is valid sequence that would change the answer if a kernel took it in."""
    import torch
    from scrubby_amd import lib as S
    L = S.require_gpu()
    n = len(reads)
    off = (np.concatenate(([0], np.cumsum([len(r) for r in reads]))) + lead).astype(np.int64)
    n_bases = int(off[-1])
    raw = b"C" * ptr_off + b"A" * lead + b"".join(reads) + b"ACGTTGCA" * 8
    d_buf = torch.from_numpy(np.frombuffer(raw, np.uint8).copy()).cuda()
    assert d_buf.data_ptr() % 256 == 0
    d_off = torch.from_numpy(off).cuda()
    torch.cuda.synchronize()
    cap = n_bases + 1
    k1info, route = np.zeros(n, np.uint32), np.full(n, 0xEE, np.uint8)
    rec_off, mz_off = np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.uint64)
    rec, mzh, mzy, info = np.zeros((cap, 4), np.uint32), np.zeros(cap, np.uint64), np.zeros(cap, np.uint32), np.zeros(5, np.int32)
    S.check(L.sh_dbg_front_end(ctx.h, C.c_void_p(d_buf.data_ptr() + ptr_off), C.c_void_p(d_off.data_ptr()), n, n_bases, k1info.ctypes.data,
                               route.ctypes.data, rec_off.ctypes.data, rec.ctypes.data, cap, mz_off.ctypes.data, mzh.ctypes.data, mzy.ctypes.data, cap,
                               info.ctypes.data))
    ro, mo = rec_off.astype(np.int64), mz_off.astype(np.int64)
    out = [{"k1info": int(k1info[r]), "route": int(route[r]), "rec": rec[ro[r]:ro[r + 1]], "mz": (mzh[mo[r]:mo[r + 1]], mzy[mo[r]:mo[r + 1]])} for r in range(n)]
    assert int((route == ROUTE_SMALL).sum()) == info[2] and int((route == ROUTE_BIG).sum()) == info[3] and int((route == ROUTE_RESKETCH).sum()) == info[4]
    return out, info


def differences(got, want, names, fields):
    bad = []
    for g, e, name in zip(got, want, names):
        for f in fields:
            same = (all(np.array_equal(a, b) for a, b in zip(g[f], e[f])) and len(g[f]) == len(e[f])) if f == "mz" else \
                   np.array_equal(g[f], e[f]) if f == "rec" else g[f] == e[f]
            if not same:
                bad.append((name, f, g[f] if f in ("k1info", "route") else (len(g[f]), len(e[f])), e[f] if f in ("k1info", "route") else ""))
    return bad


# ---- the read kernel: self-indexed, every minimizer of a read hits ----------------------------------------------------------------------------
class K1Setup:
    def __init__(self, oracle, preset, w, k):
        from scrubby_amd import lib as S
        self.w, self.k = w, k
        self.mid_occ = 1000 if preset == "sr" else 200
        self.opts = make_opts(preset, w, k, self.mid_occ)
        cases = K.sequences(w, k)
        # empty reads inside the tiles as well (the table has one); the index takes the non-empty ones, one contig per read
        self.names, self.reads = [], []
        for i, (name, s) in enumerate(cases):
            if i % 50 == 17:
                self.names.append(f"empty_{i}"); self.reads.append(b"")
            self.names.append(name); self.reads.append(s)
        self.idx = S.Index.build([s for s in self.reads if len(s)], self.opts)
        self.lut = Lookup(oracle, self.idx, w, k)
        self.ctx = S.Context(self.idx, max(len(self.reads), 130), sum(len(s) for s in self.reads) + 4096, 1024)
        self.want = [self.expect(oracle, s) for s in self.reads]

    def expect(self, oracle, s):
        h, y = K.oracle_sketch(oracle, s, self.w, self.k)
        hit, rec, same = self.lut.records(h, y)
        assert hit.all()
        n_mini = n_seed = len(h)
        occ = rec[:, 2] & np.uint32(0x0fffffff)
        q_occ_max = self.mid_occ if self.opts.q_occ_frac > 0 else 1 << 32
        if n_seed > K.SEED_CAP or n_mini > q_occ_max:
            route = ROUTE_RESKETCH
        elif n_seed == 0:
            route = ROUTE_NONE
        else:
            route = ROUTE_SMALL if int((occ > self.mid_occ).sum()) == 0 and int(occ.astype(np.int64).sum()) <= K2_CAP else ROUTE_BIG
        return {"k1info": n_mini | (n_seed & 0x7fff) << 16 | (int(same.any()) << 31), "route": route, "rec": rec[:K.SEED_CAP], "n_seed": n_seed}

    def close(self):
        self.ctx.close(); self.idx.close()


@pytest.fixture(scope="module", params=K.K1_CFG, ids=lambda c: f"{c[0]}-w{c[1]}-k{c[2]}")
def k1(request, oracle, small_arena):
    s = K1Setup(oracle, *request.param)
    yield s
    s.close()


def test_read_kernel_records_info_and_route(k1):
    got, info = front_end(k1.ctx, k1.reads)
    assert info[0] == 1 and info[1] == K.SEED_CAP
    assert not differences(got, k1.want, k1.names, ("k1info", "route", "rec"))
    routes = {e["route"] for e in k1.want}
    over = [e for e in k1.want if e["n_seed"] > K.SEED_CAP]
    print(f"w={k1.w} k={k1.k}: {len(k1.reads)} reads, routes {sorted(routes)}, {len(over)} over seed_cap, "
          f"{sum(e['k1info'] >> 31 for e in k1.want)} with a tandem seed")
    assert routes == {ROUTE_NONE, ROUTE_SMALL, ROUTE_BIG, ROUTE_RESKETCH} and over and all(e["route"] == ROUTE_RESKETCH for e in over)


def test_read_kernel_at_every_base_pointer_offset(k1):
    """the LDS stage starts at the 16-byte boundary below the tile's first base: all sixteen distances, also between the buffer and offsets[0]"""
    for ptr_off in range(16):
        lead = (1, 5, 16, 29)[ptr_off % 4]
        got, _ = front_end(k1.ctx, k1.reads, ptr_off=ptr_off, lead=lead)
        assert not differences(got, k1.want, k1.names, ("k1info", "route", "rec")), (ptr_off, lead)


@pytest.mark.parametrize("n_reads", (1, 63, 64, 65, 130))
def test_read_kernel_batch_geometry_and_neighbours(k1, n_reads):
    """tiles of 64 reads, full and partial; a read's result does not depend on its neighbours in the tile: two different draws of the table"""
    for seed in (1, 2):
        order = np.random.default_rng([seed, n_reads]).permutation(len(k1.reads))[:n_reads]
        if seed == 2 and n_reads > 1:
            order[n_reads // 2] = k1.names.index("len_0")      # an empty read inside the tile
            order[-1] = k1.names.index("queue_A_1024")         # the guarded byte path on a read that ends exactly at n_bases
        got, _ = front_end(k1.ctx, [k1.reads[i] for i in order], ptr_off=3 * seed, lead=seed)
        assert not differences(got, [k1.want[i] for i in order], [k1.names[i] for i in order], ("k1info", "route", "rec")), (n_reads, seed)


# ---- the long front end ------------------------------------------------------------------------------------------------------------------------
class LongSetup:
    def __init__(self, oracle, w, k, cases, mid_occ, q_occ_frac, max_read_len):
        from scrubby_amd import lib as S
        self.w, self.k, self.mid_occ, self.frac = w, k, mid_occ, q_occ_frac
        self.opts = make_opts("map-ont", w, k, mid_occ, q_occ_frac)
        self.names, self.reads = [n for n, _ in cases], [s for _, s in cases]
        # the first 2 kb of each read as contigs: some minimizers hit, some miss
        self.idx = S.Index.build([s[:2000] for s in self.reads if len(s)], self.opts)
        self.lut = Lookup(oracle, self.idx, w, k)
        total = sum(len(s) for s in self.reads)
        self.ctx = S.Context(self.idx, len(self.reads), 8 * total + 4096, max_read_len)      # room for a minimizer at every base
        self.oracle = oracle

    def expect(self, s, legacy=False):
        h, y = K.oracle_sketch(self.oracle, s, self.w, self.k)
        keep = K.thin(h, self.mid_occ, self.frac)
        h, y = h[keep], y[keep]
        hit, rec, _ = self.lut.records(h, y)      # PREV_SAME: over the minimizers that are left
        if legacy or len(s) == 0:
            return {"k1info": 0, "route": ROUTE_RESKETCH, "rec": rec[:0], "mz": (h[:0], y[:0]), "cut": 0}
        return {"k1info": len(h) | len(rec) << 16, "route": ROUTE_BIG if len(rec) else ROUTE_NONE, "rec": rec, "mz": (h, y), "cut": int((~keep).sum())}

    def close(self):
        self.ctx.close(); self.idx.close()


@pytest.mark.parametrize("w,k", K.LONG_WK)
def test_long_front_end_at_the_segment_seams(oracle, small_arena, w, k):
    """segments of 256 bases start from a clean state w + k bases early: lengths, tie clusters and N around every seam; no thinning"""
    L = LongSetup(oracle, w, k, K.seam_reads(w, k) + [("empty", b"")], mid_occ=50, q_occ_frac=0.0, max_read_len=8192)
    try:
        want = [L.expect(s) for s in L.reads]
        got, info = front_end(L.ctx, L.reads, ptr_off=7, lead=3)
        assert info[0] == 2
        assert not differences(got, want, L.names, ("mz", "k1info", "route", "rec"))
        assert sum(bool((e["rec"][:, 2] & K.REC_PREV_SAME).any()) for e in want) > 10
    finally:
        L.close()


def test_long_front_end_thinning_and_routes(oracle, small_arena):
    """mm_seed_mz_flt at mid_occ = 8: the survivors, PREV_SAME taken over the survivors, hits and misses in an index of the reads' first 2 kb.
    The read with more distinct hashes in over-full bins than the kernel's table has slots (LT_CAP) and the empty read leave for the re-sketch
    path.  A read with more than LT_CAP / 2 of them (table_loaded, about 55 kb) does NOT: the kernel gives up on a probe sequence of LT_CAP / 2
    slots, not on LT_CAP / 2 entries, and at that load no probe sequence is that long - it is thinned in the table, and must be thinned right."""
    w, k = K.LONG_WK[0]
    L = LongSetup(oracle, w, k, K.satellite_reads(w, k, K.THIN_MID_OCC), mid_occ=K.THIN_MID_OCC, q_occ_frac=K.THIN_Q_OCC_FRAC, max_read_len=120000)
    try:
        want = [L.expect(s, legacy=(n == "table_over")) for n, s in zip(L.names, L.reads)]
        got, info = front_end(L.ctx, L.reads)
        assert info[0] == 2
        assert not differences(got, want, L.names, ("mz", "k1info", "route", "rec"))
        by = dict(zip(L.names, want))
        assert by["table_over"]["route"] == ROUTE_RESKETCH and by["empty"]["route"] == ROUTE_RESKETCH and by["table_loaded"]["route"] == ROUTE_BIG
        cut = [n for n in L.names if by[n]["cut"]]
        # a cut right before a survivor with the hash of the survivor before it: PREV_SAME differs before and after the compaction
        print(f"thinned reads: {cut}; routes {sorted({e['route'] for e in want})}")
        assert len(cut) >= 3 and {e["route"] for e in want} == {ROUTE_NONE, ROUTE_BIG, ROUTE_RESKETCH}
        # permuted: a wave takes reads one after the other through the same LDS tables
        order = np.random.default_rng(5).permutation(len(L.reads))
        got, _ = front_end(L.ctx, [L.reads[i] for i in order], ptr_off=11, lead=2)
        assert not differences(got, [want[i] for i in order], [L.names[i] for i in order], ("mz", "k1info", "route", "rec"))
    finally:
        L.close()


# ---- the reference sketch -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,k", K.LONG_WK)
def test_reference_sketch_at_the_segment_seams(oracle, w, k):
    """k_ref_sketch cuts contigs into segments of 1024 bases the same way: the seam material as contigs, through the index dump"""
    from scrubby_amd import lib as S
    contigs = [s for _, s in K.seam_reads(w, k, K.REF_SEG)]
    o = make_opts("map-ont", w, k, 50)
    idx = S.Index.build(contigs, o)
    try:
        got = oracle.Index.wrap(*idx.export(), w, k).dump()
        want = oracle.Index.build(contigs, w, k).dump()
        assert all(np.array_equal(a, b) for a, b in zip(got, want))
        assert idx.info()["n_minimizers"] == int(want[1].sum())
    finally:
        idx.close()
