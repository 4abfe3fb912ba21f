"""stage_anchors (csrc/sh_chain.h): the anchors of a short read built straight into the LDS sort buffer of the kernel that sorts them
(k_sort_top / k_sort_lds, k_giant_chunksort) instead of being written to the arena by k_expand and read back.  Called directly through
sh_dbg_stage_anchors (csrc/sh_dbg_chain.hip), which also returns the same range from a plain one-thread loop over the seeds seed_filter keeps,
make_anchor per occurrence: the order gen_anchors and k_chain_large use.  A numpy restatement of that loop is the third opinion wherever the
filter is the plain cut.

Synthetic seed records; occurrence lists are random ascending position words on two contigs with both strand bits.  The shapes are the
smallest at which the index arithmetic can go wrong: totals around every class bound staged whole, the 2048-anchor tiles of reads of two
tiles and a bit, exactly three tiles, three tiles and one; one seed, two, 64; singletons between lists; filtered seeds (empty runs in the
prefix sums) first, in the middle and last; run lengths around 64 and around the thread count; every thread count the kernels use."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K = 21
MAX_OCC = 7000          # plain cut: one seed may carry a whole read of 6145 anchors
NTHR = (64, 128, 256, 512)
WHOLE = (65, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 4096)
TILED = (4097, 6144, 6145)
TILE = 2048


class Case(C.Structure):
    _fields_ = [("rec_off", C.c_uint64), ("out_off", C.c_uint64), ("n_seed", C.c_int32), ("qlen", C.c_int32), ("nthr", C.c_int32), ("pad", C.c_int32),
                ("c0", C.c_uint32), ("m", C.c_uint32)]


@pytest.fixture(scope="module")
def S():
    from scrubby_amd import lib
    lib.require_gpu()
    return lib


class Builder:
    """records, positions and cases of one call"""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.pos = [self._list(MAX_OCC + 1000)]      # list 0: what the filtered seeds point at
        self.n_pos = len(self.pos[0])
        self.recs, self.cases, self.reads = [], [], []
        self.n_out = 0

    def _list(self, n):
        rng = self.rng
        ctg = np.sort(rng.integers(0, 2, n)).astype(np.uint64)
        p = np.sort(rng.integers(0, 1 << 30, n)).astype(np.uint64)      # ascending inside a contig as well: sorted overall
        return ctg << np.uint64(32) | p << np.uint64(1) | rng.integers(0, 2, n).astype(np.uint64)

    def read(self, occs, qlen=150):
        """occs: occurrences per seed in query order (> MAX_OCC: filtered by the plain cut, 1: the position word sits in the record)"""
        rng = self.rng
        n = len(occs)
        assert 1 <= n <= 64
        qpos = np.sort(rng.choice(np.arange(K - 1, qlen), n, replace=False))
        rec = np.zeros((n, 4), np.uint32)
        lists = []
        for i, occ in enumerate(occs):
            if occ == 1:
                w1 = int(self._list(1)[0]); lists.append(np.array([w1], np.uint64))
            elif occ > MAX_OCC:
                w1 = 0 << 28 | (occ & 0xfffffff); lists.append(None)
                assert occ <= len(self.pos[0])
            else:
                lst = self._list(occ)
                w1 = self.n_pos << 28 | occ
                self.pos.append(lst); self.n_pos += occ; lists.append(lst)
            rec[i] = (w1 & 0xffffffff, w1 >> 32, occ, int(qpos[i]) << 1 | int(rng.integers(0, 2)))
        rid = len(self.reads)
        self.reads.append((sum(len(r) for r in self.recs), n, qlen, rec, lists))
        self.recs.append(rec)
        return rid

    def case(self, rid, nthr, c0, m):
        rec_off, n, qlen, _, _ = self.reads[rid]
        self.cases.append((rid, Case(rec_off, self.n_out, n, qlen, nthr, 0, c0, m)))
        self.n_out += m

    def expected(self, rid, max_occ=MAX_OCC):
        """the plain loop in numpy (plain cut)"""
        _, n, qlen, rec, lists = self.reads[rid]
        xs, qs = [], []
        for i in range(n):
            if rec[i, 2] > max_occ:
                continue
            r = lists[i]
            qz = int(rec[i, 3])
            same = (r & np.uint64(1)) == np.uint64(qz & 1)
            hi = r & np.uint64(0xffffffff00000000)
            rpos = (r & np.uint64(0xffffffff)) >> np.uint64(1)
            xs.append(np.where(same, hi | rpos, np.uint64(1 << 63) | hi | rpos))
            qs.append(np.where(same, np.uint32(qz >> 1), np.uint32(qlen - ((qz >> 1) + 1 - K) - 1)).astype(np.uint32))
        return np.concatenate(xs), np.concatenate(qs)

    def run(self, S, max_occ=MAX_OCC, max_max_occ=0, occ_dist=0):
        L = S.load()
        recs = np.ascontiguousarray(np.concatenate(self.recs))
        pos = np.ascontiguousarray(np.concatenate(self.pos))
        arr = (Case * len(self.cases))(*[c for _, c in self.cases])
        ox, rx = np.empty(self.n_out, np.uint64), np.empty(self.n_out, np.uint64)
        oq, rq = np.empty(self.n_out, np.uint32), np.empty(self.n_out, np.uint32)
        total = np.empty(len(self.cases), np.uint32)
        S.check(L.sh_dbg_stage_anchors(0, recs.ctypes.data, len(recs), pos.ctypes.data, len(pos), K, max_occ, max_max_occ, occ_dist, C.cast(arr, C.c_void_p),
                                       len(self.cases), self.n_out, ox.ctypes.data, oq.ctypes.data, rx.ctypes.data, rq.ctypes.data, total.ctypes.data))
        return ox, oq, rx, rq, total


def split(total, parts, rng):
    """`parts` positive run lengths that sum to total"""
    cuts = np.sort(rng.choice(np.arange(1, total), parts - 1, replace=False)) if parts > 1 else np.array([], np.int64)
    return [int(v) for v in np.diff(np.concatenate([[0], cuts, [total]]))]


def layouts(total, rng):
    """seed layouts of a read of `total` anchors"""
    out = {"one seed": [total], "two seeds": split(total, 2, rng), "64 seeds": split(total, 64, rng)}
    runs = split(total - 10, 20, rng)
    out["singletons between lists"] = [v for i, r in enumerate(runs) for v in ((r, 1) if i < 10 else (r,))]
    body = split(total, 30, rng)
    out["filtered first, middle, last"] = [MAX_OCC + 1] + body[:15] + [MAX_OCC + 7, MAX_OCC + 2] + body[15:] + [MAX_OCC + 500]
    return out


def check(B, out, max_occ=MAX_OCC, numpy_too=True):
    ox, oq, rx, rq, total = out
    assert np.array_equal(ox, rx) and np.array_equal(oq, rq), f"{int((ox != rx).sum())} x and {int((oq != rq).sum())} q differ from the plain loop"
    for ci, (rid, c) in enumerate(B.cases):
        occ = B.reads[rid][3][:, 2].astype(np.int64)
        if numpy_too:
            assert int(total[ci]) == int(occ[occ <= max_occ].sum()), (ci, int(total[ci]))
            ex, eq = B.expected(rid, max_occ)
            sl = slice(c.out_off, c.out_off + c.m)
            assert np.array_equal(ox[sl], ex[c.c0:c.c0 + c.m]) and np.array_equal(oq[sl], eq[c.c0:c.c0 + c.m]), f"case {ci}: read {rid}, {c.nthr} threads, [{c.c0}, {c.c0 + c.m})"
        assert c.c0 + c.m <= int(total[ci])


def test_whole_reads_around_every_class_bound(S):
    B = Builder(0x51A6E)
    for total in WHOLE:
        for name, occs in layouts(total, B.rng).items():
            rid = B.read(occs)
            for nthr in NTHR:
                B.case(rid, nthr, 0, total)
    print(len(B.cases), "cases,", B.n_out, "anchors")
    check(B, B.run(S))


def test_run_lengths_around_the_wave_and_the_block(S):
    B = Builder(0x51A6F)
    for nthr in NTHR:
        runs = [1, 63, 64, 65, nthr - 1, nthr, nthr + 1]
        for occs in (runs, runs[::-1], [MAX_OCC + 1] + runs + [1, 1]):
            rid = B.read(occs)
            for t in NTHR:
                B.case(rid, t, 0, sum(o for o in occs if o <= MAX_OCC))
    check(B, B.run(S))


def test_every_tile_of_reads_beyond_the_lds_classes(S):
    """k_giant_chunksort's ranges: every 2048-anchor tile, the short last one too; with one seed, or two, a run straddles every tile bound"""
    B = Builder(0x51A70)
    for total in TILED:
        for name, occs in layouts(total, B.rng).items():
            rid = B.read(occs)
            for nthr in NTHR:
                for c0 in range(0, total, TILE):
                    B.case(rid, nthr, c0, min(TILE, total - c0))
    n_tiles = sum(-(-t // TILE) for t in TILED)
    assert len(B.cases) == n_tiles * 5 * len(NTHR)
    check(B, B.run(S))


def test_the_streak_rule_keeps_a_seed_above_max_occ(S):
    """300 bases, occ_dist 500: the streak of high seeds behind the low one spans more than 250 bases, so max_high_occ = 1 and its seed of
    fewest occurrences stays (mm_seed_select); the one above max_max_occ never does"""
    B = Builder(0x51A71)
    occs = [40, 120, 90, 3000, 100, 95]      # max_occ 50: one low seed, then a streak whose smallest member is 90; 3000 > max_max_occ
    rid = B.read(occs, qlen=300)
    rec = B.reads[rid][3]
    rec[:, 3] = [(30 << 1) | 1, 80 << 1, (120 << 1) | 1, 170 << 1, 220 << 1, (280 << 1) | 1]      # the streak: query 30 .. 300
    for nthr in NTHR:
        B.case(rid, nthr, 0, 130)
        B.case(rid, nthr, 40, 90)      # the kept high seed alone
    out = B.run(S, max_occ=50, max_max_occ=2000, occ_dist=500)
    assert (out[4] == 130).all(), out[4]      # 40 + 90: the count is the sum of the occurrences that stay
    check(B, out, numpy_too=False)
    ex, eq = B.expected(rid, max_occ=10 ** 9)      # every seed's anchors; the kept ones are seeds 0 and 2
    keep = np.concatenate([np.arange(0, 40), np.arange(160, 250)])
    for ci, (_, c) in enumerate(B.cases):
        sl = slice(c.out_off, c.out_off + c.m)
        assert np.array_equal(out[0][sl], ex[keep][c.c0:c.c0 + c.m]) and np.array_equal(out[1][sl], eq[keep][c.c0:c.c0 + c.m]), ci


def test_a_range_beyond_the_read_or_outside_the_arrays_is_refused(S):
    B = Builder(0x51A72)
    rid = B.read([100, 1, 30])
    B.case(rid, 64, 100, 32)      # 131 anchors: [100, 132) reaches past them - not staged, the fill comes back
    ox, oq, rx, rq, total = B.run(S)
    assert int(total[0]) == 131 and (ox == 0).all() and (oq == 0xffffffff).all()
    L = S.load()
    rec = np.array([[5 << 28 | 9, 0, 9, 40 << 1]], np.uint32)      # nine occurrences at slot 5 of a list of eight
    pos = np.arange(8, dtype=np.uint64)
    arr = (Case * 1)(Case(0, 0, 1, 150, 64, 0, 0, 9))
    o8, o4 = np.zeros(9, np.uint64), np.zeros(9, np.uint32)
    rc = L.sh_dbg_stage_anchors(0, rec.ctypes.data, 1, pos.ctypes.data, 8, K, MAX_OCC, 0, 0, C.cast(arr, C.c_void_p), 1, 9, o8.ctypes.data, o4.ctypes.data,
                                o8.ctypes.data, o4.ctypes.data, o4.ctypes.data)
    assert rc != 0
