"""The case table of tests/sketch_cases.py, checked on the CPU before a GPU is spent on it.

(a) From the oracle alone, with a printed count per condition: the table reaches what it is meant to reach - in-window ties, a full
minimizer queue inside a block, tie pushes exactly at and right before a segment seam, reads at and over the read kernel's room for seed
records, reads the thinning screen cuts and reads its table cannot hold.
(b) The oracle's own tie behaviour against a brute force that allows ties: every emitted triple is a real k-mer, none is emitted twice, and
on N-free sequences the rightmost minimum of every full window is emitted.  The converse does not hold (the known answer below)."""
import numpy as np
import pytest

from tests import sketch_cases as K

ALL_K = K.KS + (K.K_WIDE,)


def _triples(h, y):
    return [(int(a), int(b) >> 1, int(b) & 1) for a, b in zip(h, y)]


@pytest.fixture(scope="module")
def sketches(oracle):
    """the oracle's sketch of every case of the table: {(w, k): [(name, seq, hash, y)]}"""
    return {(w, k): [(n, s) + K.oracle_sketch(oracle, s, w, k) for n, s in K.sequences(w, k)] for w in K.WS for k in ALL_K}


def test_known_answer(oracle):
    h, y = K.oracle_sketch(oracle, K.KAT_SEQ, K.KAT_W, K.KAT_K)
    assert _triples(h, y) == K.KAT_MINIMIZERS
    model = K.py_sketch(K.KAT_SEQ, K.KAT_W, K.KAT_K)
    assert [m[:3] for m in model] == K.KAT_MINIMIZERS
    assert model[0][3:] == (8, "first")                      # pushed by the first-window special case, at step 8 ...
    assert (34, 6, 1) not in K.window_minima(K.KAT_SEQ, K.KAT_W, K.KAT_K)      # ... and the minimum of no full window
    assert K.window_minima(K.KAT_SEQ, K.KAT_W, K.KAT_K) <= set(K.KAT_MINIMIZERS)


def test_model_restates_the_oracle(oracle, sketches):
    """py_sketch (which adds the step and the rule of every push) gives the oracle's list: on the table at k = 5 and 21, on the seam reads"""
    n = 0
    for w in K.WS:
        for k in (5, 21):
            for name, s, h, y in sketches[(w, k)]:
                assert [m[:3] for m in K.py_sketch(s, w, k)] == _triples(h, y), (w, k, name)
                n += 1
    for w, k in K.LONG_WK:
        for name, s in K.seam_reads(w, k)[::7]:
            assert [m[:3] for m in K.py_sketch(s, w, k)] == _triples(*K.oracle_sketch(oracle, s, w, k)), (w, k, name)
            n += 1
    print(f"model == oracle on {n} cases")


def test_table_has_in_window_ties():
    tot = tie = 0
    for w in K.WS:
        for k in ALL_K:
            for _, s in K.sequences(w, k):
                tot += 1
                tie += K.has_window_tie(s, w, k)
    print(f"in-window ties: {tie} of {tot} (sequence, w, k) cases = {100.0 * tie / tot:.1f} %")
    assert tie >= 0.25 * tot


def test_table_fills_the_queue_inside_a_block():
    """k1_lane_flush: the lane's eight-entry queue fills when nine or more pushes fall into two consecutive blocks of W steps"""
    for w in K.WS:
        best, who = 0, None
        for k in (15, 21):
            for name, s in K.sequences(w, k):
                if not name.startswith(("queue_", "homo_", "cap_")):
                    continue
                steps = np.array([m[3] for m in K.py_sketch(s, w, k) if m[4] != "end"], np.int64)
                if len(steps) == 0:
                    continue
                per_block = np.bincount(steps // w)
                two = per_block[:-1] + per_block[1:] if len(per_block) > 1 else per_block
                if int(two.max()) > best:
                    best, who = int(two.max()), (name, k)
        print(f"w = {w}: {best} pushes within two consecutive blocks ({who})")
        assert best >= 9


@pytest.mark.parametrize("seg", (K.LSEG, K.REF_SEG))
def test_seam_cases_push_ties_at_the_seam(seg):
    """per W: a tie push made at step `start` exactly (kept by the segment that starts there) and one at `start - 1` (dropped by it)"""
    for w, k in K.LONG_WK:
        at = {0: 0, -1: 0}
        for name, s in K.seam_reads(w, k, seg):
            if not name.startswith(("seam_tie_", "seam_rep_", "seam_n_")) or (at[0] >= 4 and at[-1] >= 4):
                continue
            for m in K.py_sketch(s, w, k):
                if m[4] in ("first", "tie"):
                    for d in at:
                        at[d] += (m[3] - d) % seg == 0 and m[3] - d > 0
        print(f"segment {seg}, w = {w}, k = {k}: {at[0]} tie pushes at step start, {at[-1]} at start - 1")
        assert at[0] >= 1 and at[-1] >= 1


def test_read_kernel_table_reaches_the_record_cap(oracle, sketches):
    """self-indexed, every minimizer of a read hits: its hit count is its minimizer count"""
    for _, w, k in K.K1_CFG:
        n = np.array([len(h) for _, _, h, _ in sketches[(w, k)]])
        over, at = int((n > K.SEED_CAP).sum()), int(((n >= K.SEED_CAP - 1) & (n <= K.SEED_CAP)).sum())
        print(f"w = {w}, k = {k}: {len(n)} reads, {over} over seed_cap = {100.0 * over / len(n):.1f} %, {at} at seed_cap - 1 .. seed_cap")
        assert over >= 1 and at >= 1 and over <= 0.10 * len(n)


def test_satellite_table_reaches_the_thinning_screen(oracle):
    mid_occ, frac = K.THIN_MID_OCC, K.THIN_Q_OCC_FRAC
    w, k = K.LONG_WK[0]
    cut = kept_all = 0
    for name, s in K.satellite_reads(w, k, mid_occ):
        h, _ = K.oracle_sketch(oracle, s, w, k)
        keep = K.thin(h, mid_occ, frac)
        assert len(h) < 65536
        cut += not keep.all()
        kept_all += len(h) > mid_occ and bool(keep.all())
        if name.startswith("table_"):
            bins = np.bincount((h & np.uint64(4095)).astype(np.int64), minlength=4096)
            distinct = len(np.unique(h[bins[(h & np.uint64(4095)).astype(np.int64)] > mid_occ]))
            print(f"{name}: {len(s)} bases, {len(h)} minimizers, {distinct} distinct hashes in over-full bins")
            if name == "table_over":
                assert distinct > K.LT_CAP          # more than the table has slots: some insertion must give up
            else:
                assert K.LT_CAP // 2 < distinct < 0.6 * K.LT_CAP      # past half of it, and loaded lightly enough that no probe walks 1024 slots
    print(f"thinning: {cut} reads lose minimizers, {kept_all} screened reads keep all")
    assert cut >= 3 and kept_all >= 3


def test_oracle_ties_against_the_brute_force(sketches):
    n_cases = n_tie = n_windows = 0
    for (w, k), cases in sketches.items():
        for name, s, h, y in cases:
            kh, kz, ok = K.kmers(s, k)
            pos, strand = (y >> np.uint32(1)).astype(np.int64), (y & np.uint32(1)).astype(np.uint8)
            # every emitted triple is a real k-mer of the sequence with the right hash and strand
            assert np.all(pos < len(s)) and np.all(ok[pos]) and np.array_equal(kh[pos], h) and np.array_equal(kz[pos], strand), (w, k, name)
            # a k-mer has one hash and one strand, so "no triple twice" is "no position twice"
            assert len(np.unique(pos)) == len(pos), (w, k, name)
            n_cases += 1
            if len(s) >= k and ok[k - 1:].all():
                want = K.window_minima(s, w, k)
                got = set(_triples(h, y))
                assert want <= got, (w, k, name, sorted(want - got))
                n_windows += 1
                n_tie += K.has_window_tie(s, w, k)
    print(f"brute force: {n_cases} cases, {n_windows} N-free with every window's rightmost minimum emitted, {n_tie} of those with in-window ties")
    assert n_tie >= 1000
