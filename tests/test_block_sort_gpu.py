"""The stable block sort of the repeat path (block_merge_sort, csrc/sh_wave.h), called directly: sh_dbg_block_sort (csrc/sh_dbg_chain.hip)
runs one block per case over n (x, q) pairs in LDS, with the thread counts of the kernels that call it in the product (64, 128, 256 and 512:
k_sort_top / k_sort_lds<256 .. 4096>, k_giant_chunksort, k_group_probe), and returns both arrays.

Reference: numpy's stable argsort of x.  q is the input index, so an unstable sort shows as a q out of place among equal x.  The sizes sit
on both sides of one 64-anchor tile, of two and of four tiles (the first merge rounds), and at the LDS classes' capacity; the key patterns
are the ones the tile phase and the merge rounds can go wrong on: all equal, two values, ascending (the tile phase skips such a tile),
descending, random 64-bit keys, a concatenation of ascending runs that share keys (the order anchors are generated in), keys equal to
0xffffffffffffffff (the value the padding lanes of a short tile hold) and keys that differ in the high word only."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000, 2048, 4096)
NTHR = (64, 128, 256, 512)
PATTERNS = ("equal", "two_values", "ascending", "descending", "random", "runs", "all_ones_mixed", "high_word")
FULL = np.uint64(0xFFFFFFFFFFFFFFFF)


class SortCase(C.Structure):
    _fields_ = [("off", C.c_uint64), ("n", C.c_int32), ("nthr", C.c_int32)]


def keys(pattern, n, rng):
    if pattern == "equal":
        return np.full(n, 0x0000000500000007, np.uint64)
    if pattern == "two_values":
        return np.where(np.arange(n) & 1, np.uint64(3), np.uint64(0x100000000)).astype(np.uint64)
    if pattern == "ascending":
        return np.cumsum(rng.integers(0, 3, n)).astype(np.uint64) + np.uint64(1 << 40)      # with ties
    if pattern == "descending":
        return (np.uint64(1 << 40) - np.cumsum(rng.integers(0, 3, n)).astype(np.uint64))
    if pattern == "random":
        return rng.integers(0, 1 << 64, n, dtype=np.uint64)
    if pattern == "runs":      # 2..40 ascending runs drawn from one small set of keys: equal keys across the runs
        n_runs = int(min(max(n, 1), rng.integers(2, 41)))
        cuts = np.sort(rng.choice(np.arange(1, n), n_runs - 1, replace=False)) if n > 1 and n_runs > 1 else np.zeros(0, np.int64)
        pool = np.uint64(1 << 33) + rng.integers(0, max(n // 3, 2), n).astype(np.uint64) * np.uint64(5)
        return np.concatenate([np.sort(part) for part in np.split(pool, cuts)]).astype(np.uint64)
    if pattern == "all_ones_mixed":
        x = rng.integers(0, 1 << 64, n, dtype=np.uint64)
        x[rng.random(n) < 0.3] = FULL
        x[rng.random(n) < 0.1] = FULL - np.uint64(1)
        if n:
            x[0] = FULL      # one ahead of everything: it must end behind the others and ahead of the later ones
        return x
    if pattern == "high_word":
        return (rng.integers(0, 7, n).astype(np.uint64) << np.uint64(32)) | np.uint64(0x89ABCDEF)
    raise AssertionError(pattern)


@pytest.fixture(scope="module")
def sorted_cases():
    """every (pattern, size, thread count) in ONE call: the cases, the input and what came back"""
    from scrubby_amd import lib
    L = lib.require_gpu()
    rng = np.random.default_rng(0xB10C)
    cases, xs, qs = [], [], []
    off = 0
    for pattern in PATTERNS:
        for n in SIZES:
            x = keys(pattern, n, rng)
            assert x.dtype == np.uint64 and len(x) == n
            for nthr in NTHR:
                cases.append((pattern, n, nthr, off))
                xs.append(x)
                qs.append(np.arange(n, dtype=np.uint32))
                off += n
    x = np.ascontiguousarray(np.concatenate(xs))
    q = np.ascontiguousarray(np.concatenate(qs))
    arr = (SortCase * len(cases))(*[SortCase(o, n, t) for _, n, t, o in cases])
    ox, oq = np.zeros_like(x), np.full_like(q, 0xFFFFFFFF)
    lib.check(L.sh_dbg_block_sort(0, x.ctypes.data, q.ctypes.data, len(x), C.cast(arr, C.c_void_p), len(cases), ox.ctypes.data, oq.ctypes.data))
    return cases, x, ox, oq


@pytest.mark.parametrize("pattern", PATTERNS)
def test_block_sort_is_numpys_stable_sort(sorted_cases, pattern):
    cases, x, ox, oq = sorted_cases
    seen = 0
    for pat, n, nthr, off in cases:
        if pat != pattern:
            continue
        xi = x[off:off + n]
        order = np.argsort(xi, kind="stable")
        assert np.array_equal(ox[off:off + n], xi[order]), f"{pattern}, n = {n}, {nthr} threads: keys out of order"
        assert np.array_equal(oq[off:off + n], order.astype(np.uint32)), f"{pattern}, n = {n}, {nthr} threads: equal keys changed places"
        seen += 1
    assert seen == len(SIZES) * len(NTHR)


def test_patterns_are_what_they_claim():
    rng = np.random.default_rng(1)
    assert (np.diff(keys("ascending", 300, rng).astype(np.int64)) >= 0).all() and (np.diff(keys("descending", 300, rng).astype(np.int64)) <= 0).all()
    r = keys("runs", 1000, rng)
    assert 1 <= int((np.diff(r.astype(np.int64)) < 0).sum()) <= 39 and len(np.unique(r)) < len(r)
    m = keys("all_ones_mixed", 1000, rng)
    assert int((m == FULL).sum()) > 100 and int((m != FULL).sum()) > 100
    h = keys("high_word", 1000, rng)
    assert len(np.unique(h)) == 7 and len(np.unique(h & np.uint64(0xFFFFFFFF))) == 1


def test_bad_arguments_are_refused_before_any_launch():
    from scrubby_amd import lib
    L = lib.require_gpu()
    x, q = np.zeros(8, np.uint64), np.zeros(8, np.uint32)
    for bad in (SortCase(0, 8, 100), SortCase(0, 0, 64), SortCase(4, 8, 64), SortCase(0, 4097, 512)):
        arr = (SortCase * 1)(bad)
        rc = L.sh_dbg_block_sort(0, x.ctypes.data, q.ctypes.data, 8, C.cast(arr, C.c_void_p), 1, x.ctypes.data, q.ctypes.data)
        assert lib.STATUS_NAMES[rc] == "SH_ERR_BAD_ARG", (bad.off, bad.n, bad.nthr, rc)
