"""The list search of k_local_cluster (scrubby_amd/csrc/sh_lc_search.h through tests/lc_search_host.cpp): a
seed's occurrence list is searched once (lc_open) and the answer extended at its two ends when the window grows (lc_grow); lc_collect then
gives the in-window entries of the right strand.  Held here against a brute force over the whole list, after every step of a sequence of
nested windows: first, stop, the count, the lowest and highest position, the two remembered neighbours, the collected entries - in C++ for
a few thousand seeded sequences over lists of every length around a step of the 8-ary search, and once more from Python with a brute force
of its own.  The edges the kernel's rounds can meet are walked one by one (lsh_edges), the loads counted by the list's accessor.

lc_search_host.cpp has a main of its own behind -DLC_SEARCH_MAIN that runs the same checks: built with -fsanitize=address,undefined it is
the sanitizer run of this code, a stand-alone program on the CPU (the last test builds and runs it)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "lc_search_host.cpp")
LENGTHS = (2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 511, 512, 513)
NONE, CAP = 0xffffffff, 16


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("lcs") / "liblc_search_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, SRC])
    lib = C.CDLL(so)
    lib.lsh_random.restype = C.c_int; lib.lsh_random.argtypes = [C.c_uint32, C.c_uint32, C.c_int]
    lib.lsh_edges.restype = C.c_int; lib.lsh_edges.argtypes = []
    lib.lsh_steps.restype = C.c_int
    lib.lsh_steps.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    return lib


@pytest.mark.parametrize("n", LENGTHS)
def test_seeded_growth_sequences_against_the_brute_force(L, n):
    rc = L.lsh_random(n, 1, 300)      # 13 lengths x 300: a few thousand sequences of one to four nested windows
    assert rc == 0, f"list of {n}: sequence {rc // 10000}, step {rc % 10000 // 100}, property {rc % 100}"


def test_the_edges_one_by_one(L):
    rc = L.lsh_edges()
    assert rc == 0, f"edge {rc // 1000}: {rc % 1000}"


def steps(L, words, contig, qbit, rel, wins):
    words = np.ascontiguousarray(words, np.uint64)
    win = np.ascontiguousarray(wins, np.uint32).reshape(-1)
    out = np.zeros(8 * len(wins), np.uint32)
    got, n_got = np.zeros(len(words) + 1, np.uint64), np.zeros(1, np.uint32)
    rc = L.lsh_steps(words.ctypes.data, len(words), contig, qbit, rel, win.ctypes.data, len(wins), out.ctypes.data, got.ctypes.data, n_got.ctypes.data)
    return rc, out.reshape(-1, 8), got[:int(n_got[0])]


@pytest.mark.parametrize("n", (9, 65, 513))
def test_a_second_brute_force_in_numpy(L, n):
    rng = np.random.default_rng(n)
    for it in range(60):
        span = int(rng.choice((3 * n, 40 * n, 4000)))
        words = np.unique((rng.integers(3, 6, n).astype(np.uint64) << np.uint64(32)) | rng.integers(0, 2 * span, n).astype(np.uint64))
        contig, qbit, rel = int(rng.integers(3, 6)), int(rng.integers(0, 2)), int(rng.integers(0, 2))
        lo = int(rng.integers(0, span)); hi = lo + int(rng.integers(0, span // 6 + 2))
        wins = [(lo, hi)]
        for _ in range(int(rng.integers(0, 4))):
            lo, hi = max(lo - int(rng.choice((0, 1, 7, span // 5))), 0), hi + int(rng.choice((0, 1, 7, span // 5)))
            wins.append((lo, hi))
        rc, out, got = steps(L, words, contig, qbit, rel, wins)
        assert rc == 0, (n, it, rc)
        ctg, pos, strand = (words >> np.uint64(32)).astype(np.int64), ((words & np.uint64(0xffffffff)) >> np.uint64(1)).astype(np.int64), (words & np.uint64(1)).astype(np.int64)
        right = (strand != qbit) == (rel != 0)
        for (wlo, whi), row in zip(wins, out):
            inside = (ctg == contig) & (pos >= wlo) & (pos <= whi)
            if int((inside & right).sum()) > CAP:
                assert row[2] > CAP
                break
            ix = np.where(inside)[0]
            first = int(((ctg < contig) | ((ctg == contig) & (pos < wlo))).sum())
            assert (int(row[0]), int(row[1]), int(row[2])) == (first, first + len(ix), int((inside & right).sum())), (n, it, wins)
            assert len(ix) == 0 or (ix[0] == first and ix[-1] == first + len(ix) - 1)
            assert int(row[3]) == (int(pos[first - 1]) if first > 0 and ctg[first - 1] == contig else NONE)
            stop = first + len(ix)
            assert int(row[4]) == (int(pos[stop]) if stop < len(words) and ctg[stop] == contig else NONE)
        else:
            assert np.array_equal(got, words[inside & right])


def test_a_confirming_round_costs_no_load(L):
    """what the kernel's last round of every read is: the window grown by less than the distance to either neighbour"""
    words = np.array([(4 << 32) | (p << 1) for p in range(1000, 400_000, 3000)], np.uint64)
    rc, out, got = steps(L, words, 4, 0, 0, [(150_000, 152_000), (149_500, 152_500), (149_001, 152_999), (148_000, 154_000)])
    assert rc == 0
    assert out[0][7] > 0 and out[1][7] == 0 and out[2][7] == 0      # loads of open, then of two grows that the neighbours answer
    assert out[3][7] == 16 and out[3][2] == 3 and len(got) == 3     # both sides reach a neighbour: one group of eight each
    assert [int(x) for x in out[0][3:5]] == [148_000, 154_000]


def test_stand_alone_program_under_the_sanitizers(tmp_path):
    """The same file with its own main, built with AddressSanitizer and UBSan and run as a program of its own.  The sanitizer runtimes are
    linked statically: the program needs nothing from its environment."""
    exe = str(tmp_path / "lc_search_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DLC_SEARCH_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-o", exe, SRC])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "lc search ok" in out.stdout
