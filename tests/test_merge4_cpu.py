"""The giant reads' merge passes on the host (scrubby_amd/csrc/sh_merge4.h through tests/merge4_host.cpp): the group bounds of a tile, the
four-way co-rank and the per-thread two-level merge, driven the way the kernels drive them, on tiles of 8 anchors - against a stable sort on
(key, original index), and fan-in 4 against two rounds of fan-in 2 element for element.  The sizes are the smallest at which the passes can
go wrong: groups of 1 / 2 / 3 / 4 runs, a short last run, one, two and three passes, a second-pass group that is itself incomplete.

merge4_host.cpp has a main of its own behind -DMERGE4_MAIN that runs the same cases: built with -fsanitize=address,undefined it is the
sanitizer run of this code, a stand-alone program on the CPU (the last test builds and runs it)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "merge4_host.cpp")
TILE = 8
SIZES = [T * TILE + r for T in (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 20, 64, 65) for r in (0, 1, TILE - 1)]
KEYS = {"all_equal": 0, "three_values": 1, "increasing_across_runs": 2, "decreasing_across_runs": 3, "random_64_bit": 4}


@pytest.fixture(scope="module")
def host_merge(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("m4") / "libm4_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, SRC])
    L = C.CDLL(so)
    L.m4h_sort.restype = C.c_int
    L.m4h_sort.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.m4h_keys.restype = None
    L.m4h_keys.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_uint64]
    L.m4h_case.restype = C.c_int
    L.m4h_case.argtypes = [C.c_uint32, C.c_uint32, C.c_int, C.c_uint64]
    return L


def _sort(L, x, fanin, max_pass=0xFFFFFFFF):
    n = len(x)
    ox = np.zeros(n, np.uint64); oq = np.zeros(n, np.uint32); npass = C.c_uint32(0)
    rc = L.m4h_sort(x.ctypes.data, n, TILE, fanin, max_pass, ox.ctypes.data, oq.ctypes.data, C.byref(npass))
    # 100 * pass + code: 1 / 2 group bounds, 3 offsets exceed the tile's output offset, 4 offset outside its run, 5 not monotone,
    # 6 a group's first tile does not start at the run starts, 7 the tile's inputs are not its outputs' number
    assert rc == 0, f"n {n} fan-in {fanin}: split property {rc % 100} failed in pass {rc // 100 - 1}"
    return ox, oq, npass.value


@pytest.mark.parametrize("keys", list(KEYS))
def test_passes_equal_the_stable_sort_and_two_rounds_of_fan_in_2(host_merge, keys):
    for n in SIZES:
        x = np.zeros(n, np.uint64)
        host_merge.m4h_keys(x.ctypes.data, n, TILE, KEYS[keys], 1000 * KEYS[keys] + n)
        ref = np.argsort(x, kind="stable").astype(np.uint32)
        x4, q4, p4 = _sort(host_merge, x, 4)
        x2, q2, p2 = _sort(host_merge, x, 2)
        runs = -(-n // TILE)
        assert p2 == (runs - 1).bit_length() and p4 == (p2 + 1) // 2
        assert np.array_equal(q4, ref) and np.array_equal(x4, x[ref]), f"n {n}: fan-in 4 is not the stable sort"
        assert np.array_equal(q2, ref) and np.array_equal(x2, x[ref]), f"n {n}: fan-in 2 is not the stable sort"
        for p in range(1, p4 + 1):
            a = _sort(host_merge, x, 4, p)
            b = _sort(host_merge, x, 2, 2 * p)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), f"n {n}: pass {p - 1} differs from rounds {2 * p - 2} and {2 * p - 1}"
        assert host_merge.m4h_case(n, TILE, KEYS[keys], 1000 * KEYS[keys] + n) == 0      # the same, as the stand-alone program checks it


def test_stand_alone_program_under_the_sanitizers(tmp_path):
    """The same file with its own main, built with AddressSanitizer and UBSan and run as a program of its own: an index one past a run, a
    tile or the array standing in for LDS ends it with a report.  The sanitizer runtimes are linked statically: the program needs nothing
    from its environment."""
    exe = str(tmp_path / "merge4_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DMERGE4_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-o", exe, SRC])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert f"{5 * len(SIZES)} cases ok" in out.stdout
