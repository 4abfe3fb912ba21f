"""The ladder of k_sort_top launches (scrubby_amd/csrc/sh_sort_rungs.h through tests/sort_rungs_host.cpp; DESIGN.md section 3.3, "Rungs"):
a table of the LDS sort classes may be served by several launches, each with a block sized to the reads it takes.  Checked here, on the
header big_pass reads: every anchor count of 65 .. 4096 belongs to exactly one launch, that launch's block holds it, a rung's LDS
(24 B per anchor of its NMAX plus the fixed part) fits the residency it was cut for on a CU of 160 KiB, and the rungs of a table tile it
without gap or overlap.

sort_rungs_host.cpp has a main of its own behind -DSORT_RUNGS_MAIN that runs the same checks: built with -fsanitize=address,undefined it is
the sanitizer run of this code, a stand-alone program on the CPU (the last test builds and runs it)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "sort_rungs_host.cpp")
TABLES = ((65, 256), (257, 512), (513, 1024), (1025, 2048), (2049, 4096))      # k_expand's bounds, table 0 .. 4
CU_LDS = 160 * 1024
LDS_PER_ANCHOR, LDS_FIXED = 24, 2160      # two ping-pong buffers of (x, q); k_sort_top's other shared variables


@pytest.fixture(scope="module")
def rungs(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("rungs") / "libsort_rungs_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, SRC])
    L = C.CDLL(so)
    for name in ("srh_count", "srh_check"):
        getattr(L, name).restype = C.c_int; getattr(L, name).argtypes = []
    for name in ("srh_lds", "srh_budget", "srh_rung_of", "srh_last_of_table", "srh_alone", "srh_launches_for"):
        getattr(L, name).restype = C.c_int; getattr(L, name).argtypes = [C.c_int]
    L.srh_get.restype = None; L.srh_get.argtypes = [C.c_int, C.c_void_p]
    table = []
    for i in range(L.srh_count()):
        v = np.zeros(5, np.int32)
        L.srh_get(i, v.ctypes.data)
        table.append(dict(zip(("cls", "nmin", "nmax", "nthr", "blocks"), (int(x) for x in v))))
    return L, table


def test_every_anchor_count_belongs_to_exactly_one_launch_that_holds_it(rungs):
    L, table = rungs
    for n in range(65, 4097):
        cls = next(t for t, (lo, hi) in enumerate(TABLES) if lo <= n <= hi)
        mine = [r for r in table if r["cls"] == cls and r["nmin"] < n <= r["nmax"]]      # the kernel's test, on the table the read is listed in
        assert len(mine) == 1, (n, mine)
        assert mine[0]["nmax"] >= n
        assert L.srh_launches_for(n) == 1 and table[L.srh_rung_of(n)] is mine[0]
    assert L.srh_rung_of(64) == -1 and L.srh_rung_of(4097) == -1


def test_a_rungs_lds_fits_the_residency_it_was_cut_for(rungs):
    L, table = rungs
    for r in table:
        lds = LDS_PER_ANCHOR * r["nmax"] + LDS_FIXED
        assert L.srh_lds(r["nmax"]) == lds
        assert lds <= CU_LDS // r["blocks"], r
        assert lds <= L.srh_budget(r["blocks"]) <= CU_LDS // r["blocks"], r      # in whole allocation granules too
        assert r["nmax"] % 64 == 0 and r["blocks"] * (r["nthr"] // 64) <= 32, r


def test_the_rungs_of_a_table_tile_it(rungs):
    L, table = rungs
    assert [r["cls"] for r in table] == sorted(r["cls"] for r in table)
    for cls, (lo, hi) in enumerate(TABLES):
        mine = [r for r in table if r["cls"] == cls]
        assert mine, cls
        assert mine[0]["nmin"] == lo - 1 and mine[-1]["nmax"] == hi
        for a, b in zip(mine, mine[1:]):
            assert a["nmax"] == b["nmin"] and a["nthr"] == b["nthr"] and a["blocks"] > b["blocks"], (a, b)
        assert [L.srh_last_of_table(table.index(r)) for r in mine] == [0] * (len(mine) - 1) + [1]
        # a table's only rung does not look at n (the kernel takes every listed read): only where the rung IS the table
        assert [L.srh_alone(table.index(r)) for r in mine] == [1 if len(mine) == 1 else 0] * len(mine)
    assert all(len([r for r in table if r["cls"] == cls]) == 1 for cls in (0, 1, 2))      # tables 0-2 keep one launch each
    assert L.srh_check() == 0


def test_stand_alone_program_under_the_sanitizers(tmp_path):
    """The same file with its own main, built with AddressSanitizer and UBSan and run as a program of its own.  The sanitizer runtimes are
    linked statically: the program needs nothing from its environment."""
    exe = str(tmp_path / "sort_rungs_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DSORT_RUNGS_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-o", exe, SRC])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "rungs ok" in out.stdout
