"""The wave route's public surface without a GPU: the ctypes mirrors of sh_k2_opts / sh_k2_stats against the C header's
sizeof / offsetof (a tiny host program), the defaults, the exported tile size, and the oracle's answer for the poly-A read
that tests/test_k2_long_gpu.py builds its "one run across every lane" case on."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROG = r"""
#include <stdio.h>
#include <stddef.h>
#include "scrubby_hip.h"
int main(void)
{
    printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(sh_k2_opts), offsetof(sh_k2_opts, quick), offsetof(sh_k2_opts, long_unit_bases),
           sizeof(sh_k2_stats), offsetof(sh_k2_stats, n_masked_bases), offsetof(sh_k2_stats, n_long_units), offsetof(sh_k2_stats, ms_long));
    return 0;
}
"""


def test_ctypes_layouts_match_the_header(tmp_path):
    from scrubby_amd import k2
    src, exe = tmp_path / "abi.c", tmp_path / "abi"
    src.write_text(PROG)
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    O, S = k2.K2Opts, k2.K2Stats
    assert got == [C.sizeof(O), O.quick.offset, O.long_unit_bases.offset, C.sizeof(S), S.n_masked_bases.offset, S.n_long_units.offset, S.ms_long.offset]
    # the old layouts are prefixes of the new ones
    assert O.quick.offset == 52 and O.long_unit_bases.offset == 56 and C.sizeof(O) == 64
    assert S.n_masked_bases.offset == 48 and S.n_long_units.offset == 56 and C.sizeof(S) == 72
    assert "pad_" not in k2._stats_dict(S()) and {"n_long_units", "ms_long"} <= set(k2._stats_dict(S()))


def test_defaults_and_tile():
    from scrubby_amd import k2, lib
    o = k2.default_opts()
    assert o.long_unit_bases == 0 and o.k == 35 and o.l == 31
    L = lib.load()
    L.sh_k2_wave_tile.restype = C.c_uint32
    assert L.sh_k2_wave_tile() == k2.K2_WAVE_TILE and k2.K2_WAVE_TILE % 64 == 0


def test_oracle_poly_a_is_one_hit_group(oracle):
    """a 5 000-base poly-A read whose minimizer is in the table: one run, one hit group, however many k-mers"""
    o = oracle.k2_default_opts()
    read = b"A" * 5000
    mins, amb = oracle.k2_scan(read, o)
    assert len(mins) == 5000 - 34 and not amb.any() and len(set(int(m) for m in mins)) == 1
    parent = np.array([0, 0, 1, 1], dtype=np.uint32)
    t = oracle.K2Table.empty(1009, parent, 17)
    t.set(int(mins[0]), 2)
    r = t.classify_pair(o, read)
    assert r["hit_groups"] == 1 and r["n_probes"] == 1 and r["total_kmers"] == 5000 - 34
    assert r["call"] == 0                              # one hit group is below --minimum-hit-groups 2
    s = bytearray(read)
    s[1000:1300] = b"N" * 300
    r = t.classify_pair(o, bytes(s))
    assert r["hit_groups"] == 1 and r["n_probes"] == 1 and r["total_kmers"] == 5000 - 34      # the run resumes after the ambiguous k-mers
