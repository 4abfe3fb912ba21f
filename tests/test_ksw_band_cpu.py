"""The band of ksw_extd2 in closed form (scrubby_amd/csrc/sh_ksw_band.h through tests/ksw_band_host.cpp) against the restatement in
tests/ksw_cases.py (`ranges`): the fill loops of every storage form and the backtrack take each anti-diagonal's (st0, en0, st, en) from
this one helper, so it has to give what the fill used to record per diagonal - on every diagonal, for every small shape and band, and
for the shapes a 150-bp read makes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import ksw_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "ksw_band_host.cpp")
BANDS = [-1] + list(range(46))
# what the extension stage asks for on 150-bp reads (w = 151 is `sr`'s band), and the borders of the register form
SHAPES_150 = [(ql, tl, w) for ql in (1, 16, 17, 150, 320, 336) for tl in (1, 3, 15, 16, 17, 63, 64, 65, 240, 255, 256, 257, 272)
              for w in (-1, 1, 7, 16, 40, 151)]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("kb") / "libkb_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, SRC])
    L = C.CDLL(so)
    L.kbh_ranges.restype = C.c_int32
    L.kbh_ranges.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
    return L


def _helper(L, ql, tl, w):
    out = np.zeros((ql + tl, 4), np.int32)
    n = L.kbh_ranges(ql, tl, w, out.ctypes.data)
    return [tuple(int(x) for x in row) for row in out[:n]]


def test_every_small_shape_and_band(host):
    n = 0
    for ql in range(1, 41):
        for tl in range(1, 41):
            for w in BANDS:
                assert _helper(host, ql, tl, w) == K.ranges(ql, tl, w), (ql, tl, w)
                n += 1
    assert n == 40 * 40 * 47


def test_the_shapes_of_150_bp_reads(host):
    for ql, tl, w in SHAPES_150:
        got = _helper(host, ql, tl, w)
        assert got == K.ranges(ql, tl, w), (ql, tl, w)
        assert all(st % 16 == 0 and (en + 1) % 16 == 0 and st <= st0 <= en0 <= en for st0, en0, st, en in got)
