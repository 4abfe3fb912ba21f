"""The classify path's environment switches (scrubby_amd/csrc/sh_switches.h through tests/switches_host.cpp): with an empty environment both
structs hold the defaults; every clamp; a SCRUBBY_HIP_GIANT_FANIN other than 2 or 4 is reported; every name of the context group changes
shi_switches_sig() and no name of the call group does; SCRUBBY_HIP_DBG gives the "set" field and the mask with the behaviour switches folded
in.  Then the sources: the list is the only place that reads these variables, INTEGRATION.md names all of them, and no test of a dbg bit is
left as a bare number.

switches_host.cpp has a main of its own behind -DSWITCHES_MAIN that runs the same cases: built with -fsanitize=address,undefined it is the
sanitizer run of this code, a stand-alone program on the CPU (the last test builds and runs it)."""
import ctypes as C
import glob
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "switches_host.cpp")
CSRC = os.path.join(ROOT, "scrubby_amd", "csrc")
CASES = ["defaults", "values_and_clamps", "giant_fanin", "signature", "dbg"]      # the order of CASES[] in switches_host.cpp
# what the issue of this list counted in the sources
CTX_NAMES = {"SCRUBBY_HIP_" + n for n in ("ARENA_MB EXT_MB EXT_REGCAP LEXT_A LEXT_BIG_A LEXT_P_KB LEXT_BIG_P_KB STAGE_MB STREAMS NO_FLAG_STOP NO_PAIR PAIR_MIN "
                                          "NO_S1 NO_LEMMA RMQ_EXACT_MAX RMQ_ONE_LANE E2_JOIN_MIN COOP_MIN COOP_RUN COOP_CHECK").split()}
CALL_NAMES = {"SCRUBBY_HIP_" + n for n in ("DBG AB_NOCHAIN NO_PARFILL GIANT_FANIN PFT_GMIN TOPBT_MAX NO_TOPBT LOCUS_TOP1 NO_LOCUS NO_PROBE NO_CL_LDS DBG_EXACT "
                                           "GIANT_BINS_DOWN GIANT_WAVES SIDE_PICK SIDE K2_LATE NO_COOP GIANTS_PLAIN NO_FOLLOW").split()}


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("sw") / "libsw_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-o", so, SRC])      # plain g++: the header is host only
    L = C.CDLL(so)
    L.swh_name.restype = C.c_char_p
    return L


def _names(L, call_group):
    return [L.swh_name(call_group, i).decode() for i in range(L.swh_n_names(call_group))]


@pytest.mark.parametrize("case", CASES)
def test_switch_list(host, case):
    assert host.swh_n_cases() == len(CASES)
    rc = host.swh_case(CASES.index(case))
    assert rc == 0, f"switches_host.cpp: the check in line {rc} failed"


def test_the_list_holds_the_forty_names_in_their_groups(host):
    ctx, call = _names(host, 0), _names(host, 1)
    assert len(set(ctx + call)) == len(ctx + call) == 40
    assert set(ctx) == CTX_NAMES and set(call) == CALL_NAMES


def test_sources_read_the_environment_through_the_list_only(host):
    text = {p: open(p).read() for ext in ("*.h", "*.hip", "*.cpp") for p in glob.glob(os.path.join(CSRC, ext))}
    for f in ("sh_classify.hip", "sh_long.h", "sh_api.hip"):
        assert "getenv" not in text[os.path.join(CSRC, f)], f
    for name in _names(host, 0) + _names(host, 1):
        where = [os.path.basename(p) for p, t in text.items() if f'"{name}"' in t]
        assert where == ["sh_switches.h"] and text[os.path.join(CSRC, "sh_switches.h")].count(f'"{name}"') == 1, (name, where)
    for p, t in text.items():
        assert not re.search(r"dbg\s*(&|\|=|&=)\s*~?\d", t), p


def test_integration_md_names_every_switch(host):
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in _names(host, 0) + _names(host, 1):
        assert f"`{name}`" in doc or f"`{name}=" in doc, name
    src = open(os.path.join(CSRC, "sh_switches.h")).read()
    bits = re.findall(r"^\s*(DBG_[A-Z0-9_]+) = \d+,", src, re.M)
    assert len(bits) == 9
    for b in bits:
        assert f"`{b}`" in doc, b


def test_stand_alone_program_under_the_sanitizers(tmp_path):
    """The same file with its own main, built with AddressSanitizer and UBSan and run as a program of its own, with an empty environment.
    The sanitizer runtimes are linked statically: the program needs nothing from its environment."""
    exe = str(tmp_path / "switches_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DSWITCHES_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-o", exe, SRC])
    out = subprocess.run([exe], capture_output=True, text=True, env={})
    assert out.returncode == 0, out.stdout + out.stderr
    assert f"{len(CASES)} cases ok" in out.stdout
