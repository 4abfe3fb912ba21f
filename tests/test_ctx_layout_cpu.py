"""The capacities and buffer layouts of a classify context (scrubby_amd/csrc/sh_ctx_layout.h through tests/ctx_layout_host.cpp), without a
GPU: for max_reads x max_read_len x {flag-only, SH_F_CIGAR short reads, SH_F_CIGAR long reads} x w x arena size x {no override, EXT_MB and
STAGE_MB set}, count mode and place mode of every layout agree, every array is aligned, inside its allocation and apart from the others,
the totals and capacities equal the closed forms sh_ctx_create held before, and the arena's layout fits the arena.

ctx_layout_host.cpp has a main of its own behind -DCTX_LAYOUT_MAIN: built by plain g++ (the header is host only) with
-fsanitize=address,undefined it is a stand-alone program on the CPU that writes the first and last byte of every array it places."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "ctx_layout_host.cpp")
N_COMBINATIONS = 6 * 5 * 3 * 3 * 3 * 2


def test_stand_alone_program_under_the_sanitizers(tmp_path):
    """Built with AddressSanitizer and UBSan (runtimes linked statically) and run as a program of its own, with nothing preloaded."""
    exe = str(tmp_path / "ctx_layout_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-DCTX_LAYOUT_MAIN", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-o", exe, SRC])
    out = subprocess.run([exe], capture_output=True, text=True, env={})
    assert out.returncode == 0, out.stdout + out.stderr
    m = re.search(r"(\d+) combinations, (\d+) layouts, (\d+) skipped", out.stdout)
    assert m and int(m.group(1)) == N_COMBINATIONS and int(m.group(3)) * 4 <= int(m.group(2)), out.stdout
    p = re.search(r"(\d+) layouts placed", out.stdout)
    assert p and int(p.group(1)) >= 37, out.stdout      # the floor the program derives from its inputs
    assert out.stdout.rstrip().endswith("ok")
