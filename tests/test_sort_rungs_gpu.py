"""The rungs of k_sort_top (csrc/sh_sort_rungs.h, big_pass in csrc/sh_classify.hip, DESIGN.md section 3.3 "Rungs"): tables 3 and 4 of the LDS
sort classes are each served by two launches, (1024, 1600] / (1600, 2048] and (2048, 3264] / (3264, 4096], every one with a block sized to
the reads it takes and passing over the others' untouched.  A read on the wrong side of a bound would be sorted in a block too small for it
or by no launch at all (then k_sort_lds settles it and n_top_settled drops): so reads sit exactly on both sides of each bound.

Workload: the tandem arrays of tests/test_giant_merge4_gpu.py (its generator, imported) with 50, 64, 80 and 96 copies, and candidate reads
cut across an array's edge: `inside` bases of the array bring (minimizers x copies that still carry them) anchors, and every ~6 more bases
of the unique flank add one singleton - sweeping the flank part walks the count up one by one.  The rows below were settled on the CPU
oracle so that the sweep crosses 1024 | 1025 (the table bound below the rungs), 1600 | 1601 and 3264 | 3265; the test asks the oracle again
and asserts that every wanted count is there."""
import numpy as np
import pytest

import tests.test_giant_merge4_gpu as G
from tests.test_parity_gpu import assert_trace_equal

pytestmark = pytest.mark.gpu

COPIES = (50, 64, 80, 96)
# (array, edge, bases inside the array): the flank part sweeps 0, 3, .. 198 bases
ROWS = ((0, "right", 144), (0, "right", 240), (1, "left", 196), (2, "left", 248), (3, "right", 236))
FLANK = range(0, 200, 3)
WANTED = (1024, 1025, 1600, 1601, 3264, 3265)
RUNG_BOUNDS = ((1025, 1600), (1601, 2048), (2049, 3264), (3265, 4096))
STATS = ("n_dp_parallel", "n_top_settled", "n_clusters", "n_ext_reads")


@pytest.fixture(scope="module")
def S():
    from scrubby_amd import lib
    lib.require_gpu()
    return lib


def candidates():
    """contigs, reads: the generator's own reads of every array (all classes, both strands, non-host) and the edge sweeps"""
    saved = G.COPIES
    G.COPIES = COPIES      # tandem_workload() reads the module's tuple
    try:
        contigs, bases, offs = G.tandem_workload()
    finally:
        G.COPIES = saved
    reads = [bases[int(offs[i]):int(offs[i + 1])] for i in range(len(offs) - 1)]
    for ci, edge, inside in ROWS:
        ctg = contigs[ci]
        end = 3000 + COPIES[ci] * 171
        for j, fl in enumerate(FLANK):
            r = ctg[3000 - fl:3000 + inside] if edge == "left" else ctg[end - inside:end + fl]
            reads.append(G._COMP[r][::-1] if j & 1 else r)
    return contigs, reads


@pytest.fixture(scope="module")
def rung_reads(S, oracle):
    contigs, reads = candidates()
    cidx = oracle.Index.build(contigs, 11, 21)

    def run(rs):
        offs = np.zeros(len(rs) + 1, np.uint64)
        offs[1:] = np.cumsum([len(r) for r in rs])
        bases = np.ascontiguousarray(np.concatenate(rs))
        return bases, offs, cidx.classify(oracle.preset("sr"), bases, offs, threads=8)

    n_gen = 11 * len(COPIES) + 12
    _, _, (_, ot) = run(reads)
    n = ot["n_anchor"].astype(np.int64)
    # the hits: the generator's reads as they are, of the sweeps the reads of tables 2 .. 4 next to a bound or among the first of their rung
    keep = list(range(n_gen))
    for v in WANTED:
        keep += [int(i) for i in np.nonzero(n[n_gen:] == v)[0][:2] + n_gen]
    for lo, hi in RUNG_BOUNDS:
        keep += [int(i) for i in np.nonzero((n[n_gen:] >= lo) & (n[n_gen:] <= hi))[0][:6] + n_gen]
    keep = sorted(set(keep))
    bases, offs, (of, ot) = run([reads[i] for i in keep])
    gidx = S.Index.build([bytes(c) for c in contigs], S.preset("sr"))
    return gidx, bases, offs, of, ot


def test_reads_sit_on_both_sides_of_every_bound(S, rung_reads):
    gidx, bases, offs, of, ot = rung_reads
    assert S.preset("sr").flags & S.SH_F_CIGAR      # the extension filter: flag-only calls hand chains over (k_sort_top runs)
    n = ot["n_anchor"].astype(np.int64)
    print("reads:", len(n), "anchors per read:", sorted(int(v) for v in n))
    assert len(n) <= 130
    for v in WANTED:
        assert int((n == v).sum()) >= 1, f"no read of exactly {v} anchors"
    for lo, hi in RUNG_BOUNDS:
        assert int(((n >= lo) & (n <= hi)).sum()) >= 3, f"fewer than three reads of {lo}..{hi} anchors"


def test_flags_and_statistics_whichever_streams_the_rungs_run_on(S, rung_reads, monkeypatch):
    gidx, bases, offs, of, ot = rung_reads
    out = []
    for side in ("0", "1", "2"):      # everything on the caller's stream; the tables side by side, a table's rungs in order on its stream; leftovers aside
        monkeypatch.setenv("SCRUBBY_HIP_SIDE", side)      # read at every call
        for rep in range(2):
            f, _, st, rc = gidx.classify(bases, offs, want_trace=False)
            assert rc == 0 and np.array_equal(f, of), f"SIDE={side}, call {rep}: {int((f != of).sum())} flags differ from the oracle's"
            print(f"SIDE={side}:", {k: st[k] for k in STATS})
            assert st["n_top_settled"] > 0, st
            out.append({k: st[k] for k in STATS})
    assert all(o == out[0] for o in out), out


def test_flags_without_the_read_level_backtrack(S, rung_reads, monkeypatch):
    gidx, bases, offs, of, ot = rung_reads
    monkeypatch.setenv("SCRUBBY_HIP_NO_TOPBT", "1")      # no k_sort_top at all: k_sort_lds takes every table whole
    f, _, st, rc = gidx.classify(bases, offs, want_trace=False)
    assert rc == 0 and np.array_equal(f, of), f"{int((f != of).sum())} flags differ from the oracle's"
    assert st["n_top_settled"] == 0, st


def test_trace_mode_equals_the_oracle(S, rung_reads):
    gidx, bases, offs, of, ot = rung_reads
    gf, gt, st, rc = gidx.classify(bases, offs, want_trace=True)
    assert rc == 0 and st["n_top_settled"] == 0      # no read-level backtrack in trace mode
    assert_trace_equal(S, gf, gt, of, ot)
