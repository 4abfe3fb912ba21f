"""Where the leftover kernels of the LDS sort classes run (big_pass in csrc/sh_classify.hip): by default each
k_sort_lds<c> goes to a side stream behind an event recorded after k_sort_top<c> and runs beside the next class's k_sort_top and the giant
kernels; SCRUBBY_HIP_SIDE=0 keeps it on the caller's stream.  Both orders must give the oracle's flags and the same statistics.

Workload: the tandem arrays of tests/test_giant_merge4_gpu.py (its generator, imported) with small copy numbers, so that the reads bring 65 to
4096 anchors and every LDS class has some.  SCRUBBY_HIP_TOPBT_MAX=1 makes k_sort_top settle only the reads with a single candidate at their
top score: tandem reads have many, so most of them are left to k_sort_lds - the path under test is busy in every class.  The two orders are
SCRUBBY_HIP_SIDE=0 and =2: a batch this small takes the side-by-side mode of whole classes by default, under which the leftovers stay with
their class; 2 is what a large batch gets by default.
Trace mode has no k_sort_top: there the order is the old one under either setting, and the traces must equal the oracle's."""
import numpy as np
import pytest

import tests.test_giant_merge4_gpu as G
from tests.test_parity_gpu import assert_trace_equal

pytestmark = pytest.mark.gpu

COPIES = (5, 8, 14, 20, 32, 45, 64, 90, 130)      # x ~22 minimizers of a 150-base read: ~110 .. ~2900 anchors, up to twice that for the 300-base reads
CLASS_BOUNDS = ((65, 256), (257, 512), (513, 1024), (1025, 2048), (2049, 4096))
STATS = ("n_dp_parallel", "n_top_settled", "n_clusters", "n_ext_reads")


@pytest.fixture(scope="module")
def S():
    from scrubby_amd import lib
    lib.require_gpu()
    return lib


@pytest.fixture(scope="module")
def tandem(S, oracle):
    saved = G.COPIES
    G.COPIES = COPIES      # tandem_workload() reads the module's tuple
    try:
        contigs, bases, offs = G.tandem_workload()
    finally:
        G.COPIES = saved
    cidx = oracle.Index.build(contigs, 11, 21)
    of, ot = cidx.classify(oracle.preset("sr"), bases, offs, threads=8)
    gidx = S.Index.build([bytes(c) for c in contigs], S.preset("sr"))
    return gidx, bases, offs, of, ot


def test_every_lds_class_has_reads(S, tandem):
    gidx, bases, offs, of, ot = tandem
    assert S.preset("sr").flags & S.SH_F_CIGAR      # the extension filter: flag-only calls hand chains over (k_sort_top runs)
    n = ot["n_anchor"].astype(np.int64)
    print("reads:", len(n), "anchors per read:", sorted(int(v) for v in n))
    assert 90 <= len(n) <= 130
    for lo, hi in CLASS_BOUNDS:
        assert int(((n >= lo) & (n <= hi)).sum()) >= 3, f"fewer than three reads of {lo}..{hi} anchors"


def test_flags_and_statistics_do_not_depend_on_where_the_leftovers_run(S, tandem, monkeypatch):
    gidx, bases, offs, of, ot = tandem
    monkeypatch.setenv("SCRUBBY_HIP_TOPBT_MAX", "1")
    out = {}
    for aside in ("0", "2"):
        monkeypatch.setenv("SCRUBBY_HIP_SIDE", aside)      # read at every call: 0 the old order, 2 the leftovers aside
        for rep in range(2):      # the second call finds the side stream already chosen
            f, _, st, rc = gidx.classify(bases, offs, want_trace=False)
            assert rc == 0 and np.array_equal(f, of), f"SIDE={aside}, call {rep}: {int((f != of).sum())} flags differ from the oracle's"
            print(f"SIDE={aside}:", {k: st[k] for k in STATS})
            assert st["n_top_settled"] < st["n_dp_parallel"], st      # reads were left to k_sort_lds
            out.setdefault(aside, []).append({k: st[k] for k in STATS})
    assert out["0"][0] == out["0"][1] == out["2"][0] == out["2"][1], out
    assert out["2"][0]["n_clusters"] > 0


def test_trace_mode_keeps_its_order_and_equals_the_oracle(S, tandem, monkeypatch):
    gidx, bases, offs, of, ot = tandem
    monkeypatch.setenv("SCRUBBY_HIP_TOPBT_MAX", "1")
    got = {}
    for aside in ("0", "2"):
        monkeypatch.setenv("SCRUBBY_HIP_SIDE", aside)
        gf, gt, st, rc = gidx.classify(bases, offs, want_trace=True)
        assert rc == 0 and st["n_top_settled"] == 0      # no read-level backtrack in trace mode
        assert_trace_equal(S, gf, gt, of, ot)
        got[aside] = {k: st[k] for k in STATS}
    assert got["0"] == got["2"], got
