"""Late anchors through the public API (csrc/sh_classify.hip): for a short read of more than 64 anchors k_expand
reserves the arena slots and lists the read, and the kernel that sorts the anchors - k_sort_top / k_sort_lds of its class, or
k_giant_chunksort per 2048-anchor tile - builds them in its LDS sort buffer (stage_anchors).  The option flag SH_F_NO_LATE_ANCHORS is the
path before: k_expand writes them to the arena and the sort kernels read them back.  Either way the sort sees the same anchors in the same
order, so flags, statistics and traces must be equal, and equal to the oracle's.  sh_stats.n_late_reads tells which way a call went (table
entries left to the sort kernels), sh_stats.n_deferred that reads were put off for want of arena room.

Workload: the tandem arrays of tests/test_giant_merge4_gpu.py (its generator, imported) with copy numbers that put reads into every LDS
class and the giant class; the arrays of 1500 and 2600 copies lie beyond mid_occ and reach the sort through the max_occ pass, whose filter
the sort kernels then apply themselves."""
import numpy as np
import pytest

import tests.test_giant_merge4_gpu as G
from tests.test_parity_gpu import assert_trace_equal

pytestmark = pytest.mark.gpu

COPIES = (5, 8, 14, 20, 32, 45, 64, 90, 130, 330, 700, 1500, 2600)
CLASS_BOUNDS = ((65, 256), (257, 512), (513, 1024), (1025, 2048), (2049, 4096), (4097, 1 << 30))
STATS = ("n_anchors", "n_clusters", "n_dp_parallel", "n_top_settled", "n_ext_reads", "n_ext_regions")


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


def test_every_class_has_reads_and_giants_come_through_max_occ(S, tandem):
    gidx, bases, offs, of, ot = tandem
    assert S.preset("sr").flags & S.SH_F_CIGAR      # the extension filter: flag-only calls hand chains over (k_sort_top runs)
    n = ot["n_anchor"].astype(np.int64)
    print("reads:", len(n), "anchors per read:", sorted(int(v) for v in n))
    for lo, hi in CLASS_BOUNDS:
        assert int(((n >= lo) & (n <= hi)).sum()) >= 3, f"fewer than three reads of {lo}..{hi} anchors"
    assert int((ot["rechained"][n > 4096] != 0).sum()) >= 3      # giants whose anchors the max_occ pass's filter admits
    assert of[:11 * len(COPIES)].all() and not of[11 * len(COPIES):].any()


def both_ways(gidx, S, call):
    """call(way) with late anchors (the default) and with SH_F_NO_LATE_ANCHORS (k_expand writes them to the arena)"""
    out = {}
    base = gidx.opts.flags
    try:
        for way in ("late", "arena"):
            gidx.opts.flags = base | S.SH_F_NO_LATE_ANCHORS if way == "arena" else base      # read at every call
            out[way] = call(way)
    finally:
        gidx.opts.flags = base
    return out


def flag_only(S, gidx, bases, offs, of, way, tag=""):
    f, _, st, rc = gidx.classify(bases, offs, want_trace=False)
    assert rc == 0 and np.array_equal(f, of), f"{way} {tag}: {int((f != of).sum())} flags differ from the oracle's"
    print(way, tag, {k: st[k] for k in STATS + ("n_late_reads", "n_deferred")})
    assert (st["n_late_reads"] > 0) == (way == "late"), st      # the path under test was taken / was not
    return st


def traced(S, gidx, bases, offs, of, ot, way):
    gf, gt, st, rc = gidx.classify(bases, offs, want_trace=True)
    assert rc == 0 and (st["n_late_reads"] > 0) == (way == "late"), st
    assert_trace_equal(S, gf, gt, of, ot)
    return gf, gt


def same_traces(S, a, b):
    assert np.array_equal(a[0], b[0])
    for name in S.TRACE_FIELDS:
        assert np.array_equal(a[1][name], b[1][name]), name


def test_flag_only_both_ways(S, tandem):
    gidx, bases, offs, of, ot = tandem
    out = both_ways(gidx, S, lambda way: flag_only(S, gidx, bases, offs, of, way))
    assert {k: out["late"][k] for k in STATS} == {k: out["arena"][k] for k in STATS}, out
    # five of the six classes are late and each has three reads at least (first test): tandem reads carry no singleton seed that could settle them before k_expand
    assert out["late"]["n_top_settled"] > 0 and out["late"]["n_late_reads"] >= 15, out["late"]


def test_trace_mode_both_ways(S, tandem):
    """no k_sort_top in trace mode: k_sort_lds builds the anchors of every class read"""
    gidx, bases, offs, of, ot = tandem
    out = both_ways(gidx, S, lambda way: traced(S, gidx, bases, offs, of, ot, way))
    same_traces(S, out["late"], out["arena"])


def test_leftovers_of_k_sort_top_both_ways_on_the_side_stream(S, tandem, monkeypatch):
    """SCRUBBY_HIP_TOPBT_MAX=1: k_sort_top settles few tandem reads, k_sort_lds builds the anchors of the others a second time; SCRUBBY_HIP_SIDE=2
    sends it to the side stream, the second call finds that stream already chosen"""
    gidx, bases, offs, of, ot = tandem
    monkeypatch.setenv("SCRUBBY_HIP_TOPBT_MAX", "1")
    monkeypatch.setenv("SCRUBBY_HIP_SIDE", "2")

    def call(way):
        sts = [flag_only(S, gidx, bases, offs, of, way, f"call {rep}") for rep in range(2)]
        assert {k: sts[0][k] for k in STATS} == {k: sts[1][k] for k in STATS}, sts
        assert sts[0]["n_top_settled"] < sts[0]["n_dp_parallel"], sts[0]      # reads were left to k_sort_lds
        return {k: sts[0][k] for k in STATS}, traced(S, gidx, bases, offs, of, ot, way)
    out = both_ways(gidx, S, call)
    assert out["late"][0] == out["arena"][0], (out["late"][0], out["arena"][0])
    same_traces(S, out["late"][1], out["arena"][1])


def test_deferred_reads_come_back_with_the_same_flags(S, tandem, monkeypatch):
    """An arena of 8 MiB (the value of test_small_arena_defers_and_still_matches): about 140 k anchor slots, more than the largest read here
    needs and far fewer than k_expand's waves reserve at 16 Ki a draw, so reads are deferred (n_deferred) and expanded again in a later
    iteration - listed late both times."""
    gidx, bases, offs, of, ot = tandem
    n = ot["n_anchor"].astype(np.int64)
    assert int(n.max()) < 120_000
    monkeypatch.setenv("SCRUBBY_HIP_ARENA_MB", "8")
    out = both_ways(gidx, S, lambda way: flag_only(S, gidx, bases, offs, of, way, "8 MiB"))
    assert out["late"]["n_deferred"] > 0 and out["arena"]["n_deferred"] > 0, out
    assert {k: out["late"][k] for k in STATS} == {k: out["arena"][k] for k in STATS}, out
