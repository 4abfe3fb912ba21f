"""The giant reads' four-way merge passes (k_giant_split / k_giant_merge4, scrubby_amd/csrc/sh_merge4.h) through the public API, against the
CPU oracle and against the two-way rounds the same kernels give with SCRUBBY_HIP_GIANT_FANIN=2.

Reference: tandem arrays of one random 171-bp monomer each, with a sprinkle of substitutions and unique flanks; the copy numbers set the
anchors a read brings (minimizers of the read x copies that still carry them), from ~5 k to beyond 131 072, so that the giants' tile counts
ceil(n / 2048) cover a last group of one, two, three and four runs and one, two, three and four passes.  The arrays beyond mid_occ copies
reach the sort through the max_occ re-chaining, like the satellite reads of the bench.  A giant read has more than 4096 anchors (SORT_LDS_C),
hence three tiles at least: a giant of two tiles does not exist, and the smallest bucket asked for is {3}."""
import numpy as np
import pytest

from tests.test_parity_gpu import assert_trace_equal

pytestmark = pytest.mark.gpu

COPIES = (230, 330, 420, 700, 1500, 4000, 4800)
BUCKETS = ((3, 3), (4, 4), (5, 8), (9, 16), (17, 64), (65, 256))
_COMP = np.zeros(256, np.uint8)
for _a, _b in zip(b"ACGT", b"TGCA"):
    _COMP[_a] = _b


@pytest.fixture(scope="module")
def S():
    from scrubby_amd import lib
    lib.require_gpu()
    return lib


def tandem_workload():
    """contigs, read bases, offsets"""
    rng = np.random.default_rng(0x6A4)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    contigs, reads = [], []
    for cn in COPIES:
        mono = acgt[rng.integers(0, 4, 171)]
        arr = np.tile(mono, cn)
        hit = rng.random(len(arr)) < 0.004                                  # the sprinkle: copies differ, most k-mers survive
        arr[hit] = acgt[rng.integers(0, 4, int(hit.sum()))]
        ctg = np.concatenate([acgt[rng.integers(0, 4, 3000)], arr, acgt[rng.integers(0, 4, 3000)]])
        contigs.append(ctg)
        for i in range(8):                                                   # different phases, both strands, lengths: n varies
            length = (150, 150, 150, 120, 100, 150, 250, 300)[i]
            s = 3000 + (cn // 3) * 171 + 19 * i + int(rng.integers(0, 171))
            r = ctg[s:s + length]
            reads.append(_COMP[r][::-1] if i & 1 else r)
        for i in range(2):                                                   # an internal duplication: equal x in different runs
            s = 3000 + (cn // 2) * 171 + 40 * i
            reads.append(np.concatenate([ctg[s:s + 60], ctg[s + 15:s + 60], ctg[s + 60:s + 105]]))
        s = 3000 - 70                                                        # across the flank into the array
        reads.append(ctg[s:s + 150])
    for _ in range(12):
        reads.append(acgt[rng.integers(0, 4, 150)])                          # non-host
    offs = np.zeros(len(reads) + 1, np.uint64)
    offs[1:] = np.cumsum([len(r) for r in reads])
    return contigs, np.ascontiguousarray(np.concatenate(reads)), offs


@pytest.fixture(scope="module")
def tandem(S, oracle):
    contigs, bases, offs = tandem_workload()
    cidx = oracle.Index.build(contigs, 11, 21)
    of, ot = cidx.classify(oracle.preset("sr"), bases, offs, threads=8)
    gidx = S.Index.build([bytes(c) for c in contigs], S.preset("sr"))
    return gidx, bases, offs, of, ot


def test_tile_counts_cover_every_group_and_pass_shape(S, tandem):
    gidx, bases, offs, of, ot = tandem
    gf, gt, st, rc = gidx.classify(bases, offs, want_trace=True)
    assert rc == 0
    n = gt["n_anchor"].astype(np.int64)
    tiles = -(-n[n > 4096] // 2048)
    print("giant reads:", len(tiles), "tile counts:", sorted(set(int(t) for t in tiles)))
    for lo, hi in BUCKETS:
        assert ((tiles >= lo) & (tiles <= hi)).any(), f"no giant read of {lo}..{hi} tiles: {sorted(set(int(t) for t in tiles))}"
    assert int(ot["rechained"].sum()) > 0 and int((ot["rechained"][n > 4096] != 0).sum()) > 0      # giants that came through max_occ
    # the oracle handled every read: all 11 reads of every array map, none of the 12 random ones does
    assert len(of) == len(offs) - 1 == 11 * len(COPIES) + 12 and of[:11 * len(COPIES)].all() and not of[11 * len(COPIES):].any()


@pytest.mark.parametrize("fanin", ["4", "2"])
def test_trace_and_flags_equal_the_oracle(S, tandem, monkeypatch, fanin):
    gidx, bases, offs, of, ot = tandem
    monkeypatch.setenv("SCRUBBY_HIP_GIANT_FANIN", fanin)      # read at every launch
    gf, gt, st, rc = gidx.classify(bases, offs, want_trace=True)
    assert rc == 0
    assert_trace_equal(S, gf, gt, of, ot)
    f1, _, st1, rc = gidx.classify(bases, offs, want_trace=False)
    assert rc == 0 and np.array_equal(f1, of), f"{int((f1 != of).sum())} flags differ in flag-only mode"


def test_fan_in_4_and_2_are_identical(S, tandem, monkeypatch):
    gidx, bases, offs, of, ot = tandem
    out = {}
    for fanin in ("4", "2"):
        monkeypatch.setenv("SCRUBBY_HIP_GIANT_FANIN", fanin)
        gf, gt, st, rc = gidx.classify(bases, offs, want_trace=True)
        f1, _, st1, rc1 = gidx.classify(bases, offs, want_trace=False)
        assert rc == 0 and rc1 == 0
        out[fanin] = (gf, gt, f1)
    assert np.array_equal(out["4"][0], out["2"][0]) and np.array_equal(out["4"][2], out["2"][2])
    for name in S.TRACE_FIELDS:
        assert np.array_equal(out["4"][1][name], out["2"][1][name]), name


def test_long_reads_through_the_giant_sort(S, oracle):
    """200 stand-in long reads, map-ont: host reads of thousands of anchors go through the same passes (at least one beyond 8192 anchors:
    two passes)."""
    contigs = [600_000, 400_000]      # few, large repeat families: the reads that cross them bring thousands of anchors
    Po = oracle.ref_params(0x5C2B0A01, contigs, sat_pct=10, rep_pct=70, n_sat_fam=4, n_rep_fam=6)
    Ro = oracle.read_params(0x5C2B0021, host_pct=60, sub_per_10k=200, n_read_pct=1)
    n = 200
    bases, offs = oracle.synth_long_reads(Po, Ro, 11, n)
    ref = oracle.synth_ref(Po, 0, Po.genome_len)
    seqs = [ref[Po.contig_start[i]:Po.contig_start[i + 1]] for i in range(len(contigs))]
    gidx = S.Index.build([bytes(s) for s in seqs], S.preset("map-ont"))
    cidx = oracle.Index.build(seqs, 10, 15)
    oo = cidx.update_opts(oracle.preset("map-ont"))
    gf, gt, st, rc = gidx.classify(bases, offs, want_trace=True)
    of, ot = cidx.classify(oo, bases, offs, threads=8)
    assert_trace_equal(S, gf, gt, of, ot)
    assert int(ot["n_anchor"].max()) > 8192 and int((ot["n_anchor"] > 4096).sum()) >= 4, int(ot["n_anchor"].max())
