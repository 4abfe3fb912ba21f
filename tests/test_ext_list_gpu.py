"""The extension stage's list of reads that handed over a chain (k_ext_list: a wave lists slabs of 4096 reads with one atomic each), at
classify level: batches on both sides of a wave (63, 64, 65), one read, a slab's worth and one read more (4097: a second slab of one read),
in which every read hands over a chain, none does, or every other one.  Flags and the per-read trace against the oracle; the stage's counts
(reads listed, regions aligned) against what the oracle's trace says they are.  An empty list and a list of one are cases of their own."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CONTIGS = [300_000, 200_000]
SIZES = [1, 63, 64, 65, 1000, 4097]
POOL = 12000      # records synthesised once: about half are drawn from the reference


@pytest.fixture(scope="module")
def S():
    from scrubby_amd import lib
    lib.require_gpu()
    return lib


@pytest.fixture(scope="module")
def pool(oracle, S):
    """records, their oracle flags and trace (computed once), the device index, and which records hand over a chain"""
    P, R = oracle.ref_params(0x5C2B0021, CONTIGS), oracle.read_params(0x5C2B0022)
    ref = oracle.synth_ref(P, 0, P.genome_len)
    seqs = [ref[P.contig_start[i]:P.contig_start[i + 1]] for i in range(len(CONTIGS))]
    reads = np.asarray(oracle.synth_reads(P, R, 0, POOL)).reshape(POOL, R.read_len)
    off = np.arange(POOL + 1, dtype=np.uint64) * R.read_len
    of, ot = oracle.Index.build(seqs, 11, 21).classify(oracle.preset("sr"), reads.reshape(-1), off, threads=8)
    has = np.where(ot["n_chain"] > 0)[0]
    hasnt = np.where(ot["n_chain"] == 0)[0]
    assert len(has) >= max(SIZES) and len(hasnt) >= max(SIZES)
    return reads, of, ot, S.Index.build([bytes(s) for s in seqs], S.preset("sr")), has, hasnt


def _pick(pattern, n, has, hasnt):
    if pattern == "all":
        return has[:n]
    if pattern == "none":
        return hasnt[:n]
    sel = np.empty(n, np.int64)
    sel[0::2] = has[:(n + 1) // 2]
    sel[1::2] = hasnt[:n // 2]
    return sel


@pytest.mark.parametrize("pattern", ["all", "none", "alternating"])
@pytest.mark.parametrize("n", SIZES)
def test_batches_around_a_wave_and_a_slab(S, pool, n, pattern):
    reads, of, ot, gidx, has, hasnt = pool
    sel = _pick(pattern, n, has, hasnt)
    bases = np.ascontiguousarray(reads[sel]).reshape(-1)
    off = np.arange(n + 1, dtype=np.uint64) * reads.shape[1]
    gf, gt, st, rc = gidx.classify(bases, off, want_trace=True)
    assert rc == 0 and np.array_equal(gf, of[sel]), np.where(gf != of[sel])[0][:5]
    for name in S.TRACE_FIELDS:
        assert np.array_equal(gt[name], ot[name][sel]), name
    n_listed = int((ot["n_chain"][sel] > 0).sum())
    assert n_listed == {"all": n, "none": 0, "alternating": (n + 1) // 2}[pattern]
    assert st["n_ext_reads"] == n_listed and st["n_ext_regions"] == int(ot["n_aligned"][sel].sum())
    gf2, _, st2, rc2 = gidx.classify(bases, off, want_trace=False)      # flag-only: the list feeds k_ext_top
    assert rc2 == 0 and np.array_equal(gf2, of[sel])
    assert st2["n_ext_reads"] <= n_listed
