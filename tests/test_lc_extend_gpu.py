"""k_local_cluster takes reads with seeds above mid_occ.  Flags against the CPU oracle, every read compared.
The reference is 400 kb of random bases with mid_occ / max_occ lowered to 12 / 40, so that a dozen copies make a seed "high":

  a 171-base monomer repeated 60 times, every copy with 3 % of its bases substituted.  Reads of 150 bases cut inside the array, as they are
  and with one substitution: the k-mers they share with the other copies lie above mid_occ, the private ones are singletons.

The statistics instance of the kernel (SCRUBBY_HIP_DBG=16) counts the reads decided although a seed of theirs is filtered in
sh_stats.n_lc_filtered.  The reads run as they come and with SCRUBBY_HIP_NO_LEMMA=1, which takes ext_lemma and with it the whole kernel away:
no read is decided that way then, and the flags are still the oracle's."""
import numpy as np
import pytest

from tests.test_pair_mid_gpu import cut_reads, to_batch

pytestmark = pytest.mark.gpu

REF_LEN = 400_000
MID_OCC, MAX_OCC = 12, 40
MONOMER, N_MONO, MONO_DIV = 171, 60, 0.03
ARRAY_AT = 50_000
MODES = {"off": ("SCRUBBY_HIP_NO_LEMMA",), "on": ()}


def _mutated(rng, seq, rate):
    acgt = np.frombuffer(b"ACGT", np.uint8)
    s = seq.copy()
    hit = rng.random(len(s)) < rate
    s[hit] = acgt[(np.searchsorted(acgt, s[hit]) + rng.integers(1, 4, int(hit.sum()))) % 4]
    return s


@pytest.fixture(scope="module")
def S():
    from scrubby_amd import lib
    lib.require_gpu()
    return lib


@pytest.fixture(scope="module")
def case(S, oracle):
    """the GPU index and (bases, offsets, oracle flags) of the reads"""
    rng = np.random.default_rng(0x1C5EED)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    ref = acgt[rng.integers(0, 4, REF_LEN)].copy()
    mono = acgt[rng.integers(0, 4, MONOMER)]
    array = np.concatenate([_mutated(rng, mono, MONO_DIV) for _ in range(N_MONO)])
    ref[ARRAY_AT:ARRAY_AT + len(array)] = array
    go, oo = S.preset("sr"), oracle.preset("sr")
    for o in (go, oo):
        o.mid_occ, o.max_occ = MID_OCC, MAX_OCC
        # mm_seed_mz_flt (minimizers that recur more than mid_occ times inside one read) has nothing to drop in these reads, but while it is on
        # the front end hands every read of more than mid_occ minimizers - with 12, every read here - to the legacy path: off in both
        o.q_occ_frac = 0.0
    gidx = S.Index.build([ref.tobytes()], go)
    cidx = oracle.Index.build([ref], 11, 21)
    inside = ref[ARRAY_AT:ARRAY_AT + len(array)]
    bases, offs = to_batch(cut_reads(inside, 300, 1, []) + cut_reads(inside, 300, 2, [75]))
    of, ot = cidx.classify(oo, bases, offs, threads=8)
    return gidx, (bases, offs, of)


@pytest.mark.parametrize("mode", list(MODES))
def test_array_reads_with_filtered_seeds(case, mode, monkeypatch):
    gidx, (bases, offs, of) = case
    monkeypatch.setenv("SCRUBBY_HIP_DBG", "16")
    for name in MODES[mode]:
        monkeypatch.setenv(name, "1")
    gf, _, st, rc = gidx.classify(bases, offs, want_trace=False)
    print(mode, {k: st[k] for k in ("n_host", "n_chain_small", "n_chain_large", "n_ext_shortcut", "n_lc_filtered", "n_ext_reads")},
          "oracle mapped", int(of.sum()), "of", len(of))
    assert rc == 0
    assert np.array_equal(gf, of), f"{mode}: {int((gf != of).sum())} flags differ"
    assert st["n_chain_large"] > 0
    if mode == "on":
        assert st["n_lc_filtered"] >= 1
    else:
        assert st["n_lc_filtered"] == 0
