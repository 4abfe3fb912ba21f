"""k_pair_pass mode 2 with the middle check, and SmallStore's register table of group words.

Reads cut from the cfg1 mini reference with substitutions placed so that their seeds are co-diagonal singletons with ONE gap (or
more) that leaves more than ext_unc_max = zdrop / b = 12 bases outside the exact k-mers: the pair pass has to look at the bases
(mm_test_zdrop over the ungapped stretch) and decides the read if there is no z-drop; a read whose stretch does drop stays on the
list and ends with the oracle's flag through k_chain_small and the extension stage.  Flags are compared with the CPU oracle's."""
import numpy as np
import pytest

from tests import workloads as W

pytestmark = pytest.mark.gpu

COMP = bytes.maketrans(b"ACGT", b"TGCA")
READ_LEN = 150
N_PER_VARIANT = 400


def _subst(b):
    return b"CGTA"[b"ACGT".index(bytes([b]))] if bytes([b]) in (b"A", b"C", b"G", b"T") else ord("A")


def cut_reads(ref, n, seed, positions):
    """n reads of READ_LEN bases cut from ref at seeded places, the bases at `positions` (in reference orientation) substituted, odd reads
    reverse-complemented."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        s = int(rng.integers(0, len(ref) - READ_LEN))
        r = bytearray(ref[s:s + READ_LEN].tobytes().upper())
        for p in positions:
            r[p] = _subst(r[p])
        r = bytes(r)
        if i & 1:
            r = r.translate(COMP)[::-1]
        out.append(r)
    return out


# what each variant changes (offsets in the read as cut).  Three substitutions leave a 150-base read at least four seeds (one of the four
# exact blocks has 37 bases or more, and every block of 31 holds a whole minimizer window), so the reads with two seeds only, a span
# below k and the unmapped outcomes come from the last variant: five substitutions 26 bases apart, exact blocks of 25 bases.
# stretch_every_second is beyond what a 30-base stretch can show with the sr scores
# (a = 2, b = 8, zdrop = 100: ten substitutions among thirty bases drop the score by 40) - 36 bases with every second one changed
# drop it by 18 * 8 - 18 * 2 = 108 > zdrop, so the middle check fails there and the read takes the full path
VARIANTS = {
    "exact": [],
    "one_sub": [75],
    "two_subs": [55, 95],
    "three_subs": [40, 75, 110],
    "stretch_every_third": list(range(60, 90, 3)),
    "stretch_every_second": list(range(57, 93, 2)),
    "five_subs_sparse": list(range(25, 150, 26)),
}


def to_batch(recs):
    bases = np.frombuffer(b"".join(recs), dtype=np.uint8)
    offs = np.zeros(len(recs) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(x) for x in recs])
    return bases, offs


def many_group_reads(seqs, n, seed, piece=36):
    """reads glued from one short piece of every (contig, strand) of the reference, in seeded order: 2 * len(seqs) anchor groups in a read
    of few anchors"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        parts = []
        for ci in range(len(seqs)):
            for rev in (0, 1):
                s = int(rng.integers(0, len(seqs[ci]) - piece))
                p = seqs[ci][s:s + piece].tobytes().upper()
                parts.append(p.translate(COMP)[::-1] if rev else p)
        order = rng.permutation(len(parts))
        out.append(b"".join(parts[j] for j in order))
    return out


@pytest.fixture(scope="module")
def S():
    from scrubby_amd import lib
    lib.require_gpu()
    return lib


@pytest.fixture(scope="module")
def cfg1(oracle):
    return W.cfg1(oracle, 16)


@pytest.fixture(scope="module")
def gpu_index(S, cfg1):
    P, R, ref, seqs, reads, off = cfg1
    return S.Index.build([bytes(s) for s in seqs], S.preset("sr"))


@pytest.fixture(scope="module")
def cpu_index(oracle, cfg1):
    P, R, ref, seqs, reads, off = cfg1
    return oracle.Index.build(seqs, 11, 21)


@pytest.fixture(scope="module")
def variants(oracle, cfg1, cpu_index):
    """name -> (bases, offsets, oracle flags, oracle trace), computed once"""
    P, R, ref, seqs, reads, off = cfg1
    out = {}
    for vi, (name, pos) in enumerate(VARIANTS.items()):
        bases, offs = to_batch(cut_reads(ref, N_PER_VARIANT, 100 + vi, pos))
        of, ot = cpu_index.classify(oracle.preset("sr"), bases, offs, threads=8)
        out[name] = (bases, offs, of, ot)
    return out


def test_substituted_reads_flags_equal_the_oracle(S, gpu_index, variants):
    """Every variant alone: flags equal the oracle's for every read, and the LDS path saw reads."""
    for name, (bases, offs, of, ot) in variants.items():
        gf, _, st, rc = gpu_index.classify(bases, offs, want_trace=False)
        print(name, {k: st[k] for k in ("n_host", "n_chain_small", "n_chain_large", "n_pair_decided", "n_ext_shortcut", "n_ext_reads")},
              "oracle mapped", int(of.sum()), "of", len(of))
        assert rc == 0
        assert np.array_equal(gf, of), f"{name}: {int((gf != of).sum())} flags differ"
        assert st["n_chain_small"] > 0, name
        if name == "five_subs_sparse":      # both outcomes, and reads of two seeds
            assert 0 < int(of.sum()) < len(of) and int((ot["n_seed"] == 2).sum()) > 0
        else:
            assert int(of.sum()) == len(of), name


def test_middle_check_decides_reads_in_the_pair_pass(S, gpu_index, variants, monkeypatch):
    """The four substituted variants in one batch.  The pair pass decides strictly more of them than it can without the middle check:
    SCRUBBY_HIP_NO_LEMMA=1 switches ext_lemma and with it the new branch off, and leaves the pair pass what it decides from the k-mers alone
    (every premise holds AND at most 12 bases lie outside the k-mers - the reads that fail nothing).  The difference is the new branch's
    work; the flags are the oracle's both times.  The count for exact copies of the same reads is printed beside it."""
    names = ["one_sub", "two_subs", "three_subs", "stretch_every_third"]
    bases = np.concatenate([variants[n][0] for n in names])
    offs = np.arange(len(bases) // READ_LEN + 1, dtype=np.uint64) * READ_LEN
    of = np.concatenate([variants[n][2] for n in names])
    keys = ("n_host", "n_chain_small", "n_pair_decided", "n_ext_shortcut", "n_ext_reads")
    gf, _, st, rc = gpu_index.classify(bases, offs, want_trace=False)
    assert rc == 0 and np.array_equal(gf, of)
    monkeypatch.setenv("SCRUBBY_HIP_NO_LEMMA", "1")
    g0, _, st0, rc = gpu_index.classify(bases, offs, want_trace=False)
    monkeypatch.delenv("SCRUBBY_HIP_NO_LEMMA")
    assert rc == 0 and np.array_equal(g0, of)
    eb, eo, ef, _ = variants["exact"]
    ge, _, ste, rc = gpu_index.classify(eb, eo, want_trace=False)
    assert rc == 0 and np.array_equal(ge, ef)
    print("substituted          ", {k: st[k] for k in keys})
    print("  without the check  ", {k: st0[k] for k in keys})
    print("exact copies (a 4th) ", {k: ste[k] for k in keys})
    assert st["n_chain_small"] > 0
    assert st["n_pair_decided"] > st0["n_pair_decided"], (st["n_pair_decided"], st0["n_pair_decided"])
    assert st["n_pair_decided"] + st["n_ext_shortcut"] >= st0["n_pair_decided"] + st0["n_ext_shortcut"]


def test_failed_middle_check_takes_the_full_path(S, gpu_index, variants):
    """36 bases with every second one substituted: the ungapped stretch z-drops, the pair pass must leave the read alone, and the
    extension stage gives the oracle's flag."""
    bases, offs, of, ot = variants["stretch_every_second"]
    gf, _, st, rc = gpu_index.classify(bases, offs, want_trace=False)
    assert rc == 0 and np.array_equal(gf, of)
    assert st["n_ext_reads"] > 0


def test_more_groups_than_the_register_table(S, oracle, cfg1, gpu_index, cpu_index):
    """Reads with 10 (strand, contig) groups and at most 32 anchors: ranks 8 and 9 lie beyond SmallStore's register table and are recomputed
    from the seeds.  Trace mode (every chain handed to the extension stage with its group word) field by field, flag-only (top chain and
    chain_lemma) by flag."""
    P, R, ref, seqs, reads, off = cfg1
    bases, offs = to_batch(many_group_reads(seqs, 200, 9))
    of, ot = cpu_index.classify(oracle.preset("sr"), bases, offs, threads=8)
    small = (ot["n_anchor"] <= 32) & (ot["rep_len"] == 0)
    print("reads of the LDS path:", int(small.sum()), "chains", int(ot["n_chain"][small].sum()), "mapped", int(of.sum()))
    assert int(small.sum()) >= 50 and int((ot["n_chain"][small] >= 4).sum()) >= 20      # the case is there: many chains a read, in LDS
    gf, gt, st, rc = gpu_index.classify(bases, offs, want_trace=True)
    assert rc == 0 and st["n_chain_small"] >= 50
    assert np.array_equal(gf, of), f"{int((gf != of).sum())} flags differ"
    for name in S.TRACE_FIELDS:
        bad = np.where(gt[name] != ot[name])[0]
        assert len(bad) == 0, f"trace.{name}: {len(bad)} differ, first read {bad[0]}: gpu={gt[name][bad[0]]} cpu={ot[name][bad[0]]}"
    f1, _, st1, rc = gpu_index.classify(bases, offs, want_trace=False)
    assert rc == 0 and np.array_equal(f1, of)
