"""A classify context (sh_ctx, scrubby_amd/csrc/sh_classify.hip) gives back what it took: device memory after create / destroy cycles, after
creations that fail half-way (an arena too small for its fixed part) and the status and message of a creation refused after the context
object exists (SH_F_CIGAR against an index without reference bases); and the members made on demand (d_lkind, regrown by a larger call;
d_coop and the side streams, made by the first call that needs them) live through reuse and go with the context.

The bound on the drop in free memory over four cycles: half of the smallest buffer a forgotten free would leak - d_records of a context
for 65536 reads is 65536 x 192 x 16 B = 201 MB, 800 MB over four cycles."""
import ctypes as C
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CONTIGS = [300_000, 200_000]
BOUND = 100 << 20
SH_ERR_OOM, SH_ERR_INDEX = 5, 9


@pytest.fixture(scope="module")
def S():
    from scrubby_amd import lib
    lib.require_gpu()
    return lib


@pytest.fixture(scope="module")
def ref(oracle):
    Po = oracle.ref_params(0x5C2B0C01, CONTIGS)
    r = oracle.synth_ref(Po, 0, Po.genome_len)
    return Po, [r[Po.contig_start[i]:Po.contig_start[i + 1]] for i in range(len(CONTIGS))]


@pytest.fixture(scope="module")
def indexes(S, ref):
    Po, seqs = ref
    return {p: S.Index.build([bytes(s) for s in seqs], S.preset(p)) for p in ("sr", "map-ont")}


def _opts(S, preset, cigar):
    o = S.preset(preset)
    o.flags = S.SH_F_CIGAR if cigar else 0
    return o


def _create(S, idx, opts, max_reads, max_len):
    h = C.c_void_p()
    rc = S.load().sh_ctx_create(idx.h, C.byref(opts), max_reads, max_reads * max_len, max_len, C.byref(h))
    return rc, h, S.load().sh_last_error().decode(errors="replace")


def _free_bytes():
    import torch
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


CONTEXTS = [("sr", False, 65536, 150), ("sr", True, 65536, 150), ("map-ont", True, 64, 20000)]


@pytest.mark.parametrize("preset,cigar,max_reads,max_len", CONTEXTS, ids=["sr-flag-only", "sr-cigar", "map-ont-cigar"])
def test_create_and_destroy_return_device_memory(S, indexes, preset, cigar, max_reads, max_len):
    o = _opts(S, preset, cigar)
    free0 = None
    for cycle in range(5):      # the first one warms up (code objects, the runtime's own pools)
        rc, h, msg = _create(S, indexes[preset], o, max_reads, max_len)
        assert rc == 0, msg
        assert S.load().sh_ctx_destroy(h) == 0
        if cycle == 0:
            free0 = _free_bytes()
    drop = free0 - _free_bytes()
    print(f"free device memory fell by {drop / 2**20:.1f} MiB over four create / destroy cycles ({preset}, cigar={cigar})")
    assert drop < BOUND


@pytest.mark.parametrize("cigar", [False, True], ids=["flag-only", "cigar"])
def test_failed_create_returns_device_memory(S, indexes, monkeypatch, cigar):
    """An arena of 1 MiB: its fixed part alone (40 B per read of 65536) does not fit, after a dozen buffers have been allocated."""
    monkeypatch.setenv("SCRUBBY_HIP_ARENA_MB", "1")
    o = _opts(S, "sr", cigar)
    free0 = None
    for attempt in range(5):
        rc, h, msg = _create(S, indexes["sr"], o, 65536, 150)
        assert rc == SH_ERR_OOM and not h.value
        assert "arena of 1 MiB is too small" in msg, msg
        if attempt == 0:
            free0 = _free_bytes()
    drop = free0 - _free_bytes()
    print(f"free device memory fell by {drop / 2**20:.1f} MiB over four failed creations (cigar={cigar})")
    assert drop < BOUND


def test_cigar_context_on_an_index_without_reference_bases_is_refused(S, indexes, tmp_path):
    """The index file is rewritten without its last section, the 4-bit reference (CacheHeader of sh_api.hip: has_ref is the uint32 at byte 28)."""
    p = str(tmp_path / "sr.idx")
    indexes["sr"].save(p)
    raw = bytearray(open(p, "rb").read())
    assert raw[:8] == b"SHIDX002" and struct.unpack_from("<I", raw, 28)[0] == 1
    n_bases = sum(CONTIGS)
    struct.pack_into("<I", raw, 28, 0)
    open(p, "wb").write(raw[: len(raw) - 8 * ((n_bases + 31) // 32) * 2])
    bare = S.Index.load(p, S.preset("sr"))
    rc, h, msg = _create(S, bare, _opts(S, "sr", True), 4096, 150)
    assert rc == SH_ERR_INDEX and not h.value
    assert "this index holds no reference bases" in msg, msg
    rc, h, msg = _create(S, bare, _opts(S, "sr", False), 4096, 150)      # flag-only needs none
    assert rc == 0, msg
    assert S.load().sh_ctx_destroy(h) == 0
    bare.close()


def test_members_made_on_demand_survive_reuse(S, oracle, ref, indexes):
    """Two calls on one map-ont context for 256 reads, 40 reads and then 200.  The per-read path record (d_lkind) is sized n + n / 8 + 64 by the
    call that makes it: 109 entries after the first call, so the second one drops it from the context's owner and allocates a larger one;
    the first call makes the cooperative join's queue and the side streams.  Flags equal the oracle's both times, the path lists can be
    read after each call, and destroying the context afterwards releases the regrown record once."""
    import torch
    Po, seqs = ref
    Ro = oracle.read_params(0x5C2B0C02, read_len=0, host_pct=60, sub_per_10k=300, n_read_pct=0)
    calls = (40, 200)
    assert calls[1] > calls[0] + calls[0] // 8 + 64      # the second call outgrows what the first one allocated
    bases, offs = oracle.synth_long_reads(Po, Ro, 0, calls[1])
    cidx = oracle.Index.build(seqs, 10, 15)
    of, _ = cidx.classify(cidx.update_opts(oracle.preset("map-ont")), bases, offs, threads=8)
    max_len = max(20000, int(np.diff(offs.astype(np.int64)).max()))
    ctx = S.Context(indexes["map-ont"], 256, len(bases), max_len)
    d_bases = torch.from_numpy(np.concatenate([bases, np.zeros(64, np.uint8)])).cuda()
    d_off = torch.from_numpy(offs.astype(np.int64)).cuda()
    for n in calls:
        fl = torch.zeros(n, dtype=torch.uint8, device="cuda")
        ctx.classify(d_bases[: len(bases)], d_off[: n + 1], fl, None)
        assert np.array_equal(fl.cpu().numpy(), of[:n])
        for which in range(3, 11):
            ids = ctx.debug_list(which)
            assert len(ids) <= n and (len(ids) == 0 or int(ids.max()) < n)
    ctx.close()
