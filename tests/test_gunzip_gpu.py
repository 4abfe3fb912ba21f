"""Any gzip stream inflated on the device (sh_gunzip_* of scrubby_amd/csrc/sh_inflate.hip: k_gz_find, k_gz_size, k_gz_markers, k_gz_windows,
k_gz_resolve under shgz::feed), every feed behind the C ABI.  The streams are those of tests/test_gunzip_cpu.py; the bytes must be zlib's,
the output lies between two guard bands no call may touch, and the device must agree with the host mirror (tests/gunzip_host.cpp, the
same shgz::feed over loops of the same decoder) on the chunks it took, skipped and redid and on the members it saw.

The damaged and the cut stream are there for the clean error (SH_ERR_IO naming an offset); the same kinds of stream go through the
sanitizer program of test_gunzip_cpu.py, which checks the bounds of the code both paths share."""
import zlib

import numpy as np
import pytest

from tests.test_deflate_gpu import fastq      # noqa: F401
from tests.test_gunzip_cpu import FEED_OK, FEED_ROUNDS, build_host, damaged, gz, host_find, host_run, streams, wrong_starts, zlib_read

pytestmark = pytest.mark.gpu
GUARD = 4096
MAX_IN, MAX_OUT = 2 << 20, 4 << 20
AGREE = ("n_chunks", "n_skipped", "n_redone", "n_members")


@pytest.fixture(scope="module")
def S():
    from scrubby_amd import lib
    lib.require_gpu()
    return lib


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_host(tmp_path_factory)


@pytest.fixture(scope="module")
def inflater(S):
    inf = S.Inflater(MAX_IN, MAX_OUT, 16)
    yield inf
    inf.close()


def device_run(S, inf, file_bytes, chunk, step=0, out_cap=MAX_OUT):
    """as host_run of test_gunzip_cpu.py, through sh_gunzip_feed_device -> (status or the error, bytes, counts summed over the feeds)"""
    import torch
    d_file = torch.frombuffer(bytearray(file_bytes or b"\0"), dtype=torch.uint8).cuda()
    buf = torch.full((out_cap + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    g = inf.gunzip_open(chunk)
    got, total, rc = [], {}, 0
    lo, hi = 0, min(step, len(file_bytes)) if step else len(file_bytes)
    try:
        while True:
            last = hi == len(file_bytes)
            try:
                rc, consumed, out_len, st = g.feed_device(d_file[lo:], hi - lo, last, buf[GUARD:], out_cap=out_cap)
            except S.ScrubbyHipError as e:
                rc, consumed, out_len, st = e, 0, 0, {}
            torch.cuda.synchronize()
            back = buf.cpu().numpy()
            assert (back[:GUARD] == 0xA5).all() and (back[GUARD + out_cap:] == 0xA5).all(), "a guard band was written"
            got.append(back[GUARD:GUARD + out_len].tobytes())
            for name, v in st.items():
                total[name] = max(total.get(name, 0), v) if name == "n_rounds" else total.get(name, 0) + v
            lo += consumed
            if rc != 0 or (last and (lo == hi or (consumed == 0 and out_len == 0))):
                break
            if not last:
                hi = min(len(file_bytes), hi + step)
    finally:
        g.close()
    return rc, b"".join(got), total


def check_agree(S, host, inf, name, file_bytes, chunk, **kw):
    ok, want = zlib_read(file_bytes)
    rc, got, st = device_run(S, inf, file_bytes, chunk, **kw)
    assert ok and rc == 0 and got == want, (name, rc, len(got), len(want))
    hrc, hgot, hst, _ = host_run(host, file_bytes, chunk, **kw)
    assert hrc == FEED_OK and hgot == want
    assert {k: st[k] for k in AGREE} == {k: hst[k] for k in AGREE}, (name, st, hst)
    assert st["n_marker_symbols"] == hst["n_marker_symbols"] and st["out_bytes"] == len(want)
    return st


@pytest.mark.parametrize("level", [1, 6, 9])
def test_fastq_in_one_feed_and_in_feeds_of_100_000_bytes(S, host, inflater, fastq, level):
    file_bytes = gz(fastq, level)
    for chunk in (1024, 16384):
        st = check_agree(S, host, inflater, f"level {level}, chunks of {chunk}", file_bytes, chunk)
        assert st["n_chunks"] > 1 and st["n_marker_symbols"] > 0
        print(f"level {level}, chunks of {chunk}: find {st['ms_find']:.2f} size {st['ms_size']:.2f} markers {st['ms_markers']:.2f} windows {st['ms_windows']:.2f} "
              f"resolve {st['ms_resolve']:.2f} ms, {st['ms']:.2f} ms in all")
        st = check_agree(S, host, inflater, f"level {level}, chunks of {chunk}, in feeds", file_bytes, chunk, step=100000, out_cap=300000)
        assert st["n_chunks"] > 1 and st["n_marker_symbols"] > 0


def test_flushes_stored_members_fields_repeats_and_tails(S, host, inflater, fastq):
    for name, file_bytes, chunk in streams(fastq):
        st = check_agree(S, host, inflater, name, file_bytes, chunk)
        if name.startswith("three members"):
            assert st["n_members"] == 3


def test_through_host_memory(S, inflater, fastq):
    file_bytes = gz(fastq, 6)
    g = inflater.gunzip_open(4096)
    rc, consumed, out, st = g.feed(file_bytes, True, MAX_OUT)
    g.close()
    assert rc == 0 and consumed == len(file_bytes) and out == fastq and st["n_members"] == 1


def test_wrong_starts_are_redone(S, host, inflater, fastq):
    import torch
    file_bytes, chunk = gz(fastq, 1), 4096
    found = host_find(host, file_bytes, chunk)
    starts, n_wrong = wrong_starts(found, chunk)
    d_in = torch.frombuffer(bytearray(file_bytes), dtype=torch.uint8).cuda()
    buf = torch.full((len(fastq) + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    out_len, st = inflater.gunzip_starts(d_in, starts, buf[GUARD:], chunk_bytes=chunk, out_cap=len(fastq))
    torch.cuda.synchronize()
    back = buf.cpu().numpy()
    assert (back[:GUARD] == 0xA5).all() and (back[GUARD + len(fastq):] == 0xA5).all()
    assert out_len == len(fastq) and back[GUARD:GUARD + out_len].tobytes() == fastq
    hst = host_run(host, file_bytes, chunk, starts=starts)[2]
    assert n_wrong >= 3 and st["n_redone"] >= n_wrong and {k: st[k] for k in AGREE} == {k: hst[k] for k in AGREE}, (st, hst)
    # the device's own find gives the starts the host's gives
    out_len, plain = inflater.gunzip_starts(d_in, found, buf[GUARD:], chunk_bytes=chunk, out_cap=len(fastq))
    rc, got, own = device_run(S, inflater, file_bytes, chunk)
    assert rc == 0 and got == fastq and {k: own[k] for k in AGREE} == {k: plain[k] for k in AGREE}


def test_a_damaged_and_a_cut_stream_are_io_errors(S, host, inflater, fastq):
    file_bytes = gz(fastq[:120000])
    bad = bytearray(file_bytes)
    bad[len(bad) // 2] ^= 0x10
    for name, data in (("damaged", bytes(bad)), ("cut", file_bytes[:len(file_bytes) * 2 // 3])):
        assert not zlib_read(data)[0] and host_run(host, data, 1024)[0] not in (FEED_OK, FEED_ROUNDS), name      # the sanitizer program's kind of stream
        rc, got, st = device_run(S, inflater, data, 1024)
        assert isinstance(rc, S.ScrubbyHipError) and rc.status == 7 and got == b"", (name, rc)
        assert "offset" in rc.message
    assert device_run(S, inflater, file_bytes, 1024)[1] == fastq[:120000]      # and the inflater still works


def test_fixed_blocks_are_the_fallback_status(S, host, inflater, fastq):
    file_bytes = gz(fastq, 6, zlib.Z_FIXED)
    rc, got, st = device_run(S, inflater, file_bytes, 4096)
    hrc, hgot, hst, _ = host_run(host, file_bytes, 4096)
    assert rc == S.SH_GUNZIP_FALLBACK and hrc == FEED_ROUNDS and got == hgot and fastq.startswith(got) and len(got) > 0


def test_refusals_and_where_the_scratch_is_taken(S, fastq):
    import torch
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    inf = S.Inflater(1 << 20, 64 << 20, 16)
    free1 = torch.cuda.mem_get_info()[0]
    assert free0 - free1 < (16 << 20), "the inflater takes the marker scratch before any sh_gunzip_open"
    g = inf.gunzip_open(16384)
    free2 = torch.cuda.mem_get_info()[0]
    assert free1 - free2 >= (128 << 20)      # 2 B per byte of max_out_bytes
    with pytest.raises(S.ScrubbyHipError) as e:
        g.feed(gz(fastq[:100000]), True, 1000)
    assert e.value.status == 1 and "1000" in e.value.message
    rc, consumed, out, st = g.feed(gz(fastq[:100000]), True, 1 << 20)      # a refusal for room leaves the stream open
    assert rc == 0 and out == fastq[:100000]
    g.close()
    for chunk in (512, (1 << 20) + 1):
        with pytest.raises(S.ScrubbyHipError) as e:
            inf.gunzip_open(chunk)
        assert e.value.status == 1
    inf.close()
