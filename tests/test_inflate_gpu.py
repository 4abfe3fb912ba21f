"""BGZF members inflated on the device (scrubby_amd/csrc/sh_inflate.hip through sh_inflate_members_device / sh_gunzip_bgzf): the valid
and corrupt members of tests/test_inflate_cpu.py, now through k_inflate_member.  Valid members must give zlib's bytes; corrupt ones must
end the call with SH_ERR_IO that names the member's file offset, and with the very status the host build of the same decoder gives for
the same bytes.  The output always lies between two guard bands of 4 KiB, which no call - the corrupt ones included - may touch.

The corrupt members are there for the clean error.  They run on the device only because the sanitizer program of test_inflate_cpu.py
is clean on the same bytes; a fault here is a finding about the bounds code, not something to repeat."""
import zlib

import numpy as np
import pytest

from tests import bgzf_util as B
from tests.test_deflate_gpu import fastq      # noqa: F401
from tests.test_inflate_cpu import OK, build_host, corrupt_cases, host_inflate, valid_cases

pytestmark = pytest.mark.gpu
GUARD = 4096
MAX_IN, MAX_OUT, MAX_MEMBERS = 4 << 20, 8 << 20, 1024


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
    inf = S.Inflater(MAX_IN, MAX_OUT, MAX_MEMBERS)
    yield inf
    inf.close()


def _members(S, file_bytes):
    ms, used, stopped = S.bgzf_scan(file_bytes)
    assert used == len(file_bytes) and stopped == 0
    return ms


def _device(S, inf, file_bytes, members):
    """(the bytes between the guard bands, stats or None, the error or None); both bands checked"""
    import torch
    total = sum(m.out_len for m in members)
    d_in = torch.frombuffer(bytearray(file_bytes), dtype=torch.uint8).cuda()
    buf = torch.full((total + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    st, err = None, None
    try:
        st = inf.inflate_members_device(d_in, members, buf[GUARD:], out_cap=total)
    except S.ScrubbyHipError as e:
        err = e
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[:GUARD] == 0xA5).all() and (got[GUARD + total:] == 0xA5).all(), "a guard band was written"
    return got[GUARD:GUARD + total].tobytes(), st, err


def test_valid_members_a_few_per_call(S, host, inflater, fastq):
    cases = valid_cases(host, fastq)
    kinds = [0, 0, 0]
    for o in range(0, len(cases), 4):
        group = cases[o:o + 4]
        file_bytes = b"".join(B.wrap(raw, data) for _, raw, data in group)
        members = _members(S, file_bytes)
        out, st, err = _device(S, inflater, file_bytes, members)
        assert err is None and all(m.status == OK for m in members), [n for n, _, _ in group]
        want = b"".join(data for _, _, data in group)
        assert out == want and st["n_members"] == len(group) and st["out_bytes"] == len(want), [n for n, _, _ in group]
        assert st["in_bytes"] == sum(len(raw) for _, raw, _ in group)
        kinds = [kinds[0] + st["n_stored_blocks"], kinds[1] + st["n_fixed_blocks"], kinds[2] + st["n_dynamic_blocks"]]
    assert all(kinds)


def test_three_hundred_members_through_host_memory(S, inflater, fastq):
    text = fastq * 4                                   # 4.3 MB of FASTQ in members of 14 336 bytes: ~1 MB compressed
    file_bytes = B.bgzf(text, block=14336)
    n = B.n_members(text, block=14336)
    assert 295 <= n <= 305 and 800_000 < len(file_bytes) < MAX_IN
    out, st = inflater.gunzip(file_bytes)
    assert out == text == b"".join(zlib.decompress(file_bytes[m.in_off:m.in_off + m.in_len], -15) for m in _members(S, file_bytes))
    assert st["n_members"] == n and st["out_bytes"] == len(text) and st["n_dynamic_blocks"] >= n - 1
    print(f"{n} members, {len(file_bytes)} -> {len(text)} bytes: {st['ms']:.3f} ms on the device")


def test_round_trip_with_the_device_encoder_and_members_out_of_order(S, inflater, fastq):
    df = S.Deflater(1 << 16, 65535)
    datas = [fastq[:1], fastq[100:100 + 32768], fastq[7:7 + 65535]]
    file_bytes = b"".join(B.wrap(df.deflate(d)[0], d) for d in datas)
    df.close()
    members = _members(S, file_bytes)
    order = [2, 0, 1]
    listed = [members[i] for i in order]               # member i's bytes go to the sum of out_len of those listed before it
    out, st, err = _device(S, inflater, file_bytes, listed)
    assert err is None and out == b"".join(datas[i] for i in order)
    assert inflater.gunzip(file_bytes)[0] == b"".join(datas)


def test_corrupt_members_end_with_the_host_decoders_status(S, host, inflater, fastq):
    good = fastq[:5000]
    first = B.member(good)
    for name, raw, isize, crc, want in corrupt_cases(fastq):
        host_status = host_inflate(host, raw, isize, crc)[0]
        assert host_status != OK and (want is None or host_status == want), name
        bad = B.wrap(raw, b"", crc=crc, isize=isize)
        file_bytes = first + bad
        members = _members(S, file_bytes)
        assert len(members) == 2 and members[1].file_off == len(first)
        out, st, err = _device(S, inflater, file_bytes, members)
        assert err is not None and err.status == 7, name
        assert str(len(first)) in err.message and S.INFLATE_STATUS[host_status] in err.message, (name, err.message)
        assert members[0].status == OK and members[1].status == host_status, (name, members[1].status, host_status)
        assert out[:len(good)] == good, name
    out, st = inflater.gunzip(first)                   # and the inflater still works
    assert out == good


def test_a_call_leaves_the_callers_current_device(S, fastq):
    """an inflater of the last visible device (another one than 0 where the box has several), used from a thread whose current device
    is 0: the bytes are right and the thread's device has not moved, through creation, a good call, a refused one and the release"""
    import torch
    other = torch.cuda.device_count() - 1
    torch.cuda.set_device(0)
    inf = S.Inflater(1 << 20, 1 << 20, 64, device=other)
    assert torch.cuda.current_device() == 0
    data = fastq[:150000]
    out, st = inf.gunzip(B.bgzf(data))
    assert out == data and st["n_members"] == 4 and torch.cuda.current_device() == 0
    with pytest.raises(S.ScrubbyHipError):
        inf.gunzip(B.bgzf(data, block=1000))      # 151 members: more than the 64 it was made for
    assert torch.cuda.current_device() == 0
    inf.close()
    assert torch.cuda.current_device() == 0


def test_refusals(S, inflater, fastq):
    import torch
    file_bytes = B.bgzf(fastq[:30000], block=10000)
    members = _members(S, file_bytes)
    d_in = torch.frombuffer(bytearray(file_bytes), dtype=torch.uint8).cuda()
    d_out = torch.zeros(30000, dtype=torch.uint8, device="cuda")
    with pytest.raises(S.ScrubbyHipError) as e:
        inflater.inflate_members_device(d_in, members, d_out, out_cap=29999)
    assert e.value.status == 1 and "29999" in e.value.message and "30000" in e.value.message
    with pytest.raises(S.ScrubbyHipError) as e:
        inflater.inflate_members_device(d_in, members * 300, d_out)
    assert e.value.status == 1 and str(len(members) * 300) in e.value.message and str(MAX_MEMBERS) in e.value.message
    far = S.GzMember(0, MAX_IN - 10, 11, 5, 0, 0)
    with pytest.raises(S.ScrubbyHipError) as e:
        inflater.inflate_members_device(d_in, [far], d_out)
    assert e.value.status == 1 and str(MAX_IN + 1) in e.value.message
    small = S.Inflater(1 << 20, 20000, 16)
    with pytest.raises(S.ScrubbyHipError) as e:
        small.inflate_members_device(d_in, members, d_out)
    assert e.value.status == 1 and "30000" in e.value.message and "20000" in e.value.message
    with pytest.raises(S.ScrubbyHipError) as e:
        small.gunzip(bytes(2 << 20), out_cap=0)
    assert e.value.status == 1 and str(2 << 20) in e.value.message
    small.close()
    with pytest.raises(S.ScrubbyHipError) as e:
        inflater.gunzip(file_bytes[:-5], out_cap=30000)      # the last member is cut short
    assert e.value.status == 7 and str(len(file_bytes) - 28) in e.value.message
    with pytest.raises(S.ScrubbyHipError) as e:
        S.Inflater(1 << 20, 1 << 20, 0)
    assert e.value.status == 1
    d_out.zero_()
    inflater.inflate_members_device(d_in, members, d_out)      # and the inflater still works
    assert d_out.cpu().numpy().tobytes() == fastq[:30000]
