"""Any gzip stream in parallel, on the host: tests/gunzip_host.cpp runs shgz::feed (scrubby_amd/csrc/sh_gunzip.h: chunks, the chain walk
with its rounds, layout, CRC-32 and ISIZE per member) over loops of the SHIN_FN code the kernels of sh_inflate.hip call (candidate test,
span decoder with the size and the marker sink, window step, resolve).  The expected bytes are always zlib's; for files with a tail or
with damage, what gzread makes of them (members one after another, a tail that is no gzip member ignored, anything else an error),
which is what shc::In gives for the same file today.

gunzip_host.cpp has a main of its own behind -DGUNZIP_MAIN: built with -fsanitize=address,undefined it is the sanitizer run of this
code, a stand-alone program on the CPU (the last test builds and runs it) over the same families of streams.

The streams are functions of this module: tests/test_gunzip_gpu.py sends the same ones through the device."""
import ctypes as C
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

from tests.test_deflate_gpu import fastq      # noqa: F401  (the varied-quality FASTQ text, about 1 MB)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "gunzip_host.cpp")
FEED_OK, FEED_ROUNDS, FEED_ENDS, FEED_DATA, FEED_TRUNCATED, FEED_NOT_GZIP, FEED_OUT_CAP, FEED_BACKEND = range(8)
COUNTS = ("n_chunks", "n_skipped", "n_redone", "n_rounds", "n_members", "n_marker_symbols", "n_window_steps", "in_bytes", "out_bytes")
NO_START = 2 ** 64 - 1
NEW_EXPORTS = ["sh_gunzip_open", "sh_gunzip_feed_device", "sh_gunzip_feed", "sh_gunzip_close", "sh_dbg_gunzip_starts"]
OUT_CAP = 4 << 20


def build_host(tmp_path_factory):
    d = tmp_path_factory.mktemp("gzh")
    so = str(d / "libgunzip_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, SRC])
    L = C.CDLL(so)
    L.gzh_open.restype = C.c_void_p
    L.gzh_open.argtypes = [C.c_uint32]
    L.gzh_close.argtypes = [C.c_void_p]
    L.gzh_max_rounds.restype = C.c_uint32
    L.gzh_feed.restype = C.c_int
    L.gzh_feed.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_void_p, C.c_void_p]
    L.gzh_find.restype = C.c_int
    L.gzh_find.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p]
    L.gzh_candidates.restype = C.c_int
    L.gzh_candidates.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
    return L


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_host(tmp_path_factory)


# ---- streams ---------------------------------------------------------------------------------------------------------------------------------
def gz(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=0, flush=zlib.Z_SYNC_FLUSH):
    """one gzip member by zlib, with a flush of that kind after flush_at bytes"""
    c = zlib.compressobj(level, zlib.DEFLATED, 31, 8, strategy)
    if flush_at:
        return c.compress(data[:flush_at]) + c.flush(flush) + c.compress(data[flush_at:]) + c.flush()
    return c.compress(data) + c.flush()


def gz_fields(data, level=6, extra=b"", name=None, comment=None, fhcrc=False):
    """one gzip member with the optional header fields"""
    flg = (4 if extra else 0) | (8 if name is not None else 0) | (16 if comment is not None else 0) | (2 if fhcrc else 0)
    h = bytes([0x1f, 0x8b, 8, flg, 0, 0, 0, 0, 0, 3])
    if extra:
        h += struct.pack("<H", len(extra)) + extra
    if name is not None:
        h += name + b"\0"
    if comment is not None:
        h += comment + b"\0"
    if fhcrc:
        h += struct.pack("<H", zlib.crc32(h) & 0xffff)
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return h + c.compress(data) + c.flush() + struct.pack("<II", zlib.crc32(data), len(data) & 0xffffffff)


def zlib_read(file_bytes):
    """(True, bytes) or (False, the bytes before the error): what gzread gives for the file"""
    out, rest, first = [], file_bytes, True
    while True:
        if len(rest) < 2 or rest[:2] != b"\x1f\x8b":
            return (not first or not file_bytes), b"".join(out)
        d = zlib.decompressobj(31)
        try:
            out.append(d.decompress(rest))
        except zlib.error:
            return False, b"".join(out)
        if not d.eof:
            return False, b"".join(out)
        rest, first = d.unused_data, False


def four_letters():
    unit = bytes(np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(5).integers(0, 4, 30000)])
    return unit * 40


def random_block():
    return np.random.default_rng(6).integers(0, 256, 20000, dtype=np.uint8).tobytes() * 100


def member_end_at_chunk_end(part, chunk=1024):
    plain = gz_fields(part, name=b"")
    first = gz_fields(part, name=b"n" * ((chunk - len(plain) % chunk) % chunk))
    assert len(first) % chunk == 0
    return first + gz(part)


def streams(text):
    """[(name, the file, chunk_bytes)]: every one must come back as zlib's bytes with no fallback"""
    part = text[:200000]
    fields = dict(extra=b"XY\x01\x00\x07", name=b"reads.fastq", comment=b"a comment", fhcrc=True)
    return [
        ("sync flush in mid-stream", gz(text, 6, flush_at=500000, flush=zlib.Z_SYNC_FLUSH), 4096),
        ("full flush in mid-stream", gz(text, 6, flush_at=500000, flush=zlib.Z_FULL_FLUSH), 4096),
        ("level 0, 1 KiB", gz(text, 0), 1024),
        ("level 0, 16 KiB", gz(text, 0), 16384),
        ("three members, one empty", gz(part, 6) + gz(b"", 6) + gz(part, 1), 4096),
        ("header fields", gz_fields(part, 6, **fields) + gz_fields(part, 9, **fields), 4096),
        ("30 000 bytes over four letters, 40 times", gz(four_letters()), 1024),
        ("a random block of 20 000 bytes, 100 times", gz(random_block()), 1024),
        ("a run of A", gz(b"A" * (3 << 20)), 1024),
        ("a member end in the last byte of a chunk", member_end_at_chunk_end(part), 1024),
        ("100 zero bytes behind the last member", gz(part) + bytes(100), 4096),
        ("100 other bytes behind the last member", gz(part) + b"q" * 100, 4096),
    ]


def wrong_starts(found, chunk, seed=11):
    """every third chunk that has a start gets another position of its own range -> (starts, how many)"""
    rng = np.random.default_rng(seed)
    starts, k, n_wrong = found.copy(), 0, 0
    for j in range(1, len(found)):
        if found[j] != NO_START:
            if k % 3 == 0:
                starts[j] = 8 * chunk * j + (int(found[j]) + 1 + int(rng.integers(0, 8 * chunk - 1))) % (8 * chunk)
                n_wrong += 1
            k += 1
    return starts, n_wrong


def damaged(file_bytes, n_flips, n_cuts, seed=7):
    rng = np.random.default_rng(seed)
    flips, cuts = [], []
    for bit in rng.integers(0, 8 * len(file_bytes), n_flips):
        b = bytearray(file_bytes)
        b[int(bit) >> 3] ^= 1 << (int(bit) & 7)
        flips.append((int(bit), bytes(b)))
    for at in rng.integers(1, len(file_bytes), n_cuts):
        cuts.append((int(at), file_bytes[:int(at)]))
    return flips, cuts


# ---- the host mirror ------------------------------------------------------------------------------------------------------------------------
def host_find(L, file_bytes, chunk):
    src = np.frombuffer(file_bytes, np.uint8)
    found = np.full(-(-len(file_bytes) // chunk), NO_START, np.uint64)
    assert L.gzh_find(src.ctypes.data, len(file_bytes), chunk, found.ctypes.data) == 0
    return found


def host_run(L, file_bytes, chunk, step=0, out_cap=OUT_CAP, starts=None):
    """the file through feeds of `step` compressed bytes (0: one feed), the unconsumed rest presented again in front of new bytes
    -> (outcome, bytes, counts summed over the feeds (n_rounds: the largest), (status, offset, need))"""
    h = L.gzh_open(chunk)
    src = np.frombuffer(file_bytes, np.uint8) if file_bytes else np.zeros(1, np.uint8)
    out = np.full(out_cap + 128, 0xA5, np.uint8)
    got, total = [], dict.fromkeys(COUNTS, 0)
    lo, hi = 0, min(step, len(file_bytes)) if step else len(file_bytes)
    sp = None if starts is None else np.ascontiguousarray(starts, np.uint64)
    while True:
        last = hi == len(file_bytes)
        consumed, out_len = C.c_uint64(0), C.c_uint64(0)
        counts, err = (C.c_uint64 * 9)(), (C.c_uint64 * 3)()
        rc = L.gzh_feed(h, src.ctypes.data + lo, hi - lo, int(last), out.ctypes.data + 64, out_cap, None if sp is None else sp.ctypes.data, C.byref(consumed), C.byref(out_len), counts, err)
        assert (out[:64] == 0xA5).all() and (out[64 + out_cap:] == 0xA5).all() and out_len.value <= out_cap, "a write outside the output extent"
        got.append(out[64:64 + out_len.value].tobytes())
        for i, name in enumerate(COUNTS):
            total[name] = max(total[name], counts[i]) if name == "n_rounds" else total[name] + counts[i]
        lo += consumed.value
        if rc != FEED_OK or (last and (lo == hi or (consumed.value == 0 and out_len.value == 0))):
            break
        if not last:
            hi = min(len(file_bytes), hi + step)
    L.gzh_close(h)
    return rc, b"".join(got), total, tuple(err)


def check_good(L, name, file_bytes, chunk, **kw):
    ok, want = zlib_read(file_bytes)
    assert ok, name
    rc, got, st, err = host_run(L, file_bytes, chunk, **kw)
    assert rc == FEED_OK and got == want, (name, rc, err, len(got), len(want))
    assert st["n_rounds"] < L.gzh_max_rounds(), (name, st)
    assert st["out_bytes"] == len(want)
    return st


# ---- tests -------------------------------------------------------------------------------------------------------------------------------------
def test_the_library_exports_the_entries():
    from scrubby_amd import lib
    header = open(os.path.join(ROOT, "include", "scrubby_hip.h")).read()
    for name in NEW_EXPORTS:
        assert name in lib.EXPORTS and name + "(" in header, name
    assert lib.SH_GUNZIP_FALLBACK == 10 and "#define SH_GUNZIP_FALLBACK 10" in header


@pytest.mark.parametrize("level", [1, 6, 9])
def test_fastq_at_three_levels_and_three_chunk_sizes(host, fastq, level):
    file_bytes = gz(fastq, level)
    for chunk in (1024, 4096, 16384):
        st = check_good(host, f"level {level}, chunks of {chunk}", file_bytes, chunk)
        assert st["n_chunks"] > 1 and st["n_marker_symbols"] > 0 and st["n_members"] == 1
        print(f"level {level}, chunks of {chunk}: {st}")


def test_flushes_stored_members_fields_repeats_and_tails(host, fastq):
    for name, file_bytes, chunk in streams(fastq):
        st = check_good(host, name, file_bytes, chunk)
        print(f"{name}: {st}")
        if name.startswith("three members"):
            assert st["n_members"] == 3
        if name.startswith("a random block"):
            assert st["n_marker_symbols"] > 1_000_000      # every window is all markers


def test_feeds_of_100_000_bytes_with_an_output_that_forces_carry_over(host, fastq):
    for level in (1, 6, 9):
        st = check_good(host, f"level {level} in feeds", gz(fastq, level), 4096, step=100000, out_cap=300000)
        assert st["n_chunks"] > 1


def test_fixed_blocks_end_in_the_fallback_with_the_bytes_so_far_right(host, fastq):
    file_bytes = gz(fastq, 6, zlib.Z_FIXED)
    rc, got, st, err = host_run(host, file_bytes, 4096)
    assert rc == FEED_ROUNDS and st["n_rounds"] == host.gzh_max_rounds()
    assert 0 < len(got) < len(fastq) and fastq.startswith(got)


def test_more_members_in_a_span_than_it_records_is_the_fallback(host):
    file_bytes = gz(b"x" * 100) * 6
    rc, got, st, err = host_run(host, file_bytes, 1024)
    assert rc == FEED_ENDS and got == b""


def test_what_is_no_gzip_file_and_an_empty_file(host):
    assert host_run(host, b"plain text, no gzip member at all", 1024)[0] == FEED_NOT_GZIP
    assert host_run(host, b"", 1024)[:2] == (FEED_OK, b"")
    rc, got, st, err = host_run(host, gz(b"abc") + b"\x1f\x8b\x08", 1024)      # a header cut short behind a member: gzread's error too
    assert rc == FEED_TRUNCATED and not zlib_read(gz(b"abc") + b"\x1f\x8b\x08")[0]


def test_an_output_below_the_first_chunk_names_the_size(host, fastq):
    rc, got, st, err = host_run(host, gz(fastq[:100000]), 4096, out_cap=1000)
    assert rc == FEED_OUT_CAP and got == b"" and err[2] > 1000


def test_flipped_bits_never_give_other_bytes(host, fastq):
    text = fastq[:120000]
    flips, _ = damaged(gz(text), 200, 0)
    n_ok = 0
    for bit, bad in flips:
        rc, got, st, err = host_run(host, bad, 1024)
        ok, want = zlib_read(bad)
        if rc == FEED_OK:
            assert ok and got == want, bit
            n_ok += 1
        elif rc in (FEED_ROUNDS, FEED_ENDS):
            assert want.startswith(got), bit
        else:
            assert rc in (FEED_DATA, FEED_TRUNCATED, FEED_NOT_GZIP), (bit, rc)
    print(f"{n_ok} of {len(flips)} damaged files still decode (header bytes zlib ignores)")


def test_a_cut_stream_is_an_error(host, fastq):
    _, cuts = damaged(gz(fastq[:120000]), 0, 50)
    for at, bad in cuts:
        rc, got, st, err = host_run(host, bad, 1024)
        assert rc in (FEED_TRUNCATED, FEED_DATA, FEED_NOT_GZIP), (at, rc)
        assert not zlib_read(bad)[0]


def test_wrong_starts_are_redone(host, fastq):
    text = fastq
    file_bytes, chunk = gz(text, 1), 4096      # level 1 ends a block every ~25 KB of compressed bytes: a dozen chunks have a start
    found = host_find(host, file_bytes, chunk)
    starts, n_wrong = wrong_starts(found, chunk)
    assert n_wrong >= 3
    rc, got, st, err = host_run(host, file_bytes, chunk, starts=starts)
    assert rc == FEED_OK and got == text and st["n_redone"] >= n_wrong, (rc, st, n_wrong)
    rc, got, plain, err = host_run(host, file_bytes, chunk, starts=found)
    assert rc == FEED_OK and got == text and plain["n_redone"] < st["n_redone"]


def test_candidates_by_kind(host, fastq):
    """the counts behind the decision to take non-empty stored blocks as candidates: over the compressed FASTQ (one long dynamic-block
    stream) the stored candidates are all false, and few; a stored stream's block starts are found only through them"""
    kinds = (C.c_uint64 * 3)()
    z = np.frombuffer(gz(fastq, 6), np.uint8)
    host.gzh_candidates(z.ctypes.data, len(z), kinds)
    print(f"level 6, {len(z)} bytes: {kinds[0]} dynamic, {kinds[1]} empty stored, {kinds[2]} non-empty stored candidates")
    assert kinds[0] >= 5 and kinds[1] + kinds[2] <= 64      # 2^-21 per bit position would be ~1 over these 2.0 M positions
    z0 = np.frombuffer(gz(fastq, 0), np.uint8)
    host.gzh_candidates(z0.ctypes.data, len(z0), kinds)
    print(f"level 0, {len(z0)} bytes: {kinds[0]} dynamic, {kinds[1]} empty stored, {kinds[2]} non-empty stored candidates")
    assert kinds[2] >= len(fastq) // 65535 - 1


def test_sanitizer_program(tmp_path):
    exe = str(tmp_path / "gunzip_main")
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DGUNZIP_MAIN", "-o", exe, SRC, "-lz"])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "cases ok" in r.stdout, r.stdout + r.stderr
