"""The BGZF / DEFLATE decoder's pure parts on the host (scrubby_amd/csrc/sh_inflate.h through tests/inflate_host.cpp): the member scan,
the decode tables, the block decoder and CRC-32 in 64 pieces - the code every lane of k_inflate_member runs.  Valid members are compared
byte for byte with Python's zlib; table rejections with the rejections zlib makes of a block that carries the same lengths; every
corrupt member is first shown to be rejected by zlib (or, for CRC-32 and ISIZE, by gzip), so no case depends on this decoder being
stricter than the reference.

inflate_host.cpp has a main of its own behind -DINFLATE_MAIN: built with -fsanitize=address,undefined it is the sanitizer run of this
code, a stand-alone program on the CPU (the last test builds and runs it).  The decoder works on heap copies of exactly the member's
input and output extents there, so an access outside them ends the program with a report.

The valid and corrupt cases are functions of this module: tests/test_inflate_gpu.py sends the same ones through the device."""
import ctypes as C
import gzip
import os
import subprocess
import zlib

import numpy as np
import pytest

from tests import bgzf_util as B
from tests.test_deflate_gpu import fastq      # noqa: F401  (the varied-quality FASTQ text)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "inflate_host.cpp")
DFH_SRC = os.path.join(ROOT, "tests", "deflate_host.cpp")
MATCH = 0x80000000
OK, BAD_BTYPE, BAD_LENGTHS, BAD_SYMBOL, DIST_FAR, IN_OVERRUN, OUT_OVERRUN, OUT_SHORT, STORED_LEN, CRC = range(10)
NEW_EXPORTS = ["sh_bgzf_scan", "sh_inflater_create", "sh_inflate_members_device", "sh_gunzip_bgzf", "sh_inflater_free"]


class Member(C.Structure):
    _fields_ = [("file_off", C.c_uint64), ("in_off", C.c_uint64), ("in_len", C.c_uint32), ("out_len", C.c_uint32), ("crc32", C.c_uint32), ("status", C.c_uint32)]


def build_host(tmp_path_factory):
    d = tmp_path_factory.mktemp("inh")
    so, dfh = str(d / "libinflate_host.so"), str(d / "libdeflate_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, SRC])
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", dfh, DFH_SRC])
    L, D = C.CDLL(so), C.CDLL(dfh)
    L.inh_scan.restype = C.c_int
    L.inh_scan.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(Member), C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.inh_build.restype = C.c_int
    L.inh_build.argtypes = [C.c_void_p, C.c_uint32, C.c_int]
    L.inh_crc.restype = C.c_uint32
    L.inh_crc.argtypes = [C.c_void_p, C.c_uint32]
    L.inh_inflate.restype = C.c_int
    L.inh_inflate.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    D.dfh_lengths.restype = C.c_uint32
    D.dfh_lengths.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p]
    D.dfh_encode.restype = C.c_int
    D.dfh_encode.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
    L.dfh = D
    return L


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_host(tmp_path_factory)


def host_inflate(L, raw, isize, crc):
    """(status, the bytes produced, (stored, fixed, dynamic) blocks) of the host decoder; guard bytes around the output stay as they were"""
    src = np.frombuffer(raw, np.uint8) if raw else np.zeros(1, np.uint8)
    out = np.full(isize + 128, 0xA5, np.uint8)
    info = (C.c_uint32 * 5)()
    st = L.inh_inflate(src.ctypes.data, len(raw), out.ctypes.data + 64, isize, crc, info)
    assert (out[:64] == 0xA5).all() and (out[64 + isize:] == 0xA5).all(), "a write outside the output extent"
    assert st == info[0] and info[1] <= isize
    return st, out[64:64 + info[1]].tobytes(), (info[2], info[3], info[4])


def encode_tokens(L, tokens):
    """one final dynamic block over a token list, by the encoder's token writer (dfh_encode) -> (raw stream, literal code lengths)"""
    tok = np.ascontiguousarray(tokens, dtype=np.uint32)
    out = np.zeros(6 * len(tok) + 1024, np.uint8)
    n = C.c_uint64(0)
    lit, dist = np.zeros(286, np.uint8), np.zeros(30, np.uint8)
    assert L.dfh.dfh_encode(tok.ctypes.data, len(tok), out.ctypes.data, len(out), C.byref(n), lit.ctypes.data, dist.ctypes.data) == 0
    return out[:n.value].tobytes(), lit


def _match(length, dist):
    return MATCH | (dist - 1) << 8 | (length - 3)


def _fib(n):
    f = [1, 2]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f


def valid_cases(L, text):
    """[(name, raw stream, the bytes it means)]; text: FASTQ, at least 65 536 bytes"""
    assert len(text) >= 65536
    piece = text[:B.BLOCK]
    cases = [(name, B.raw_deflate(piece, **kw), piece) for name, kw in B.SHAPES.items()]
    for n in (0, 1, 65536):
        cases.append((f"{n} bytes", B.raw_deflate(text[:n]), text[:n]))
    run = b"A" * 60000
    cases.append(("a run of one byte", B.raw_deflate(run, 9), run))      # distance 1, length 258
    rng = np.random.default_rng(3)
    lits = [int(v) for v in rng.integers(0, 256, 32768)]
    far = bytes(lits) + bytes(lits[:258])
    cases.append(("distance 32768 back to the first byte", encode_tokens(L, lits + [_match(258, 32768)])[0], far))
    cases.append(("length 3 at distance 1", encode_tokens(L, [97, _match(3, 1)])[0], b"aaaa"))
    # the end-of-block symbol and 21 literals with counts F(1)..F(22): Huffman's tree is a comb of depth 21, the limiter acts
    sym = np.repeat(np.arange(21, dtype=np.uint8) + 65, _fib(21))
    np.random.default_rng(2).shuffle(sym)
    raw, lit_lens = encode_tokens(L, [int(v) for v in sym])
    assert lit_lens.max() == 15
    cases.append(("15-bit literal codes", raw, sym.tobytes()))
    return cases


def _zlib_rejects_raw(raw):
    z = zlib.decompressobj(-15)
    try:
        z.decompress(raw)
    except zlib.error:
        return True
    return not z.eof


def _gzip_rejects(member):
    try:
        gzip.decompress(member)
    except (gzip.BadGzipFile, zlib.error, EOFError):
        return True
    return False


def corrupt_cases(text):
    """[(name, raw stream, ISIZE, CRC-32, the status wanted or None for any but OK)]; each is first shown to be rejected by zlib / gzip"""
    piece = text[:B.BLOCK]
    good, crc, n = B.raw_deflate(piece), zlib.crc32(piece), len(piece)
    flipped = None
    for bit in range(4 * len(good), 8 * len(good)):      # the first bit past the middle whose flip zlib itself refuses
        z = bytearray(good)
        z[bit >> 3] ^= 1 << (bit & 7)
        if _zlib_rejects_raw(bytes(z)):
            flipped = bytes(z)
            break
    stored = bytearray(B.raw_deflate(piece, 0))
    stored[3] ^= 1
    cases = [
        ("one bit flipped", flipped, n, crc, None),
        ("NLEN mismatch", bytes(stored), n, crc, STORED_LEN),
        ("block type 3", b"\x07\x00", 0, 0, BAD_BTYPE),
        ("distance 1 as the first token", b"\x03\x02\x00\x00", 3, 0, DIST_FAR),      # fixed block: length symbol 257, distance symbol 0
        ("input one byte short", good[:-1], n, crc, IN_OVERRUN),
    ]
    for name, raw, _, _, _ in cases:
        assert _zlib_rejects_raw(raw), name
    trailer = [("ISIZE one too small", good, n - 1, crc, OUT_OVERRUN), ("ISIZE one too large", good, n + 1, crc, OUT_SHORT),
               ("CRC off by one", good, n, (crc + 1) & 0xFFFFFFFF, CRC)]
    for name, raw, isize, c, _ in trailer:
        assert _gzip_rejects(B.wrap(raw, piece, crc=c, isize=isize)), name
    return cases + trailer


# ---- the scan ------------------------------------------------------------------------------------------------------------------------
def _scan(L, buf, cap=64):
    arr = (Member * cap)()
    n, used = C.c_uint64(0), C.c_uint64(0)
    src = np.frombuffer(buf, np.uint8) if buf else np.zeros(1, np.uint8)
    stopped = L.inh_scan(src.ctypes.data, len(buf), arr, cap, C.byref(n), C.byref(used))
    return [arr[i] for i in range(n.value)], used.value, stopped


def test_scan_takes_every_form_of_header(host, fastq):
    a, b = fastq[:5000], fastq[5000:70000]
    m1 = B.member(a, extra_before=b"XY\x03\x00abc", fname=b"reads.fastq", fhcrc=True)      # a foreign subfield before BC, FNAME, FHCRC
    m2 = B.member(b)
    buf = m1 + m2 + B.EOF
    assert gzip.decompress(buf) == a + b and len(B.EOF) == 28
    ms, used, stopped = _scan(host, buf)
    assert stopped == 0 and used == len(buf) and len(ms) == 3
    assert [m.file_off for m in ms] == [0, len(m1), len(m1) + len(m2)]
    assert [m.out_len for m in ms] == [len(a), len(b), 0] and [m.crc32 for m in ms] == [zlib.crc32(a), zlib.crc32(b), 0]
    for m, data in zip(ms, (a, b, b"")):      # the extent is exactly the raw stream
        assert zlib.decompress(buf[m.in_off:m.in_off + m.in_len], -15) == data
        assert m.in_off + m.in_len + 8 == m.file_off + (len(m1) if m is ms[0] else len(m2) if m is ms[1] else 28)
    ms, used, stopped = _scan(host, buf, cap=2)
    assert len(ms) == 2 and used == len(m1) + len(m2) and stopped == 0


@pytest.mark.parametrize("where", ["header", "data", "trailer", "bsize"])
def test_scan_stops_at_an_incomplete_member(host, fastq, where):
    m1, m2 = B.member(fastq[:3000]), B.member(fastq[3000:9000])
    cut = {"header": len(m1) + 7, "data": len(m1) + len(m2) // 2, "trailer": len(m1) + len(m2) - 3, "bsize": len(m1) + 18}[where]
    ms, used, stopped = _scan(host, (m1 + m2)[:cut])
    assert stopped == 1 and len(ms) == 1 and used == len(m1)


def test_scan_stops_at_what_is_not_bgzf(host, fastq):
    m1, m2 = B.member(fastq[:3000]), B.member(fastq[3000:9000])
    plain = gzip.compress(fastq[9000:12000])
    ms, used, stopped = _scan(host, m1 + m2 + plain + B.EOF)
    assert stopped == 2 and len(ms) == 2 and used == len(m1) + len(m2)
    ms, used, stopped = _scan(host, m1 + b"not gzip at all")
    assert stopped == 2 and len(ms) == 1 and used == len(m1)
    big = B.wrap(B.raw_deflate(b""), b"", isize=65537)
    ms, used, stopped = _scan(host, m1 + big)
    assert stopped == 2 and len(ms) == 1 and used == len(m1)
    ms, used, stopped = _scan(host, b"")
    assert stopped == 0 and not ms and used == 0


# ---- the tables ----------------------------------------------------------------------------------------------------------------------
def _dynamic_block(lit_lens, dist_lens, body_bits=()):
    """A final dynamic block that carries these code lengths verbatim (code-length code: 5 bits for every length 0..15) and then
    `body_bits`: what zlib is shown, so that its verdict on the lengths can be read"""
    bits = [1, 0, 1]      # BFINAL, BTYPE 10 (LSB first)

    def put(v, n):
        bits.extend((v >> i) & 1 for i in range(n))
    hlit, hdist = max(257, len(lit_lens)), max(1, len(dist_lens))
    lit = list(lit_lens) + [0] * (hlit - len(lit_lens))
    dist = list(dist_lens) + [0] * (hdist - len(dist_lens))
    put(hlit - 257, 5), put(hdist - 1, 5), put(19 - 4, 4)
    cl = {s: 5 for s in range(16)}      # sixteen codes of 5 bits: 16 / 32 of the code space; 16, 17, 18 take 2, 3, 3 bits for the rest
    cl.update({16: 2, 17: 3, 18: 3})
    for s in (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15):
        put(cl[s], 3)
    # canonical codes of that code-length code: lengths 2 (16), 3 (17, 18), 5 (0..15)
    code, nxt = 0, {}
    for ln in range(1, 8):
        for s in sorted(cl):
            if cl[s] == ln:
                nxt[s] = (code, ln)
                code += 1
        code <<= 1
    for v in lit + dist:
        c, ln = nxt[v]
        bits.extend((c >> (ln - 1 - i)) & 1 for i in range(ln))      # Huffman codes go MSB first
    bits.extend(body_bits)
    bits += [0] * (-len(bits) % 8)
    return bytes(sum(b << i for i, b in enumerate(bits[o:o + 8])) for o in range(0, len(bits), 8))


def _zlib_verdict(raw):
    try:
        zlib.decompressobj(-15).decompress(raw)
    except zlib.error as e:
        return str(e)
    return None


def test_tables_reject_what_zlib_rejects(host):
    def build(lens, kind):
        a = np.asarray(lens, np.uint8)
        return host.inh_build(a.ctypes.data, len(a), kind)
    lit_ok = [0] * 257
    lit_ok[65], lit_ok[256] = 1, 1      # 'A' and end-of-block, one bit each: a complete code
    eob = (1,)                          # the end-of-block code: the second code of one bit
    # over-subscribed: three codes of one bit
    assert build([1, 1, 1], 2) == BAD_LENGTHS and "invalid distances set" in _zlib_verdict(_dynamic_block(lit_ok, [1, 1, 1], eob))
    over = list(lit_ok); over[66] = 1
    assert build(over, 1) == BAD_LENGTHS and "invalid literal/lengths set" in _zlib_verdict(_dynamic_block(over, [1], eob))
    # incomplete: three codes of two bits
    assert build([2, 2, 2], 2) == BAD_LENGTHS and "invalid distances set" in _zlib_verdict(_dynamic_block(lit_ok, [2, 2, 2], eob))
    inc = [0] * 257; inc[65], inc[66], inc[256] = 2, 2, 2
    assert build(inc, 1) == BAD_LENGTHS and "invalid literal/lengths set" in _zlib_verdict(_dynamic_block(inc, [1], (1, 0)))
    assert build([2, 2, 2] + [0] * 16, 0) == BAD_LENGTHS and build([1] + [0] * 18, 0) == BAD_LENGTHS      # the code-length code is never incomplete
    # the one-code distance alphabet, and no distance code at all in a block of literals only: both taken, by zlib too
    assert build([0] * 7 + [1], 2) == OK and _zlib_verdict(_dynamic_block(lit_ok, [0] * 7 + [1], eob)) is None
    assert build([0] * 30, 2) == OK and _zlib_verdict(_dynamic_block(lit_ok, [0], (0, 0, 1))) is None
    one = [0] * 257; one[256] = 1       # a literal/length code of the end-of-block symbol alone
    assert build(one, 1) == OK and _zlib_verdict(_dynamic_block(one, [0], (0,))) is None
    assert build([1, 1] + [0] * 28, 2) == OK and build(lit_ok, 1) == OK


def test_blocks_with_such_tables_decode_as_zlib_decodes_them(host):
    lit_ok = [0] * 257
    lit_ok[65], lit_ok[256] = 1, 1
    for raw, want in ((_dynamic_block(lit_ok, [0], (0, 0, 1)), b"AA"), (_dynamic_block([0] * 256 + [1], [0], (0,)), b"")):
        assert zlib.decompress(raw, -15) == want
        assert host_inflate(host, raw, len(want), zlib.crc32(want))[:2] == (OK, want)
    # a distance symbol where there is no distance code, and the unused half of a one-code distance alphabet
    lit_m = [0] * 258
    lit_m[65], lit_m[256], lit_m[257] = 1, 2, 2      # A = 0, EOB = 10, length 3 = 11
    for dist_lens, body in (([0], (0, 1, 1, 0)), ([1], (0, 1, 1, 1))):
        raw = _dynamic_block(lit_m, dist_lens, body + (1, 0))
        assert "invalid distance" in _zlib_verdict(raw)
        assert host_inflate(host, raw, 4, 0)[0] == BAD_SYMBOL


# ---- whole members -------------------------------------------------------------------------------------------------------------------
def test_valid_members_inflate_to_zlibs_bytes(host, fastq):
    kinds = [0, 0, 0]
    for name, raw, data in valid_cases(host, fastq):
        z = zlib.decompressobj(-15)
        assert z.decompress(raw) == data and z.eof and z.unused_data == b"", name
        st, out, blocks = host_inflate(host, raw, len(data), zlib.crc32(data))
        assert (st, out) == (OK, data), name
        kinds = [a + b for a, b in zip(kinds, blocks)]
        if name == "stored":
            assert blocks[0] >= 1 and blocks[1:] == (0, 0)
        if name == "fixed":
            assert blocks[1] >= 1 and (blocks[0], blocks[2]) == (0, 0)
        if name in ("full_flush", "sync_flush"):
            assert blocks[0] == 1 and blocks[2] >= 2      # the flush's empty stored block between dynamic ones
    assert all(kinds)


def test_crc_in_pieces_is_zlibs_crc32(host, fastq):
    for n in (0, 1, 63, 64, 65, 127, 4097, 65535, 65536):
        a = np.frombuffer(fastq[:n], np.uint8) if n else np.zeros(1, np.uint8)
        assert host.inh_crc(a.ctypes.data, n) == zlib.crc32(fastq[:n]), n


def test_corrupt_members_end_with_their_status(host, fastq):
    for name, raw, isize, crc, want in corrupt_cases(fastq):
        st, out, _ = host_inflate(host, raw, isize, crc)
        assert st != OK and (want is None or st == want), (name, st)
    # every 61st bit of a member flipped: any status, no write outside the extent, and OK only with the right bytes
    piece = fastq[:20000]
    good, crc = B.raw_deflate(piece), zlib.crc32(piece)
    for bit in range(0, 8 * len(good), 61):
        z = bytearray(good)
        z[bit >> 3] ^= 1 << (bit & 7)
        st, out, _ = host_inflate(host, bytes(z), len(piece), crc)
        assert st != OK or out == piece, bit


def test_c_abi_has_the_inflate_symbols_and_scans_on_the_host(fastq):
    from scrubby_amd import lib as S
    L = S.load()
    assert L.sh_version() == 104
    for name in NEW_EXPORTS:
        assert name in S.EXPORTS and hasattr(L, name), name
    hdr = open(os.path.join(ROOT, "include", "scrubby_hip.h")).read()
    assert "typedef struct sh_gz_member { uint64_t file_off, in_off; uint32_t in_len, out_len, crc32, status; } sh_gz_member;" in hdr
    assert C.sizeof(S.GzMember) == 32 and C.sizeof(S.InflateStats) == 56
    m1, m2 = B.member(fastq[:3000]), B.member(fastq[3000:9000])
    ms, used, stopped = S.bgzf_scan(m1 + m2 + B.EOF)
    assert (len(ms), used, stopped) == (3, len(m1) + len(m2) + 28, 0) and ms[1].file_off == len(m1) and ms[1].out_len == 6000
    ms, used, stopped = S.bgzf_scan(m1 + m2[:100])
    assert (len(ms), used, stopped) == (1, len(m1), 1)
    ms, used, stopped = S.bgzf_scan(m1 + gzip.compress(b"x"))
    assert (len(ms), used, stopped) == (1, len(m1), 2)


def test_stand_alone_program_under_the_sanitizers(tmp_path):
    """The same file with its own main (and deflate_host.cpp for the token writer), built with AddressSanitizer and UBSan and run as a
    program of its own: valid members of every shape, the corrupt ones, and a member with every 61st bit flipped in turn, each decoded
    on heap blocks of exactly the member's extents.  The sanitizer runtimes are linked statically: the program needs nothing from its
    environment."""
    exe = str(tmp_path / "inflate_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DINFLATE_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-o", exe, SRC, DFH_SRC, "-lz"])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "cases ok" in out.stdout
