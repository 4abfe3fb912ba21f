"""The DEFLATE encoder's pure parts on the host (scrubby_amd/csrc/sh_deflate.h through tests/deflate_host.cpp): length-limited code
lengths from a histogram, canonical codes, the dynamic header and the token writer - the code lane 0 of k_deflate_block runs.  Code
lengths are checked by their limit and Kraft sum; whole blocks by Python's zlib, which must return the bytes the token list means, see
the end of the stream and leave nothing over.

deflate_host.cpp has a main of its own behind -DDEFLATE_MAIN that runs the same cases and inflates with zlib: built with
-fsanitize=address,undefined it is the sanitizer run of this code, a stand-alone program on the CPU (the last test builds and runs it)."""
import ctypes as C
import os
import subprocess
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "deflate_host.cpp")
N_LIT, N_DIST = 286, 30
MATCH = 0x80000000


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("dfh") / "libdeflate_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, SRC])
    L = C.CDLL(so)
    L.dfh_lengths.restype = C.c_uint32
    L.dfh_lengths.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p]
    L.dfh_kraft.restype = C.c_uint64
    L.dfh_kraft.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
    L.dfh_codes_ok.restype = C.c_int
    L.dfh_codes_ok.argtypes = [C.c_void_p, C.c_uint32]
    L.dfh_cl_freq.restype = None
    L.dfh_cl_freq.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.dfh_encode.restype = C.c_int
    L.dfh_encode.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
    L.dfh_bound.restype = C.c_uint64
    L.dfh_bound.argtypes = [C.c_uint64, C.c_uint32]
    L.dfh_len_sym.restype = None
    L.dfh_len_sym.argtypes = [C.c_uint32, C.c_void_p]
    L.dfh_dist_sym.restype = None
    L.dfh_dist_sym.argtypes = [C.c_uint32, C.c_void_p]
    return L


def _lengths(L, freq, limit, complete):
    freq = np.ascontiguousarray(freq, dtype=np.uint32)
    lens = np.zeros(len(freq), np.uint8)
    used = L.dfh_lengths(freq.ctypes.data, len(freq), limit, int(complete), lens.ctypes.data)
    assert all(lens[freq > 0] > 0), "a used symbol has no code"
    assert lens.max(initial=0) <= limit
    return used, lens, L.dfh_kraft(lens.ctypes.data, len(lens), limit)


def _fib(n):
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f


def test_fibonacci_histogram_is_pulled_under_the_limit(host):
    """Counts F(1)..F(24): Huffman's tree is a comb of depth 23, so the limiter must act; the code stays complete."""
    used, lens, kraft = _lengths(host, _fib(24), 15, True)
    assert used == 24 and lens.max() == 15 and kraft == 1 << 15
    assert host.dfh_codes_ok(lens.ctypes.data, len(lens))
    assert all(lens[i] >= lens[i + 1] for i in range(23)), "a rarer symbol has the shorter code"
    # the code-length alphabet: 19 symbols, 7 bits
    used, lens, kraft = _lengths(host, _fib(19), 7, True)
    assert used == 19 and lens.max() == 7 and kraft == 1 << 7
    assert host.dfh_codes_ok(lens.ctypes.data, len(lens))


def test_one_two_and_all_symbols_used(host):
    one = np.zeros(N_LIT, np.uint32); one[65] = 9
    used, lens, kraft = _lengths(host, one, 15, True)      # completed with a second code of one bit: inflate wants a complete literal code
    assert used == 2 and lens[65] == 1 and lens[0] == 1 and kraft == 1 << 15
    zero_only = np.zeros(N_LIT, np.uint32); zero_only[0] = 3
    used, lens, kraft = _lengths(host, zero_only, 15, True)
    assert used == 2 and lens[0] == 1 and lens[1] == 1 and kraft == 1 << 15
    two = np.zeros(N_LIT, np.uint32); two[65] = 9; two[256] = 1
    used, lens, kraft = _lengths(host, two, 15, True)
    assert used == 2 and lens[65] == 1 and lens[256] == 1 and kraft == 1 << 15
    rng = np.random.default_rng(7)
    for freq in (np.ones(N_LIT, np.uint32), rng.integers(1, 1000, N_LIT), rng.geometric(0.01, N_LIT) ** 2):
        used, lens, kraft = _lengths(host, freq, 15, True)
        assert used == N_LIT and kraft == 1 << 15 and host.dfh_codes_ok(lens.ctypes.data, N_LIT)


def test_distance_alphabet_may_be_incomplete_in_two_cases_only(host):
    """RFC 1951 3.2.7: no distance code at all (a block of literals), or one code of one bit."""
    used, lens, kraft = _lengths(host, np.zeros(N_DIST, np.uint32), 15, False)
    assert used == 0 and not lens.any() and kraft == 0
    for sym in (0, 17, 29):
        f = np.zeros(N_DIST, np.uint32); f[sym] = 5
        used, lens, kraft = _lengths(host, f, 15, False)
        assert used == 1 and lens[sym] == 1 and lens.sum() == 1 and kraft == 1 << 14
    f = np.zeros(N_DIST, np.uint32); f[3] = 1; f[29] = 1000
    used, lens, kraft = _lengths(host, f, 15, False)
    assert used == 2 and kraft == 1 << 15


def test_length_and_distance_symbols_match_the_tables_of_rfc_1951(host):
    len_base = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
    len_extra = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
    dist_base = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
    dist_extra = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]
    out = (C.c_uint32 * 3)()
    for n in range(3, 259):
        host.dfh_len_sym(n, out)
        s = max(i for i in range(29) if len_base[i] <= n)
        assert (out[0], out[1], out[2]) == (257 + s, len_extra[s], n - len_base[s]), n
    for d in list(range(1, 1200)) + [4096, 4097, 6144, 6145, 16384, 16385, 24576, 24577, 32767, 32768]:
        host.dfh_dist_sym(d, out)
        s = max(i for i in range(30) if dist_base[i] <= d)
        assert (out[0], out[1], out[2]) == (s, dist_extra[s], d - dist_base[s]), d


def _match(length, dist):
    return MATCH | (dist - 1) << 8 | (length - 3)


def _expand(tokens):
    o = bytearray()
    for t in tokens:
        if not t & MATCH:
            o.append(t)
            continue
        length, dist = (t & 0xFF) + 3, ((t >> 8) & 0x7FFF) + 1
        for _ in range(length):
            o.append(o[-dist])
    return bytes(o)


def _round_trip(L, tokens):
    tok = np.ascontiguousarray(tokens, dtype=np.uint32)
    out = np.zeros(6 * len(tok) + 1024, np.uint8)
    n = C.c_uint64(0)
    lit, dist = np.zeros(N_LIT, np.uint8), np.zeros(N_DIST, np.uint8)
    rc = L.dfh_encode(tok.ctypes.data, len(tok), out.ctypes.data, len(out), C.byref(n), lit.ctypes.data, dist.ctypes.data)
    # 1 / 2 Kraft sum of the literal / distance code, 3 codes not prefix-free, 4 header bits, 5 body bits differ from the histogram's, 6 space
    assert rc == 0, f"encode failed with code {rc}"
    z = zlib.decompressobj(-15)
    back = z.decompress(out[:n.value].tobytes())
    assert back == _expand(tokens) and z.eof and z.unused_data == b"" and z.unconsumed_tail == b""
    return lit, dist


def test_token_lists_inflate_to_what_they_mean(host):
    lit, dist = _round_trip(host, [(i * 37) % 251 for i in range(300)])      # literals only
    assert not dist.any()
    lit, dist = _round_trip(host, [ord("a"), _match(3, 1)])
    assert dist[0] == 1 and dist.sum() == 1 and lit[257] > 0
    rng = np.random.default_rng(3)
    lit, dist = _round_trip(host, [int(v) for v in rng.integers(0, 256, 32768)] + [_match(258, 32768)])
    assert lit[285] > 0 and dist[29] == 1
    _round_trip(host, [])      # the end-of-block symbol alone
    every = [1, 2]
    for n in range(3, 259):
        every += [n & 0xFF, _match(n, 1 + n % 2)]
    _round_trip(host, every)


def test_a_long_run_of_unused_symbols_takes_codes_17_and_18(host):
    """Bytes 0 and 255 only: the lengths of literals 1..254 are a run of 254 zeros - code 18 for 138 of them, and again for the rest."""
    lit, dist = _round_trip(host, [0, 255, 0, 255, 255, 0])
    assert lit[0] and lit[255] and lit[256] and not lit[1:255].any()
    cl = np.zeros(19, np.uint32)
    host.dfh_cl_freq(lit.ctypes.data, dist.ctypes.data, cl.ctypes.data)
    assert cl[18] == 2 and cl[0] == 1, cl      # 138 + 116; the lengths of 255 and 256; the one zero is the distance code's
    lit2, dist2 = _round_trip(host, [0, 1, 2, 3, 4, 5, 6, 7, 8, 200])      # 9..199 is 191 zeros (18 twice), 201..255 is 55 (18 once)
    host.dfh_cl_freq(lit2.ctypes.data, dist2.ctypes.data, cl.ctypes.data)
    assert cl[18] == 3 and cl[16] >= 1, cl      # eight literals of one length: the length, then code 16


def test_bound(host):
    assert host.dfh_bound(0, 32768) == 5 and host.dfh_bound(1, 1024) == 6 and host.dfh_bound(1024, 1024) == 1029 and host.dfh_bound(1025, 1024) == 1035
    assert host.dfh_bound(70000, 65535) == 70010


def test_stand_alone_program_under_the_sanitizers(tmp_path):
    """The same file with its own main, built with AddressSanitizer and UBSan and run as a program of its own: a write past the header
    buffer, a shift by a length past 15 or an index past an alphabet ends it with a report.  The sanitizer runtimes are linked statically:
    the program needs nothing from its environment."""
    exe = str(tmp_path / "deflate_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DDEFLATE_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-o", exe, SRC, "-lz"])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "12 cases ok" in out.stdout
