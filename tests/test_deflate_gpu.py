"""DEFLATE on the device (scrubby_amd/csrc/sh_deflate.hip through sh_deflate_device / sh_gzip_member): every stream is inflated by
Python's zlib (raw, so a distance past the window or a broken block boundary is an error) or gzip (CRC-32 and ISIZE), must give back the
input, fit the bound, and agree with the stats.  Sizes are the smallest at which the kernel can go wrong: inputs shorter than the hash's
4 bytes, blocks that end on / one before / one past a block edge, a run that needs length 258, data that must be stored, a match at the
window's edge, a histogram that needs the 15-bit limiter, every alignment of the input pointer.

FASTQ at block 32768 (1 072 155 bytes from the generator below; zlib on the same 32768-byte pieces: Huffman only 413 862, Z_RLE 345 630,
level 1 305 236, level 6 259 619): the device stream must be smaller than Z_RLE's, which finds distance-1 matches only."""
import gzip
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def S():
    from scrubby_amd import lib
    lib.require_gpu()
    return lib


@pytest.fixture(scope="module")
def deflaters(S):
    made = {}

    def get(block):
        if block not in made:
            made[block] = S.Deflater(2 << 20, block)
        return made[block]
    yield get
    for d in made.values():
        d.close()


@pytest.fixture(scope="module")
def fastq():
    rng = np.random.default_rng(1)
    out = []
    for i in range(3000):
        x, y = rng.integers(1000, 30000, 2)
        seq = "".join("ACGT"[k] for k in rng.integers(0, 4, 150))
        qual = "".join("FF:,#"[min(int(g), 4)] for g in rng.geometric(0.7, 150) - 1)
        out.append(f"@A00123:45:HXXXXXXX:{1 + i % 4}:{1101 + i // 977}:{x}:{y} 1:N:0:ACGTACGT\n{seq}\n+\n{qual}\n")
    return "".join(out).encode()


def _check(S, df, data, block, flags=0):
    """deflate `data`, inflate it with zlib, and hold the stream to the bound and the stats"""
    z, st = df.deflate(data, flags)
    inf = zlib.decompressobj(-15)
    back = inf.decompress(z)
    assert back == data, f"{len(data)} bytes in blocks of {block}: zlib returns other bytes"
    assert inf.eof and inf.unused_data == b"" and inf.unconsumed_tail == b""
    assert len(z) <= S.deflate_bound(len(data), block) and st["out_bytes"] == len(z)
    if len(data):
        assert st["n_blocks"] == -(-len(data) // (block or 32768))
    return z, st


@pytest.mark.parametrize("n", [0, 1, 2, 3, 4, 5])
def test_tiny_inputs(S, deflaters, n):
    z, st = _check(S, deflaters(1024), b"abcab"[:n], 1024)
    if n == 0:
        assert z == b"\x03\x00" and S.deflate_bound(0, 1024) == 5


@pytest.mark.parametrize("n", [1023, 1024, 1025, 2055, 8192])
def test_block_edges(S, deflaters, n):
    """text-like bytes, so the blocks are coded and each is followed by the empty stored block that realigns the stream; BFINAL on the
    last block only, or zlib stops early / runs out of input"""
    rng = np.random.default_rng(n)
    data = bytes(rng.choice(np.frombuffer(b"ACGTN\n@+F:", np.uint8), n, p=[.2, .2, .2, .2, .02, .02, .02, .02, .1, .02]))
    z, st = _check(S, deflaters(1024), data, 1024)
    # a last block of 1 or 7 bytes is stored - 6 and 12 bytes, less than any dynamic header; the full blocks are coded
    assert st["n_stored"] == (1 if n % 1024 in (1, 7) else 0) and len(z) < n


def test_a_long_run_takes_length_258(S, deflaters):
    n = 70000
    z, st = _check(S, deflaters(65535), b"A" * n, 65535)
    assert st["n_blocks"] == 2
    assert len(z) < n / 50      # 258 bytes per token of at most ~20 bits
    assert st["n_matches"] >= n // 258 and st["n_literals"] <= 2 * (1 + 3)      # a block's first byte has nothing to point at; a tail under 4 bytes


def test_no_match_and_no_distance_code(S, deflaters):
    data = bytes(range(256))
    z, st = _check(S, deflaters(1024), data, 1024)
    assert st["n_matches"] == 0 and st["n_literals"] == 256


def test_random_bytes_are_stored(S, deflaters):
    data = np.random.default_rng(5).integers(0, 256, 8192, dtype=np.uint8).tobytes()
    z, st = _check(S, deflaters(1024), data, 1024)
    assert st["n_stored"] > 0 and len(z) <= 8192 + 5 * 8


@pytest.mark.parametrize("filler", ["random", "zeros"])
def test_distance_cap(S, deflaters, filler):
    """R + filler + R with the second R exactly 32768, then 32769, behind the first: the first distance may be used, the second must not
    be - zlib refuses 'distance too far back'.  Random filler overwrites the first R's hash slots; a filler of zeros leaves them, so there
    the match at the cap is found, and missed one byte further."""
    rng = np.random.default_rng(11)
    R = rng.integers(0, 256, 258, dtype=np.uint8).tobytes()
    lits = []
    for gap in (32768, 32769):
        F = rng.integers(0, 256, gap - 258, dtype=np.uint8).tobytes() if filler == "random" else bytes(gap - 258)
        z, st = _check(S, deflaters(65535), R + F + R, 65535)
        lits.append(st["n_literals"])
    if filler == "zeros":
        # R's 258 literals and the zeros of its last strip either way; the second R is one match at the cap, 258 literals past it
        assert lits[0] < 258 + 64 + 16 and lits[1] >= 2 * 258


def test_literals_only_with_a_fibonacci_histogram(S, deflaters):
    fib = [1, 1]
    while len(fib) < 24:
        fib.append(fib[-1] + fib[-2])
    rng = np.random.default_rng(2)
    data = np.repeat(np.arange(24, dtype=np.uint8) + 65, fib)
    rng.shuffle(data)
    data = data[:65535].tobytes()
    z, st = _check(S, deflaters(65535), data, 65535, S.SH_DEFLATE_LITERALS_ONLY)
    assert st["n_matches"] == 0 and st["n_literals"] == 65535 and st["n_stored"] == 0
    assert len(z) < 65535 * 3 // 8      # counts in the golden ratio: 2.5 bits of entropy a byte; a code cut at 15 bits still spends under 3


@pytest.mark.parametrize("offset", range(8))
def test_input_at_any_alignment(S, deflaters, fastq, offset):
    import torch
    n = 4099
    base = torch.frombuffer(bytearray(bytes(offset) + fastq[:n]), dtype=torch.uint8).cuda()
    d_in = base[offset:]
    assert d_in.data_ptr() % 8 == offset
    d_out = torch.zeros(S.deflate_bound(n, 1024), dtype=torch.uint8, device="cuda")
    out_len, st = deflaters(1024).deflate_device(d_in, n, d_out)
    z = d_out[:out_len].cpu().numpy().tobytes()
    assert zlib.decompress(z, -15) == fastq[:n] and st["out_bytes"] == out_len <= S.deflate_bound(n, 1024)


def test_same_bytes_from_run_to_run(S, deflaters, fastq):
    data = fastq[:1 << 20]
    a, _ = _check(S, deflaters(0), data, 0)
    b, _ = deflaters(0).deflate(data)
    c, _ = deflaters(32768).deflate(data)
    assert a == b == c


def test_fastq_beats_z_rle(S, deflaters, fastq):
    z, st = _check(S, deflaters(32768), fastq, 32768)
    rle = 0
    for o in range(0, len(fastq), 32768):
        c = zlib.compressobj(1, zlib.DEFLATED, -15, 8, zlib.Z_RLE)
        rle += len(c.compress(fastq[o:o + 32768]) + c.flush(zlib.Z_FULL_FLUSH))
    print(f"fastq {len(fastq)} bytes: device {len(z)}, Z_RLE {rle}, matches {st['n_matches']}, literals {st['n_literals']}, stored {st['n_stored']}, {st['ms']:.3f} ms")
    assert st["n_stored"] == 0 and len(z) < rle


def test_gzip_member(S, deflaters, fastq):
    for data in (fastq, b""):
        m, st = deflaters(32768).gzip_member(data)
        assert m[:10] == b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\x03"
        assert gzip.decompress(m) == data
        assert len(m) == st["out_bytes"] + 18 <= S.deflate_bound(len(data), 32768) + 18
    assert gzip.decompress(deflaters(32768).gzip_member(fastq[:5000])[0] + deflaters(1024).gzip_member(fastq[5000:9000])[0]) == fastq[:9000]


def test_refusals(S, deflaters):
    import torch
    df = deflaters(1024)
    n = 3000
    d_in = torch.zeros(n, dtype=torch.uint8, device="cuda")
    d_out = torch.zeros(S.deflate_bound(n, 1024), dtype=torch.uint8, device="cuda")
    with pytest.raises(S.ScrubbyHipError) as e:
        df.deflate_device(d_in, n, d_out, out_cap=S.deflate_bound(n, 1024) - 1)
    assert e.value.status == 1 and str(S.deflate_bound(n, 1024)) in e.value.message and "3000" in e.value.message
    with pytest.raises(S.ScrubbyHipError) as e:
        df.deflate_device(d_in, (2 << 20) + 1, d_out)
    assert e.value.status == 1 and str((2 << 20) + 1) in e.value.message
    with pytest.raises(S.ScrubbyHipError) as e:
        df.gzip_member(b"x" * n, out_cap=S.deflate_bound(n, 1024) + 17)
    assert e.value.status == 1
    with pytest.raises(S.ScrubbyHipError) as e:
        S.Deflater(1 << 20, 1000)
    assert e.value.status == 1
    out_len, st = df.deflate_device(d_in, n, d_out)      # and the deflater still works
    assert zlib.decompress(d_out[:out_len].cpu().numpy().tobytes(), -15) == bytes(n)
