"""BGZF written from bytes with Python's zlib, for the inflate tests and scripts/inflate_speed.py: raw DEFLATE streams from
compressobj(level, DEFLATED, -15, 8, strategy), wrapped in the 18-byte header with the BC subfield (the member's size - 1) and the
CRC-32 / ISIZE trailer.  The options force particular shapes of stream: level 0 (stored blocks), Z_FIXED, Z_HUFFMAN_ONLY, Z_RLE, and a
flush in mid-member (several blocks and an empty stored block inside one member).  `tamper` arguments write members that are wrong on
purpose."""
import struct
import zlib

BLOCK = 65280      # what bgzip cuts its input at
SHAPES = {
    "stored": dict(level=0),
    "fixed": dict(level=6, strategy=zlib.Z_FIXED),
    "huffman_only": dict(level=6, strategy=zlib.Z_HUFFMAN_ONLY),
    "rle": dict(level=6, strategy=zlib.Z_RLE),
    "level1": dict(level=1),
    "level6": dict(level=6),
    "level9": dict(level=9),
    "full_flush": dict(level=6, flush_at=0.4, flush=zlib.Z_FULL_FLUSH),
    "sync_flush": dict(level=6, flush_at=0.1, flush=zlib.Z_SYNC_FLUSH),
}


def raw_deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=None, flush=zlib.Z_FULL_FLUSH):
    """One raw DEFLATE stream; flush_at (a fraction of the input): a flush there, which ends the block, appends an empty stored block
    and goes on with a new block."""
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    if flush_at is None or len(data) < 2:
        return c.compress(data) + c.flush()
    k = max(1, int(len(data) * flush_at))
    return c.compress(data[:k]) + c.flush(flush) + c.compress(data[k:]) + c.flush()


def wrap(raw, data, extra_before=b"", fname=None, fhcrc=False, crc=None, isize=None):
    """The gzip member around a raw stream that inflates to `data`: FEXTRA with BC (after `extra_before`, other subfields), FNAME and
    FHCRC on request; crc / isize replace the true trailer values."""
    flg = 4 | (8 if fname is not None else 0) | (2 if fhcrc else 0)
    xlen = len(extra_before) + 6
    tail = (fname + b"\0" if fname is not None else b"")
    size = 12 + xlen + len(tail) + (2 if fhcrc else 0) + len(raw) + 8
    head = struct.pack("<4BI2BH", 0x1F, 0x8B, 8, flg, 0, 0, 0xFF, xlen) + extra_before + struct.pack("<2BHH", 66, 67, 2, size - 1) + tail
    if fhcrc:
        head += struct.pack("<H", zlib.crc32(head) & 0xFFFF)
    return head + raw + struct.pack("<II", zlib.crc32(data) if crc is None else crc, len(data) if isize is None else isize)


def member(data, **kw):
    wrap_kw = {k: kw.pop(k) for k in ("extra_before", "fname", "fhcrc", "crc", "isize") if k in kw}
    return wrap(raw_deflate(data, **kw), data, **wrap_kw)


EOF = member(b"")      # the empty end-of-file member: 28 bytes


def bgzf(data, block=BLOCK, eof=True, **kw):
    """`data` as a BGZF file: members of `block` bytes and the end-of-file member."""
    out = [member(data[o:o + block], **kw) for o in range(0, len(data), block)]
    return b"".join(out) + (EOF if eof else b"")


def n_members(data, block=BLOCK, eof=True):
    return -(-len(data) // block) + (1 if eof else 0)
