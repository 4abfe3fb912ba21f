"""BAM and SAM written from Python tuples, the plain model of `scrubby alignment`'s rule on them, and the case table that
test_bam_cpu.py and test_bam_gpu.py run over the same bytes.

The rule (ReadAlignment::from_bam): a record that is not unmapped is selected iff (qalen >= min_len or qalen / l_seq >= min_cov) and
mapq >= min_mapq, qalen = the M and I ops of its CIGAR - the CG:B,I tag's when the stored CIGAR begins with <l_seq>S, the record is
placed (refID, pos >= 0) and the first CG tag is B,I with at least n_cigar_op entries, else the stored one.  The model works on the
tuples, never on the bytes, so it shares nothing with csrc/sh_bam.h.

Records are written with quality bytes 0xff, sequence bytes 0x11 and padding 'x', none of which reads as a record's length word, and are
a few hundred bytes long, so an ordinary case holds few positions at which a record may start; the decoy cases put well-formed record
headers into quality strings and B arrays on purpose."""
import math
import struct
from dataclasses import dataclass, field

from tests.bgzf_util import bgzf

OPS = "MIDNSHP=X"
M, I, D, N, S, H, P, EQ, X = range(9)
QUERY_OPS = (M, I, S, EQ, X)
LANE_CIGAR = 16          # = SHB_LANE_CIGAR (csrc/sh_bam.h): more ops than this and the whole wave sums the record
MAX_RECORD = 64 << 20    # = SHB_MAX_RECORD


@dataclass
class Rec:
    name: bytes = b"r"
    flag: int = 0
    ref: int = 0
    pos: int = 100
    mapq: int = 60
    cigar: tuple = ()
    l_seq: int = None            # None: what the CIGAR's query ops add up to
    aux: tuple = ()              # (tag, type, value) or (tag, "B", subtype, values)
    qual: bytes = None           # None: 0xff
    seq: bytes = None            # the packed bases; None: 0x11
    next_ref: int = -1
    next_pos: int = -1
    # what a corrupt case overrides
    block_size_delta: int = 0
    l_read_name: int = None
    raw_name: bytes = None       # the name field as written, NUL or not

    def qlen(self):
        return sum(n for op, n in self.cigar if op in QUERY_OPS) if self.l_seq is None else self.l_seq


def aux_bytes(aux):
    out = b""
    for t in aux:
        tag, typ = t[0].encode(), t[1]
        if typ == "B":
            sub, vals = t[2], t[3]
            out += tag + b"B" + sub.encode() + struct.pack("<I", len(vals)) + struct.pack("<%d%s" % (len(vals), {"c": "b", "C": "B", "s": "h", "S": "H", "i": "i", "I": "I", "f": "f"}[sub]), *vals)
        elif typ == "Z":
            out += tag + b"Z" + t[2] + b"\0"
        else:
            out += tag + typ.encode() + struct.pack("<" + {"A": "c", "c": "b", "C": "B", "s": "h", "S": "H", "i": "i", "I": "I", "f": "f"}[typ], t[2])
    return out


def encode(r):
    """One record: block_size and the rest, as the SAM/BAM specification lays it out."""
    l_seq = r.qlen()
    name = r.name + b"\0" if r.raw_name is None else r.raw_name
    l_read_name = len(name) if r.l_read_name is None else r.l_read_name
    cig = b"".join(struct.pack("<I", n << 4 | op) for op, n in r.cigar)
    qual = b"\xff" * l_seq if r.qual is None else r.qual
    assert len(qual) == l_seq and (r.seq is None or len(r.seq) == (l_seq + 1) // 2)
    body = struct.pack("<iiBBHHHiiii", r.ref, r.pos, l_read_name, r.mapq, 4680, len(r.cigar), r.flag, l_seq, r.next_ref, r.next_pos, 0) + name + cig + \
        (b"\x11" * ((l_seq + 1) // 2) if r.seq is None else r.seq) + qual + aux_bytes(r.aux)
    return struct.pack("<I", len(body) + r.block_size_delta) + body


def header(n_ref, text=b"@HD\tVN:1.6\n"):
    out = b"BAM\1" + struct.pack("<I", len(text)) + text + struct.pack("<I", n_ref)
    for i in range(n_ref):
        nm = b"chr%d\0" % (i + 1)
        out += struct.pack("<I", len(nm)) + nm + struct.pack("<I", 1_000_000 * (i + 1))
    return out


def filler(total, name=b"f"):
    """An unmapped record of exactly `total` bytes (38 + len(name), or 4 more at least): padding in a Z tag."""
    base = 36 + len(name) + 1
    assert total == base or total >= base + 4, total
    aux = () if total == base else (("XP", "Z", b"x" * (total - base - 4)),)
    return Rec(name=name, flag=4, ref=-1, pos=-1, mapq=0, aux=aux)


def decoy(block_size):
    """37 bytes that pass for a record's start wherever they lie: unplaced, a name of its NUL alone."""
    return struct.pack("<IiiBBHHHiiii", block_size, -1, -1, 1, 0, 4680, 0, 4, 0, -1, -1, 0) + b"\0"


# ---- the model -------------------------------------------------------------------------------------------------------------------------------
def real_cigar(r):
    if r.cigar and r.ref >= 0 and r.pos >= 0 and r.cigar[0] == (S, r.qlen()):
        for t in r.aux:
            if t[0] == "CG":
                if t[1] == "B" and t[2] == "I" and len(r.cigar) <= len(t[3]) < 1 << 29:
                    return tuple((v & 15, v >> 4) for v in t[3]), True
                break
    return r.cigar, False


def selects(r, rule):
    if r.flag & 4:
        return False
    cig, _ = real_cigar(r)
    qalen = sum(n for op, n in cig if op in (M, I))
    qlen = r.qlen()
    qcov = 0.0 if qlen == 0 else qalen / qlen
    return (qalen >= rule["min_len"] or qcov >= rule["min_cov"]) and r.mapq >= rule["min_mapq"]


def model(recs, rule):
    """-> (the names as the filter writes them, the counts the stats must show)"""
    sel = [r for r in recs if selects(r, rule)]
    names = b"".join(r.name + b"\0" for r in sel)
    return names, dict(n_records=len(recs), n_unmapped=sum(1 for r in recs if r.flag & 4), n_selected=len(sel),
                       n_cg=sum(1 for r in recs if not r.flag & 4 and real_cigar(r)[1]), name_bytes=len(names))


def rule(min_len=0, min_cov=0.0, min_mapq=0):
    return dict(min_len=min_len, min_cov=min_cov, min_mapq=min_mapq)


# ---- cases -----------------------------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    label: str
    n_ref: int
    recs: list
    rules: list
    flood: bool = False
    error_at: int = None         # corrupt: the offset "not a BAM record at" names (filled by build)
    text: bytes = b""
    starts: list = field(default_factory=list)      # offset of every record; starts[-1] = len(text)

    def build(self):
        self.text = header(self.n_ref)
        self.starts = [len(self.text)]
        for r in self.recs:
            self.text += encode(r)
            self.starts.append(len(self.text))
        return self

    @property
    def first(self):
        return self.starts[0]


ANY = [rule(), rule(min_len=100, min_cov=2.0), rule(min_len=10 ** 6, min_cov=0.5, min_mapq=30)]


def aligned(name, n_m=200, **kw):
    return Rec(name=name, cigar=((M, n_m),), **kw)


def at_offsets(seg, targets):
    """Records that start exactly at the given offsets (ascending), fillers between them."""
    recs, at = [], len(header(3))
    for k, t in enumerate(targets):
        gap = t - at
        while gap > 3000:      # fillers of a few KB
            recs.append(filler(2000, b"g%d" % k)); gap -= 2000
        recs.append(filler(gap, b"f%d" % k))
        r = aligned(b"edge%d" % k, 150 + k)
        recs.append(r)
        at = t + len(encode(r))
    return recs


def cases(seg, cap):
    """The table.  seg = sh_bam_segment(), cap = sh_bam_segment_cap()."""
    out = []
    # segment borders: starts at S-3 .. S+1 (the length word and the fixed fields straddle a border), a record longer than 2 S
    out.append(Case("border_starts", 3, at_offsets(seg, [seg - 3, 2 * seg - 2, 3 * seg - 1, 4 * seg, 5 * seg + 1]), ANY))
    out.append(Case("long_record", 3, [aligned(b"a"), Rec(name=b"long", cigar=((M, 3 * seg),)), aligned(b"b", 120), aligned(b"c", 90, mapq=3)], ANY))
    # CIGARs: 0, 1, and the lane / wave threshold -1, +0, +1 ops; 3 000 ops across segments; all nine ops, where only M and I count
    recs = [Rec(name=b"ops0", l_seq=200), aligned(b"ops1", 200)]
    for k in (LANE_CIGAR - 1, LANE_CIGAR, LANE_CIGAR + 1):
        recs.append(Rec(name=b"ops%d" % k, cigar=tuple((M, 10) if i % 2 == 0 else (D, 3) for i in range(k)), l_seq=400))
    recs.append(Rec(name=b"ops3000", cigar=tuple((M, 2) if i % 2 == 0 else (I, 1) for i in range(3000)) , l_seq=9000))
    recs.append(Rec(name=b"nine", cigar=((H, 7), (S, 20), (M, 30), (I, 5), (D, 9), (N, 1000), (EQ, 40), (X, 60), (P, 3), (M, 15), (S, 30)), l_seq=200))
    out.append(Case("cigars", 3, recs, [rule(), rule(min_len=50, min_cov=2.0), rule(min_len=51, min_cov=2.0), rule(min_len=4500, min_cov=2.0), rule(min_len=4501, min_cov=2.0),
                                         rule(min_len=10 ** 6, min_cov=0.25), rule(min_len=10 ** 6, min_cov=0.26), rule(min_len=80, min_cov=2.0), rule(min_len=81, min_cov=2.0)]))
    # CG: the real CIGAR of 70 000 ops in the tag, and the near misses that must use the stored one
    big = tuple((M, 1) if i % 2 == 0 else (D, 1) for i in range(70000))
    cg = ("CG", "B", "I", [n << 4 | op for op, n in big])
    small = ("CG", "B", "I", [200 << 4 | M, 5 << 4 | D])
    stored = ((S, 200), (N, 500))
    out.append(Case("cg", 3, [
        Rec(name=b"cg70000", cigar=((S, 35000), (N, 35000)), aux=(("NM", "i", 7), cg)),
        Rec(name=b"cg_small", cigar=stored, aux=(("XZ", "Z", b"text"), ("XB", "B", "s", [1, -2, 3]), small)),
        Rec(name=b"miss_first_op", cigar=((H, 200), (N, 500)), l_seq=200, aux=(small,)),
        Rec(name=b"miss_s_len", cigar=((S, 199), (N, 500)), l_seq=200, aux=(small,)),
        Rec(name=b"miss_no_tag", cigar=stored, aux=(("NM", "i", 7),)),
        Rec(name=b"miss_subtype_i", cigar=stored, aux=(("CG", "B", "i", [200 << 4 | M, 5 << 4 | D]),)),
        Rec(name=b"miss_ref", cigar=stored, ref=-1, aux=(small,)),
        Rec(name=b"miss_count", cigar=stored, aux=(("CG", "B", "I", [200 << 4 | M]),)),
    ], [rule(min_len=1, min_cov=2.0), rule(min_len=35000, min_cov=2.0), rule(min_len=35001, min_cov=2.0), rule()]))
    # fields: the unmapped flag, mapq 0 and 255 against min_mapq 0, 1, 255, l_seq 0, names of 0 and 254 bytes, duplicate names
    out.append(Case("fields", 3, [
        aligned(b"unmapped", flag=4), aligned(b"unmapped_paired", flag=77), aligned(b"mapq0", mapq=0), aligned(b"mapq255", mapq=255),
        Rec(name=b"lseq0", cigar=((M, 50),), l_seq=0, aux=(("XP", "Z", b"x" * 300),)), Rec(name=b"", cigar=((M, 200),)), Rec(name=b"n" * 254, cigar=((M, 200),)),
        aligned(b"dup"), aligned(b"other", 180), aligned(b"dup", 170, flag=16), aligned(b"dup", 10, l_seq=200),
    ], [rule(), rule(min_mapq=1), rule(min_mapq=255), rule(min_len=100, min_cov=2.0), rule(min_len=10 ** 6, min_cov=0.0)]))
    out.append(Case("n_ref_0", 0, [aligned(b"u%d" % i, 100 + i, ref=-1, pos=-1, mapq=10 * i) for i in range(6)], ANY))
    # coverage boundaries: qalen / qlen exactly min_cov and one ulp to either side; min_cov above 1; min_len met while coverage is not, and the reverse
    third = 50 / 150
    covs = [0.5, math.nextafter(0.5, 1.0), math.nextafter(0.5, 0.0), third, math.nextafter(third, 1.0), math.nextafter(third, 0.0), 1.5]
    out.append(Case("coverage", 3, [aligned(b"half", 100, l_seq=200), aligned(b"third", 50, l_seq=150), aligned(b"full", 200), aligned(b"tenth", 30, l_seq=300)],
                    [rule(min_len=10 ** 6, min_cov=c) for c in covs] + [rule(min_len=100, min_cov=2.0), rule(min_len=10 ** 6, min_cov=0.3), rule(min_len=30, min_cov=0.9)]))
    # decoys: well-formed record headers inside a quality string and a B array; one whose own chain leads off the true one, one that joins it
    q = bytearray(b"\xff" * 600)
    q[40:77] = decoy(33)            # its chain continues at +37: the next decoy
    q[77:114] = decoy(1000)         # leads into the middle of a later record
    q[300:337] = decoy(600 - 300 - 4 + 3 + 5 * 4 + 5)      # ends where the record's aux data ends: it joins the true chain
    arr = decoy(33) + decoy(2 * seg) + b"\xee" * 3
    out.append(Case("decoys", 3, [aligned(b"d0"), Rec(name=b"host", cigar=((M, 600),), qual=bytes(q), aux=(("XB", "B", "C", list(arr)),)), aligned(b"d1", 150),
                                   Rec(name=b"arr", cigar=((M, 100),), aux=(("XB", "B", "C", list(decoy(33) * 2)),)), aligned(b"d3", 120, mapq=3)], ANY))
    # the flood: decoys denser than the table's cap, in segments the chain enters
    flood_q = decoy(33) * (3 * seg // 2 // 37)
    out.append(Case("flood", 3, [aligned(b"before", 180)] + [Rec(name=b"flood%d" % i, cigar=((M, len(flood_q)),), qual=flood_q, mapq=10 * i) for i in range(4)] +
                    [aligned(b"after", 170), aligned(b"after2", 20)], ANY + [rule(min_mapq=20)], flood=True))
    return [c.build() for c in out]


def corrupt_cases(seg):
    """Each ends with "not a BAM record at <error_at>"."""
    def mk(label, bad, at_delta=0, k=2):
        recs = [aligned(b"c%d" % i, 100 + i) for i in range(5)]
        recs[k] = bad(recs[k])
        c = Case(label, 3, recs, [rule()]).build()
        c.error_at = c.starts[k] + at_delta
        return c

    def with_(**kw):
        return lambda r: Rec(**{**r.__dict__, **kw})
    out = [
        mk("block_size_small", with_(block_size_delta=-170)),
        mk("l_read_name_0", with_(l_read_name=0)),
        mk("name_without_nul", with_(raw_name=b"c2x")),
        mk("ref_id_beyond", with_(ref=3)),
    ]
    # a block_size one too large: record 2 still holds its fields, the chain lands one byte into record 3
    c = Case("lands_mid_record", 3, [aligned(b"c%d" % i, 100 + i) for i in range(5)], [rule()])
    c.recs[2] = Rec(**{**c.recs[2].__dict__, "block_size_delta": 1})
    c.build()
    c.error_at = c.starts[3] + 1
    out.append(c)
    # the same past a segment border: the table of the next segment is asked for a position it does not hold
    c = Case("lands_mid_record_next_segment", 3, at_offsets(seg, [seg - 400, seg + 100]), [rule()])
    k = len(c.recs) - 3      # the record that starts at seg - 400
    c.recs[k] = Rec(**{**c.recs[k].__dict__, "block_size_delta": 1})
    c.build()
    c.error_at = c.starts[k + 1] + 1
    out.append(c)
    return out


def window_cuts(case):
    """(label, cut, complete): windows text[:cut] that end inside a length word, the fixed fields, a name, and exactly at a record's end."""
    k = min(2, len(case.recs) - 1)
    s = case.starts[k]
    return [("in_length_word", s + 2, False), ("in_fixed_fields", s + 20, False), ("in_name", s + 37, False), ("at_record_end", case.starts[k + 1], True)]


# ---- files -----------------------------------------------------------------------------------------------------------------------------------
def bam_file(n_ref, recs, block=65280, **kw):
    return bgzf(header(n_ref) + b"".join(encode(r) for r in recs), block=block, **kw)


def sam_line(r):
    cigar = "".join("%d%s" % (n, OPS[op]) for op, n in r.cigar) or "*"
    qlen = r.qlen()
    return "\t".join([r.name.decode(), str(r.flag), "chr%d" % (r.ref + 1) if r.ref >= 0 else "*", str(r.pos + 1), str(r.mapq), cigar, "*", "0", "0",
                      "A" * qlen if qlen else "*", "*"])


def sam_text(n_ref, recs):
    head = "@HD\tVN:1.6\n" + "".join("@SQ\tSN:chr%d\tLN:%d\n" % (i + 1, 1_000_000 * (i + 1)) for i in range(n_ref))
    return head + "".join(sam_line(r) + "\n" for r in recs)
