// sh_bam.h — the pure parts of the BAM record filter behind `scrubby alignment` (DESIGN.md §6 "SAM / BAM"), shared by the device kernels
// (sh_bam.hip), the host mirror (sh_bam_filter_host) and tests/bam_host.cpp: the header parse, the ONE predicate that says whether a
// record may start at a position, and the decision of a record (ReadAlignment::from_bam, /root/reference/src/alignment.rs:115-211:
// qalen = the M and I ops of the CIGAR, qlen = l_seq, selected iff (qalen >= min_len || qcov >= min_cov) && mapq >= min_mapq).
// The record layout is the SAM/BAM specification's (section 4.2).  The CIGAR of a record that keeps it in the CG:B,I tag is taken from
// there under the conditions of htslib's bam_tag2cigar as recalled: PARITY WITH htslib UNPINNED.
//
// Everything is written against one abstraction, as sh_inflate.h is:
//   Src   uint32_t byte(uint64_t pos)      byte `pos` of the window text[0, n); asked for pos < n only
// so the host build and the kernels share every decision, the double division included.
#pragma once
#include <stdint.h>
#include <stddef.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SHB_FN __host__ __device__ inline
#else
#define SHB_FN inline
#endif

#define SHB_MAX_RECORD (64u << 20)      // block_size above this is no record: a read of 40 Mb with qualities still fits
#define SHB_SEGMENT 4096u               // bytes of the window one wave probes (sh_bam_segment)
#define SHB_SEGMENT_CAP 64u             // plausible starts a segment's table holds, one per lane (sh_bam_segment_cap)
#define SHB_LANE_CIGAR 16u              // a record with more CIGAR ops than this is summed by the whole wave, else by the lane that has it
#define SHB_MIN_STEP 37u                // 4 + the least block_size (32 fixed bytes and a name of its NUL): no chain step is shorter
#define SHB_HALO (36u + 255u)           // bytes behind a position that shb_record_ok may ask for

enum { SHB_HDR_OK = 0, SHB_HDR_MORE = 1, SHB_HDR_NOT_BAM = 2 };

// same layout as sh_bam_rule (include/scrubby_hip.h)
struct ShbRule { uint64_t min_len; double min_cov; uint32_t min_mapq; int32_t n_ref; };
// what a record is decided on
struct ShbRec {
    uint64_t name_off, cig_off;      // the name's first byte; the first CIGAR word (the stored CIGAR's, or the CG tag's)
    uint32_t block_size, name_len, cig_n, flag, mapq;
    int32_t l_seq;
    uint32_t cg;                     // 1: cig_off / cig_n are the CG tag's
};

struct ShbPtrSrc {
    const uint8_t *p;
    SHB_FN uint32_t byte(uint64_t pos) const { return p[pos]; }
};

template <class Src> SHB_FN uint32_t shb_u16(const Src &s, uint64_t p) { return s.byte(p) | s.byte(p + 1) << 8; }
template <class Src> SHB_FN uint32_t shb_u32(const Src &s, uint64_t p) { return s.byte(p) | s.byte(p + 1) << 8 | s.byte(p + 2) << 16 | s.byte(p + 3) << 24; }
template <class Src> SHB_FN int32_t shb_i32(const Src &s, uint64_t p) { return (int32_t)shb_u32(s, p); }

// ---- the header: magic, l_text, text, n_ref, and per reference l_name, name, l_ref ----------------------------------------------------------
// SHB_HDR_OK: *n_ref and *first_record (the offset of the first record) are set.  SHB_HDR_MORE: text[0, n) is a prefix of a header.
template <class Src> inline int shb_header(const Src &src, uint64_t n, int32_t *n_ref, uint64_t *first_record)
{
    const uint8_t magic[4] = {'B', 'A', 'M', 1};
    for (uint64_t i = 0; i < 4 && i < n; ++i) if (src.byte(i) != magic[i]) return SHB_HDR_NOT_BAM;
    if (n < 8) return SHB_HDR_MORE;
    uint64_t p = 8 + (uint64_t)shb_u32(src, 4);
    if (n < p + 4) return SHB_HDR_MORE;
    const uint32_t refs = shb_u32(src, p);
    if (refs > 0x7fffffffu) return SHB_HDR_NOT_BAM;
    p += 4;
    for (uint32_t i = 0; i < refs; ++i) {
        if (n < p + 4) return SHB_HDR_MORE;
        p += 4 + (uint64_t)shb_u32(src, p) + 4;
    }
    if (n < p) return SHB_HDR_MORE;
    *n_ref = (int32_t)refs; *first_record = p;
    return SHB_HDR_OK;
}

// ---- the predicate: "a record may start at p" and "the record at p is well formed" are the same question --------------------------------
// Judged on as many of the record's bytes as lie below n (p <= n): a check whose bytes are cut off by the window's end passes.
template <class Src> SHB_FN bool shb_record_ok(const Src &src, uint64_t p, uint64_t n, int32_t n_ref)
{
    const uint64_t have = n - p;
    if (have < 4) return true;
    const uint32_t block_size = shb_u32(src, p);
    if (block_size < SHB_MIN_STEP - 4 || block_size > SHB_MAX_RECORD) return false;
    if (have < 8) return true;
    const int32_t ref_id = shb_i32(src, p + 4);
    if (ref_id < -1 || ref_id >= n_ref) return false;
    if (have < 12) return true;
    if (shb_i32(src, p + 8) < -1) return false;
    if (have < 13) return true;
    const uint32_t l_read_name = src.byte(p + 12);
    if (l_read_name == 0) return false;
    if (have < 24) return true;
    const uint32_t n_cigar_op = shb_u16(src, p + 16);
    const int32_t l_seq = shb_i32(src, p + 20);
    if (l_seq < 0) return false;
    if ((uint64_t)block_size < 32ull + l_read_name + 4ull * n_cigar_op + ((uint64_t)l_seq + 1) / 2 + (uint64_t)l_seq) return false;
    if (have < 28) return true;
    const int32_t next_ref = shb_i32(src, p + 24);
    if (next_ref < -1 || next_ref >= n_ref) return false;
    if (have < 32) return true;
    if (shb_i32(src, p + 28) < -1) return false;
    const uint64_t name_end = 36ull + l_read_name - 1;
    if (have <= name_end) return true;
    return src.byte(p + name_end) == 0;
}

// the record at p lies in the window whole
template <class Src> SHB_FN bool shb_complete(const Src &src, uint64_t p, uint64_t n)
{
    return n - p >= 4 && n - p - 4 >= (uint64_t)shb_u32(src, p);
}

SHB_FN uint32_t shb_aux_size(uint32_t type)
{
    switch (type) {
    case 'A': case 'c': case 'C': return 1;
    case 's': case 'S': return 2;
    case 'i': case 'I': case 'f': return 4;
    default: return 0;
    }
}

// ---- the fields of a record that is ok and complete; every read stays inside the record ---------------------------------------------------
template <class Src> SHB_FN ShbRec shb_fields(const Src &src, uint64_t p)
{
    ShbRec r;
    r.block_size = shb_u32(src, p);
    const uint32_t l_read_name = src.byte(p + 12), n_cigar_op = shb_u16(src, p + 16);
    r.mapq = src.byte(p + 13);
    r.flag = shb_u16(src, p + 18);
    r.l_seq = shb_i32(src, p + 20);
    r.name_off = p + 36;
    r.name_len = l_read_name - 1;
    r.cig_off = p + 36 + l_read_name;
    r.cig_n = n_cigar_op;
    r.cg = 0;
    // bam_tag2cigar: a mapped record whose stored CIGAR begins with <l_seq>S may keep the real one in CG:B,I
    if (n_cigar_op == 0 || shb_i32(src, p + 4) < 0 || shb_i32(src, p + 8) < 0) return r;
    const uint32_t first = shb_u32(src, r.cig_off);
    if ((first & 15u) != 4u || (first >> 4) != (uint32_t)r.l_seq) return r;
    const uint64_t end = p + 4 + r.block_size;
    uint64_t a = r.cig_off + 4ull * n_cigar_op + ((uint64_t)r.l_seq + 1) / 2 + (uint64_t)r.l_seq;
    while (a + 3 <= end) {      // the first CG tag decides, as bam_aux_get finds the first; aux data that does not parse ends the search
        const bool is_cg = src.byte(a) == 'C' && src.byte(a + 1) == 'G';
        const uint32_t type = src.byte(a + 2);
        a += 3;
        if (is_cg && type != 'B') break;
        if (type == 'Z' || type == 'H') {
            while (a < end && src.byte(a) != 0) ++a;
            if (a >= end) break;
            ++a;
        } else if (type == 'B') {
            if (a + 5 > end) break;
            const uint32_t sub = src.byte(a), count = shb_u32(src, a + 1), size = shb_aux_size(sub);
            const uint64_t bytes = (uint64_t)count * size;
            if (size == 0 || sub == 'A' || bytes > end - (a + 5)) break;
            if (is_cg) {
                if (sub == 'I' && count >= n_cigar_op && count < (1u << 29)) { r.cig_off = a + 5; r.cig_n = count; r.cg = 1; }
                break;
            }
            a += 5 + bytes;
        } else {
            const uint32_t size = shb_aux_size(type);
            if (size == 0 || size > end - a) break;
            a += size;
        }
    }
    return r;
}

// the query bases the CIGAR words first, first + step, .. align: ops M (0) and I (1) only, as qalen_from_cigar matches Match and Ins
template <class Src> SHB_FN uint64_t shb_qalen(const Src &src, const ShbRec &r, uint32_t first, uint32_t step)
{
    uint64_t sum = 0;
    for (uint32_t i = first; i < r.cig_n; i += step) {
        const uint32_t w = shb_u32(src, r.cig_off + 4ull * i);
        if ((w & 15u) <= 1u) sum += w >> 4;
    }
    return sum;
}

SHB_FN bool shb_select(const ShbRec &r, uint64_t qalen, const ShbRule &rule)
{
    if (r.flag & 4u) return false;
    const uint64_t qlen = (uint64_t)r.l_seq;
    const double qcov = qlen == 0 ? 0.0 : (double)qalen / (double)qlen;
    return (qalen >= rule.min_len || qcov >= rule.min_cov) && r.mapq >= rule.min_mapq;
}

// the whole decision of the record at p by one caller
template <class Src> SHB_FN bool shb_decide(const Src &src, uint64_t p, const ShbRule &rule, ShbRec *rec)
{
    *rec = shb_fields(src, p);
    if (rec->flag & 4u) return false;
    return shb_select(*rec, shb_qalen(src, *rec, 0, 1), rule);
}

// the most name bytes (each name with its NUL) the records of n window bytes give: a record of 36 + l_read_name bytes at least gives
// l_read_name of them, and l_read_name <= 255
SHB_FN uint64_t shb_names_bound(uint64_t n) { return n / 291 * 255 + 255; }

// ---- the serial walk: the host mirror, and the device path's way through segments whose table overflowed -------------------------------------
struct ShbCounts { uint64_t n_records, n_unmapped, n_selected, n_cg, n_segments, name_bytes; };
enum { SHB_WALK_END = 0, SHB_WALK_OPEN = 1, SHB_WALK_BROKEN = 2, SHB_WALK_CAP = 3 };

// Walks the chain from `entry` while the position is below `stop` (<= n).  Names of the selected records go to names[*names_len ..), each
// with its NUL.  Returns how it ended and *pos: the first chain position at or past stop (END), the incomplete record (OPEN), the
// position that is no record (BROKEN), or the record whose name did not fit (CAP).  *last_seg: the segment of the last record counted
// in n_segments, ~0 before any.
template <class Src>
inline int shb_walk(const Src &src, uint64_t n, uint64_t entry, uint64_t stop, const ShbRule &rule, uint8_t *names, uint64_t names_cap, uint64_t *names_len, uint64_t *pos,
                    ShbCounts *c, uint64_t *last_seg)
{
    uint64_t p = entry;
    while (p < stop) {
        if (!shb_record_ok(src, p, n, rule.n_ref)) { *pos = p; return SHB_WALK_BROKEN; }
        if (!shb_complete(src, p, n)) { *pos = p; return SHB_WALK_OPEN; }
        ShbRec r;
        const bool sel = shb_decide(src, p, rule, &r);
        if (sel) {
            if (names_cap - *names_len < (uint64_t)r.name_len + 1) { *pos = p; return SHB_WALK_CAP; }
            for (uint32_t i = 0; i < r.name_len; ++i) names[*names_len + i] = (uint8_t)src.byte(r.name_off + i);
            names[*names_len + r.name_len] = 0;
            *names_len += r.name_len + 1;
            c->name_bytes += r.name_len + 1;
            ++c->n_selected;
        }
        ++c->n_records;
        if (r.flag & 4u) ++c->n_unmapped; else if (r.cg) ++c->n_cg;
        if (p / SHB_SEGMENT != *last_seg) { *last_seg = p / SHB_SEGMENT; ++c->n_segments; }
        p += 4 + (uint64_t)r.block_size;
    }
    *pos = p;
    return SHB_WALK_END;
}
