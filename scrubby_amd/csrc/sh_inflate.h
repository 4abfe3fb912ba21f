// sh_inflate.h — the pure parts of the BGZF / DEFLATE (RFC 1951, RFC 1952) decoder, shared by the device kernel (sh_inflate.hip) and
// the host (tests/inflate_host.cpp): the scan of BGZF member headers, canonical decode tables from code lengths, the bit reader and the
// block decoder, and CRC-32 in pieces.  The mirror of sh_deflate.h.
//
// The decoder is written against two abstractions, so that the host build and the kernel share every decision:
//   Src   uint32_t byte(uint32_t pos)                  the member's compressed byte `pos`; the decoder asks for pos < in_len only
//   Sink  void lit(uint32_t c), void match(uint32_t len, uint32_t dist), void raw(uint32_t in_pos, uint32_t n)
//         the decoder calls them only after it has checked the output extent and the distance, so a sink never has to refuse.
// On the device every lane of the wave runs the decoder with the same values (SHIN_UNI makes what comes out of LDS scalar again).
#pragma once
#include <stdint.h>
#include <stddef.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SHIN_FN __host__ __device__ inline
#else
#define SHIN_FN inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define SHIN_UNI(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))
#else
#define SHIN_UNI(x) ((uint32_t)(x))
#endif

// what a member ends with
enum {
    SHIN_OK = 0,
    SHIN_BAD_BTYPE = 1,        // block type 3
    SHIN_BAD_LENGTHS = 2,      // a set of code lengths zlib's inflate_table refuses, too many symbols, a repeat without a length before it, no end-of-block code
    SHIN_BAD_SYMBOL = 3,       // bits that are no code of an incomplete code, length symbols 286 / 287, distance symbols 30 / 31
    SHIN_DIST_FAR = 4,         // a distance past the bytes this member has produced
    SHIN_IN_OVERRUN = 5,       // the data asks for bits past the member's input extent
    SHIN_OUT_OVERRUN = 6,      // the data holds more than ISIZE bytes
    SHIN_OUT_SHORT = 7,        // the last block ended with fewer than ISIZE bytes
    SHIN_STORED_LEN = 8,       // a stored block whose NLEN is not ~LEN
    SHIN_CRC = 9,              // the bytes are not the ones the trailer's CRC-32 was taken over
    // what a span of a general gzip stream ends with besides (shin_inflate_span)
    SHIN_SPAN_END = 10,        // a member's trailer with no gzip member behind it: the stream is over, what follows is ignored as zlib's gzread ignores it
    SHIN_MANY_ENDS = 11,       // more than SHIN_MAX_ENDS members end inside one span
    SHIN_BAD_HEADER = 12,      // a gzip header with another method than 8, reserved flags, or a header CRC that does not hold
    SHIN_SIZE_DIFFERS = 13,    // the second decode of a span did not end where the first one did
    SHIN_ISIZE = 14            // the member's length is not the trailer's ISIZE modulo 2^32
};

#define SHIN_MAX_ISIZE 65536u
#define SHIN_LIT_BITS 10       // a FASTQ member's literal codes are 3..10 bits; longer codes take the canonical walk
#define SHIN_DIST_BITS 8
#define SHIN_CL_BITS 7         // the code-length code has at most 7 bits: its table is complete
#define SHIN_N_LIT 288         // the fixed code names 288 / 32 symbols; a dynamic block at most 286 / 30
#define SHIN_N_DIST 32
#define SHIN_N_CL 19

// same layout as sh_gz_member (include/scrubby_hip.h)
struct ShinMember { uint64_t file_off, in_off; uint32_t in_len, out_len, crc32, status; };

// ---- the BGZF member scan (host) ---------------------------------------------------------------------------------------------------------
// Walks the gzip member headers of buf[0, n): 1f 8b 08 FLG, FEXTRA with the BC subfield (the member's size - 1), FNAME / FCOMMENT / FHCRC
// skipped.  members[0, cap) receive what is found; *consumed is the offset of the first member not taken.
// Returns why it stopped: 0 the end of the buffer (or cap members), 1 a member that runs past the buffer (its header included: the
// buffer is a window of a file), 2 a member that is not BGZF (not gzip, reserved flags, no BC, too small for its own header and trailer,
// ISIZE above 65 536).
inline int shin_bgzf_scan(const uint8_t *buf, uint64_t n, ShinMember *members, uint64_t cap, uint64_t *n_members, uint64_t *consumed)
{
    uint64_t p = 0, k = 0;
    int stopped = 0;
    while (p < n && k < cap) {
        const uint64_t avail = n - p;
        const uint8_t magic[3] = {0x1f, 0x8b, 8};
        bool is_gzip = true;
        for (uint64_t i = 0; i < 3 && i < avail; ++i) if (buf[p + i] != magic[i]) is_gzip = false;
        if (!is_gzip) { stopped = 2; break; }
        if (avail < 4) { stopped = 1; break; }
        const uint32_t flg = buf[p + 3];
        if ((flg & 0xe0) || !(flg & 4)) { stopped = 2; break; }
        if (avail < 12) { stopped = 1; break; }
        const uint64_t xlen = (uint64_t)buf[p + 10] | (uint64_t)buf[p + 11] << 8, xend = p + 12 + xlen;
        if (xend > n) { stopped = 1; break; }
        uint64_t bsize = 0;
        for (uint64_t q = p + 12; q + 4 <= xend;) {
            const uint64_t slen = (uint64_t)buf[q + 2] | (uint64_t)buf[q + 3] << 8;
            if (q + 4 + slen > xend) break;
            if (buf[q] == 66 && buf[q + 1] == 67 && slen == 2) { bsize = ((uint64_t)buf[q + 4] | (uint64_t)buf[q + 5] << 8) + 1; break; }
            q += 4 + slen;
        }
        if (!bsize) { stopped = 2; break; }
        const uint64_t end = p + bsize;
        if (end > n) { stopped = 1; break; }
        uint64_t q = xend;
        bool fits = true;
        for (uint32_t bit = 8; bit <= 16 && fits; bit <<= 1)      // FNAME, FCOMMENT: zero-terminated
            if (flg & bit) { while (q < end && buf[q]) ++q; if (q >= end) fits = false; else ++q; }
        if (flg & 2) q += 2;
        if (!fits || q + 8 > end) { stopped = 2; break; }
        const uint8_t *t = buf + end - 8;
        const uint32_t crc = (uint32_t)t[0] | (uint32_t)t[1] << 8 | (uint32_t)t[2] << 16 | (uint32_t)t[3] << 24;
        const uint32_t isize = (uint32_t)t[4] | (uint32_t)t[5] << 8 | (uint32_t)t[6] << 16 | (uint32_t)t[7] << 24;
        if (isize > SHIN_MAX_ISIZE) { stopped = 2; break; }
        members[k++] = ShinMember{p, q, (uint32_t)(end - 8 - q), isize, crc, 0};
        p = end;
    }
    *n_members = k; *consumed = p;
    return stopped;
}

// ---- decode tables -------------------------------------------------------------------------------------------------------------------------
// A code is decoded by one look-up of its first `fast_bits` bits (entry = length << 9 | symbol, 0 = not in the table) and, for a longer
// code or bits that are no code, by the canonical walk over count[] / sorted[] (one bit a step).
struct ShinTables {
    uint16_t lit_fast[1u << SHIN_LIT_BITS], dist_fast[1u << SHIN_DIST_BITS], cl_fast[1u << SHIN_CL_BITS];
    uint16_t lit_sorted[SHIN_N_LIT], dist_sorted[SHIN_N_DIST], cl_sorted[SHIN_N_CL + 1];      // symbols by (length, symbol)
    uint16_t lit_count[16], dist_count[16], cl_count[16];                                     // codes per length
    uint16_t offs[16];
    uint8_t lens[SHIN_N_LIT + SHIN_N_DIST];
};

enum { SHIN_KIND_CL = 0, SHIN_KIND_LIT = 1, SHIN_KIND_DIST = 2 };

SHIN_FN uint32_t shin_bit_reverse(uint32_t v, uint32_t n)
{
    uint32_t r = 0;
    for (uint32_t i = 0; i < n; ++i) { r = r << 1 | (v & 1); v >>= 1; }
    return r;
}

// Tables of lens[0, n) (each 0..15).  Refuses what zlib's inflate_table refuses: an over-subscribed set, and an incomplete one unless it
// is a literal/length or distance code of ONE code of one bit.  No code at all is taken (a block of literals has no distance code; the
// caller refuses a literal/length code without the end-of-block symbol), except for the code-length code, which then decodes nothing.
// On the device all 64 lanes of the wave run this with the same values and store the same value to the same LDS address (count, offs,
// sorted, fast; the caller's lens likewise).  That is intended: the wave executes each LDS instruction for all lanes at once and its LDS
// operations complete in order, so every read-modify-write sees what the wave wrote before.  It is what keeps one code path for host and
// device; a lane-parallel build (count per length, offsets, scatter) is the first thing a faster kernel would change.
SHIN_FN int shin_build_table(const uint8_t *lens, uint32_t n, uint32_t fast_bits, int kind, uint16_t *fast, uint16_t *sorted, uint16_t *count, uint16_t *offs)
{
    for (uint32_t l = 0; l < 16; ++l) count[l] = 0;
    for (uint32_t s = 0; s < n; ++s) { const uint32_t l = SHIN_UNI(lens[s]) & 15u; count[l] = (uint16_t)(SHIN_UNI(count[l]) + 1); }
    for (uint32_t i = 0; i < (1u << fast_bits); ++i) fast[i] = 0;
    if (SHIN_UNI(count[0]) == n) return kind == SHIN_KIND_CL ? SHIN_BAD_LENGTHS : SHIN_OK;
    int32_t left = 1;
    uint32_t max_len = 0;
    for (uint32_t l = 1; l < 16; ++l) {
        const uint32_t c = SHIN_UNI(count[l]);
        left = (left << 1) - (int32_t)c;
        if (left < 0) return SHIN_BAD_LENGTHS;
        if (c) max_len = l;
    }
    if (left > 0 && (kind == SHIN_KIND_CL || max_len != 1)) return SHIN_BAD_LENGTHS;
    offs[1] = 0;
    for (uint32_t l = 1; l < 15; ++l) offs[l + 1] = (uint16_t)(SHIN_UNI(offs[l]) + SHIN_UNI(count[l]));
    for (uint32_t s = 0; s < n; ++s) {
        const uint32_t l = SHIN_UNI(lens[s]) & 15u;
        if (l) { const uint32_t o = SHIN_UNI(offs[l]); sorted[o] = (uint16_t)s; offs[l] = (uint16_t)(o + 1); }
    }
    uint32_t code = 0, idx = 0;
    for (uint32_t l = 1; l <= fast_bits; ++l) {
        const uint32_t c = SHIN_UNI(count[l]);
        for (uint32_t k = 0; k < c; ++k, ++idx, ++code) {
            const uint16_t e = (uint16_t)(l << 9 | SHIN_UNI(sorted[idx]));
            for (uint32_t j = shin_bit_reverse(code, l); j < (1u << fast_bits); j += 1u << l) fast[j] = e;
        }
        code <<= 1;
    }
    return SHIN_OK;
}

// the symbol the low bits of `acc` begin with and its length; SHIN_BAD_SYMBOL when 15 bits are no code
SHIN_FN int shin_decode_sym(uint64_t acc, const uint16_t *fast, uint32_t fast_bits, const uint16_t *count, const uint16_t *sorted, uint32_t *sym, uint32_t *len)
{
    const uint32_t e = SHIN_UNI(fast[(uint32_t)acc & ((1u << fast_bits) - 1)]);
    if (e) { *sym = e & 0x1ffu; *len = e >> 9; return SHIN_OK; }
    uint32_t code = 0, first = 0, index = 0;
    for (uint32_t l = 1; l < 16; ++l) {
        code |= (uint32_t)(acc >> (l - 1)) & 1u;
        const uint32_t c = SHIN_UNI(count[l]);
        if (code < first + c) { *sym = SHIN_UNI(sorted[index + (code - first)]); *len = l; return SHIN_OK; }
        index += c; first = (first + c) << 1; code <<= 1;
    }
    return SHIN_BAD_SYMBOL;
}

// length symbol 257..285 -> base and extra bits; distance symbol 0..29 -> base and extra bits (RFC 1951 3.2.5, in closed form)
SHIN_FN uint32_t shin_len_base(uint32_t sym, uint32_t *n_extra)
{
    const uint32_t i = sym - 257;
    if (sym == 285) { *n_extra = 0; return 258; }
    if (i < 8) { *n_extra = 0; return 3 + i; }
    const uint32_t e = (i - 4) >> 2;
    *n_extra = e;
    return 3 + ((4 + (i & 3)) << e);
}
SHIN_FN uint32_t shin_dist_base(uint32_t sym, uint32_t *n_extra)
{
    if (sym < 4) { *n_extra = 0; return sym + 1; }
    const uint32_t e = (sym - 2) >> 1;
    *n_extra = e;
    return 1 + ((2 + (sym & 1)) << e);
}

// ---- the bit reader: LSB first, at most 64 bits held, every byte asked of the source lies inside [0, in_len) -----------------------------
struct ShinBits { uint64_t acc; uint32_t n, pos, in_len; };

template <class Src>
SHIN_FN void shin_refill(ShinBits *b, Src &src)
{
    while (b->n <= 56 && b->pos < b->in_len) { b->acc |= (uint64_t)src.byte(b->pos) << b->n; ++b->pos; b->n += 8; }
}
SHIN_FN uint32_t shin_peek(const ShinBits *b, uint32_t k) { return (uint32_t)b->acc & ((1u << k) - 1); }      // k <= 16
SHIN_FN void shin_drop(ShinBits *b, uint32_t k) { b->acc >>= k; b->n -= k; }                                   // k <= n

// ---- what a block's header holds, checked as zlib checks it before a token is decoded ---------------------------------------------------
SHIN_FN void shin_fixed_lengths(ShinTables *T)
{
    for (uint32_t s = 0; s < SHIN_N_LIT; ++s) T->lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
    for (uint32_t s = 0; s < SHIN_N_DIST; ++s) T->lens[SHIN_N_LIT + s] = 5;
}

// The header of a dynamic block behind its three type bits: HLIT, HDIST, HCLEN, the code-length code (its table is left in T) and the
// HLIT + HDIST lengths, which go to T->lens[0, n_lit) and T->lens[SHIN_N_LIT, + n_dist).
template <class Src>
SHIN_FN uint32_t shin_dynamic_lengths(ShinBits *b, Src &src, ShinTables *T, uint32_t *n_lit_out, uint32_t *n_dist_out)
{
    shin_refill(b, src);
    if (b->n < 14) return SHIN_IN_OVERRUN;
    const uint32_t n_lit = shin_peek(b, 5) + 257, n_dist = (shin_peek(b, 10) >> 5) + 1, n_cl = (shin_peek(b, 14) >> 10) + 4;
    shin_drop(b, 14);
    if (n_lit > 286 || n_dist > 30) return SHIN_BAD_LENGTHS;
    for (uint32_t s = 0; s < SHIN_N_CL; ++s) T->lens[s] = 0;
    for (uint32_t i = 0; i < n_cl; ++i) {
        // 16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15
        const uint32_t perm = i < 3 ? 16 + i : i == 3 ? 0 : (i & 1) ? 8 - ((i - 3) >> 1) : 8 + ((i - 4) >> 1);
        shin_refill(b, src);
        if (b->n < 3) return SHIN_IN_OVERRUN;
        T->lens[perm] = (uint8_t)shin_peek(b, 3);
        shin_drop(b, 3);
    }
    if (shin_build_table(T->lens, SHIN_N_CL, SHIN_CL_BITS, SHIN_KIND_CL, T->cl_fast, T->cl_sorted, T->cl_count, T->offs) != SHIN_OK) return SHIN_BAD_LENGTHS;
    const uint32_t total = n_lit + n_dist;
    for (uint32_t i = 0; i < total;) {
        uint32_t sym, len;
        shin_refill(b, src);
        if (shin_decode_sym(b->acc, T->cl_fast, SHIN_CL_BITS, T->cl_count, T->cl_sorted, &sym, &len) != SHIN_OK) return SHIN_BAD_SYMBOL;
        const uint32_t n_extra = sym < 16 ? 0 : sym == 16 ? 2 : sym == 17 ? 3 : 7;
        if (b->n < len + n_extra) return SHIN_IN_OVERRUN;
        shin_drop(b, len);
        if (sym < 16) { T->lens[i++] = (uint8_t)sym; continue; }
        if (sym == 16 && i == 0) return SHIN_BAD_LENGTHS;
        const uint32_t v = sym == 16 ? SHIN_UNI(T->lens[i - 1]) : 0, rep = (sym == 18 ? 11 : 3) + shin_peek(b, n_extra);
        shin_drop(b, n_extra);
        if (i + rep > total) return SHIN_BAD_LENGTHS;
        for (uint32_t k = 0; k < rep; ++k) T->lens[i++] = (uint8_t)v;
    }
    if (SHIN_UNI(T->lens[256]) == 0) return SHIN_BAD_LENGTHS;
    // the distance lengths to their own place, so that both builds read lens[0, n)
    for (uint32_t s = n_dist; s-- > 0;) T->lens[SHIN_N_LIT + s] = (uint8_t)SHIN_UNI(T->lens[n_lit + s]);
    *n_lit_out = n_lit; *n_dist_out = n_dist;
    return SHIN_OK;
}

SHIN_FN uint32_t shin_block_tables(ShinTables *T, uint32_t n_lit, uint32_t n_dist)
{
    if (shin_build_table(T->lens, n_lit, SHIN_LIT_BITS, SHIN_KIND_LIT, T->lit_fast, T->lit_sorted, T->lit_count, T->offs) != SHIN_OK) return SHIN_BAD_LENGTHS;
    if (shin_build_table(T->lens + SHIN_N_LIT, n_dist, SHIN_DIST_BITS, SHIN_KIND_DIST, T->dist_fast, T->dist_sorted, T->dist_count, T->offs) != SHIN_OK) return SHIN_BAD_LENGTHS;
    return SHIN_OK;
}

// The tokens of one fixed or dynamic block up to its end-of-block symbol.  A distance may reach `back` bytes before output byte `base`
// (a member: 0 before its first byte; a span that began inside a member: the 32 KiB that precede it).
template <class Src, class Sink>
SHIN_FN uint32_t shin_block_tokens(ShinBits *b, Src &src, Sink &sink, const ShinTables *T, uint32_t *produced_io, uint32_t out_len, uint32_t base, uint32_t back)
{
    uint32_t produced = *produced_io, status = SHIN_OK;
#define SHIN_FAIL(code) do { status = (code); goto done; } while (0)
#define SHIN_NEED(k) do { if (b->n < (k)) SHIN_FAIL(SHIN_IN_OVERRUN); } while (0)
    for (;;) {
        uint32_t sym, len, n_extra;
        shin_refill(b, src);      // 57 bits or the rest of the input: a token takes at most 15 + 5 + 15 + 13
        if (shin_decode_sym(b->acc, T->lit_fast, SHIN_LIT_BITS, T->lit_count, T->lit_sorted, &sym, &len) != SHIN_OK) SHIN_FAIL(SHIN_BAD_SYMBOL);
        SHIN_NEED(len);
        shin_drop(b, len);
        if (sym < 256) {
            if (produced >= out_len) SHIN_FAIL(SHIN_OUT_OVERRUN);
            sink.lit(sym);
            ++produced;
            continue;
        }
        if (sym == 256) break;
        if (sym > 285) SHIN_FAIL(SHIN_BAD_SYMBOL);
        uint32_t mlen = shin_len_base(sym, &n_extra);
        SHIN_NEED(n_extra);
        mlen += shin_peek(b, n_extra);
        shin_drop(b, n_extra);
        if (shin_decode_sym(b->acc, T->dist_fast, SHIN_DIST_BITS, T->dist_count, T->dist_sorted, &sym, &len) != SHIN_OK) SHIN_FAIL(SHIN_BAD_SYMBOL);
        SHIN_NEED(len);
        shin_drop(b, len);
        if (sym > 29) SHIN_FAIL(SHIN_BAD_SYMBOL);
        uint32_t dist = shin_dist_base(sym, &n_extra);
        SHIN_NEED(n_extra);
        dist += shin_peek(b, n_extra);
        shin_drop(b, n_extra);
        if (dist > produced - base + back) SHIN_FAIL(SHIN_DIST_FAR);
        if (mlen > out_len - produced) SHIN_FAIL(SHIN_OUT_OVERRUN);
        sink.match(mlen, dist);
        produced += mlen;
    }
done:
#undef SHIN_FAIL
#undef SHIN_NEED
    *produced_io = produced;
    return status;
}

struct ShinResult { uint32_t status, produced, n_stored, n_fixed, n_dynamic; };

// One member: any number of stored, fixed and dynamic blocks up to the one with BFINAL.  out_len is the trailer's ISIZE: the member ends
// with SHIN_OUT_OVERRUN before the sink sees a byte past it, and with SHIN_OUT_SHORT when the last block ends below it.
template <class Src, class Sink>
SHIN_FN void shin_inflate_member(Src &src, uint32_t in_len, Sink &sink, uint32_t out_len, ShinTables *T, ShinResult *res)
{
    ShinBits b{0, 0, 0, in_len};
    uint32_t produced = 0, n_stored = 0, n_fixed = 0, n_dynamic = 0, status = SHIN_OK;
#define SHIN_FAIL(code) do { status = (code); goto done; } while (0)
#define SHIN_NEED(k) do { if (b.n < (k)) SHIN_FAIL(SHIN_IN_OVERRUN); } while (0)
    for (;;) {
        shin_refill(&b, src);
        SHIN_NEED(3);
        const uint32_t bfinal = shin_peek(&b, 1), btype = shin_peek(&b, 3) >> 1;
        shin_drop(&b, 3);
        if (btype == 3) SHIN_FAIL(SHIN_BAD_BTYPE);
        if (btype == 0) {
            ++n_stored;
            shin_drop(&b, b.n & 7);
            shin_refill(&b, src);
            SHIN_NEED(32);
            const uint32_t len = shin_peek(&b, 16), nlen = (uint32_t)(b.acc >> 16) & 0xffffu;
            shin_drop(&b, 32);
            if ((len ^ 0xffffu) != nlen) SHIN_FAIL(SHIN_STORED_LEN);
            b.pos -= b.n >> 3;      // whole bytes are held: hand them back, the data is copied from the source
            b.acc = 0; b.n = 0;
            if (len > in_len - b.pos) SHIN_FAIL(SHIN_IN_OVERRUN);
            if (len > out_len - produced) SHIN_FAIL(SHIN_OUT_OVERRUN);
            if (len) sink.raw(b.pos, len);
            b.pos += len; produced += len;
        } else {
            uint32_t n_lit = SHIN_N_LIT, n_dist = SHIN_N_DIST, st;
            if (btype == 1) {
                ++n_fixed;
                shin_fixed_lengths(T);
            } else {
                ++n_dynamic;
                if ((st = shin_dynamic_lengths(&b, src, T, &n_lit, &n_dist)) != SHIN_OK) SHIN_FAIL(st);
            }
            if ((st = shin_block_tables(T, n_lit, n_dist)) != SHIN_OK) SHIN_FAIL(st);
            if ((st = shin_block_tokens(&b, src, sink, T, &produced, out_len, 0, 0)) != SHIN_OK) SHIN_FAIL(st);
        }
        if (bfinal) break;
    }
    if (produced != out_len) status = SHIN_OUT_SHORT;
done:
#undef SHIN_FAIL
#undef SHIN_NEED
    res->status = status; res->produced = produced; res->n_stored = n_stored; res->n_fixed = n_fixed; res->n_dynamic = n_dynamic;
}

// ---- CRC-32 (the polynomial of RFC 1952) in pieces -----------------------------------------------------------------------------------------
// crc(A || B) = shin_crc_shift(crc(A), |B|) ^ crc(B): the shift multiplies by x^(8 |B|) modulo the polynomial, as zlib's crc32_combine
// does.  So the CRC of a buffer cut into pieces is the XOR of every piece's CRC shifted by the bytes that follow the piece.
#define SHIN_CRC_POLY 0xedb88320u

SHIN_FN uint32_t shin_crc_table_entry(uint32_t i)
{
    uint32_t c = i;
    for (int k = 0; k < 8; ++k) c = c & 1 ? (c >> 1) ^ SHIN_CRC_POLY : c >> 1;
    return c;
}
SHIN_FN uint32_t shin_crc_piece(const uint32_t *table, const uint8_t *p, uint32_t n)
{
    uint32_t c = 0xffffffffu;
    for (uint32_t i = 0; i < n; ++i) c = table[(c ^ p[i]) & 0xff] ^ (c >> 8);
    return ~c;
}
SHIN_FN uint32_t shin_gf2_mul(uint32_t a, uint32_t b)      // a(x) * b(x) modulo the polynomial, bit 31 = x^0
{
    uint32_t p = 0;
    for (uint32_t i = 0; i < 32; ++i) {
        if (a & (0x80000000u >> i)) p ^= b;
        b = b & 1 ? (b >> 1) ^ SHIN_CRC_POLY : b >> 1;
    }
    return p;
}
SHIN_FN uint32_t shin_crc_shift(uint32_t crc, uint32_t n_bytes)
{
    uint32_t sq = 0x40000000u;      // x^1
    for (int k = 0; k < 3; ++k) sq = shin_gf2_mul(sq, sq);      // x^8
    uint32_t p = 0x80000000u;       // x^0
    for (; n_bytes; n_bytes >>= 1) {
        if (n_bytes & 1) p = shin_gf2_mul(sq, p);
        sq = shin_gf2_mul(sq, sq);
    }
    return shin_gf2_mul(p, crc);
}

// ---- a general gzip stream in spans (sh_gunzip.h) ---------------------------------------------------------------------------
// A gzip file that is one long member is cut into chunks of compressed bytes at fixed offsets.  A chunk's span starts at a DEFLATE block
// start inside the chunk and runs to the first block boundary at or past the chunk's end; it is decoded without the 32 KiB of output
// before it: a reference into them becomes a marker, which the window step and the resolve step replace (the scheme of pugz / rapidgzip).
#define SHIN_MAX_ENDS 4u                    // members that may end inside one span
#define SHIN_WINDOW 32768u
#define SHIN_MARKER 0x8000u                 // a symbol below 256 is the byte; SHIN_MARKER | k is byte k of the window before the span
#define SHIN_SPAN_MAX_OUT (1u << 30)        // what the size pass lets one span hold
#define SHIN_NO_START (~0ull)

struct ShinMemberEnd { uint32_t out_off, crc32, isize, end_byte; };      // the member's last byte is span byte out_off - 1; end_byte: the input byte behind its trailer
struct ShinSpan { uint32_t status, produced, n_ends, pad; uint64_t end_bit; ShinMemberEnd ends[SHIN_MAX_ENDS]; };

// A gzip member header at input byte pos: SHIN_OK and *data_pos (the first DEFLATE byte); SHIN_SPAN_END when what is there is no gzip
// member (zlib's gzread ends the stream there: fewer than two bytes at the end of the input, or another magic); SHIN_IN_OVERRUN when the
// header leaves the input; SHIN_BAD_HEADER.  FEXTRA, FNAME, FCOMMENT are skipped and FHCRC is checked.
template <class Src>
SHIN_FN uint32_t shin_gzip_header(Src &src, uint32_t pos, uint32_t in_len, bool in_is_end, uint32_t *data_pos)
{
    const uint32_t avail = in_len - pos;
    if (avail < 2) return in_is_end ? SHIN_SPAN_END : SHIN_IN_OVERRUN;
    if (src.byte(pos) != 0x1f || src.byte(pos + 1) != 0x8b) return SHIN_SPAN_END;
    if (avail < 10) return SHIN_IN_OVERRUN;
    const uint32_t flg = src.byte(pos + 3);
    if (src.byte(pos + 2) != 8 || (flg & 0xe0)) return SHIN_BAD_HEADER;
    uint32_t q = pos + 10;
    if (flg & 4) {
        if (in_len - q < 2) return SHIN_IN_OVERRUN;
        const uint32_t xlen = src.byte(q) | src.byte(q + 1) << 8;
        q += 2;
        if (in_len - q < xlen) return SHIN_IN_OVERRUN;
        q += xlen;
    }
    for (uint32_t bit = 8; bit <= 16; bit <<= 1)
        if (flg & bit)
            for (;;) {
                if (q >= in_len) return SHIN_IN_OVERRUN;
                if (src.byte(q++) == 0) break;
            }
    if (flg & 2) {
        if (in_len - q < 2) return SHIN_IN_OVERRUN;
        uint32_t c = 0xffffffffu;
        for (uint32_t i = pos; i < q; ++i) c = shin_crc_table_entry((c ^ src.byte(i)) & 0xff) ^ (c >> 8);
        if (((~c) & 0xffffu) != (src.byte(q) | src.byte(q + 1) << 8)) return SHIN_BAD_HEADER;
        q += 2;
    }
    *data_pos = q;
    return SHIN_OK;
}

// the reader at a bit position of the input
template <class Src>
SHIN_FN bool shin_seek_bit(ShinBits *b, Src &src, uint64_t bit)
{
    b->acc = 0; b->n = 0; b->pos = (uint32_t)(bit >> 3);
    if (b->pos > b->in_len) return false;
    shin_refill(b, src);
    if (b->n < (uint32_t)(bit & 7)) return false;
    shin_drop(b, (uint32_t)(bit & 7));
    return true;
}
SHIN_FN uint64_t shin_bit_pos(const ShinBits *b) { return 8ull * b->pos - b->n; }

// What 128 bits of input (lo: the first 64) that begin at a bit position with bit index `bit_in_byte` say about a block start there,
// with `avail` of them inside the input: 0 none, 2 a stored block (BFINAL 0, padding zero, LEN == ~NLEN), 1 a dynamic block whose
// HLIT and HDIST are in range and whose code-length code is complete.  Plain arithmetic on the lane's own values, so the lanes of a
// wave test 64 positions at once; shin_block_candidate decides the dynamic ones.
SHIN_FN uint32_t shin_candidate_quick(uint64_t lo, uint64_t hi, uint64_t avail, uint32_t bit_in_byte)
{
    if (avail < 3 || (lo & 1)) return 0;
    const uint32_t btype = (uint32_t)(lo >> 1) & 3;
    if (btype == 0) {
        const uint32_t pad = (8 - ((bit_in_byte + 3) & 7)) & 7, at = 3 + pad;
        if (avail < at + 32 || ((lo >> 3) & ((1u << pad) - 1))) return 0;
        const uint32_t w = (uint32_t)(lo >> at);      // at <= 10
        return ((w ^ (w >> 16)) & 0xffffu) == 0xffffu ? 2 : 0;
    }
    if (btype != 2) return 0;
    const uint32_t hlit = (uint32_t)(lo >> 3) & 31, hdist = (uint32_t)(lo >> 8) & 31, n_cl = ((uint32_t)(lo >> 13) & 15) + 4;
    if (hlit > 29 || hdist > 29 || avail < 17 + 3 * n_cl) return 0;
    uint32_t kraft = 0;
    for (uint32_t i = 0; i < n_cl; ++i) {
        const uint32_t at = 17 + 3 * i;
        const uint32_t l = (uint32_t)(at < 64 ? (lo >> at) | (at > 61 ? hi << (64 - at) : 0) : hi >> (at - 64)) & 7;
        if (l) kraft += 128u >> l;
    }
    return kraft == 128 ? 1 : 0;
}

// Is bit position `bit` a block start a span may begin at?  A dynamic block with BFINAL 0 whose header passes every check the decoder
// makes before its first token (the very functions it makes them with), or a stored block with BFINAL 0, zero padding and LEN == ~NLEN
// (the empty block a flush leaves among them).  A fixed block has nothing to check and is never one.
template <class Src>
SHIN_FN bool shin_block_candidate(Src &src, uint32_t in_len, uint64_t bit, ShinTables *T)
{
    ShinBits b{0, 0, 0, in_len};
    if (!shin_seek_bit(&b, src, bit) || b.n < 3) return false;
    const uint32_t hdr = shin_peek(&b, 3);
    shin_drop(&b, 3);
    if (hdr & 1) return false;
    if ((hdr >> 1) == 0) {
        const uint32_t pad = b.n & 7;
        if (shin_peek(&b, pad)) return false;
        shin_drop(&b, pad);
        shin_refill(&b, src);
        if (b.n < 32) return false;
        return (shin_peek(&b, 16) ^ 0xffffu) == ((uint32_t)(b.acc >> 16) & 0xffffu);
    }
    if ((hdr >> 1) != 2) return false;
    uint32_t n_lit, n_dist;
    if (shin_dynamic_lengths(&b, src, T, &n_lit, &n_dist) != SHIN_OK) return false;
    return shin_block_tables(T, n_lit, n_dist) == SHIN_OK;
}

// One span: from start_bit (a block start, or with at_header the first byte of a member header) block after block to the first block
// boundary at or past stop_bit (SHIN_OK), or to the end of the stream (SHIN_SPAN_END).  Behind a final block the trailer is recorded in
// res->ends and the next member's header parsed.  out_cap bounds what the sink is given.  Until a member has started inside the span a
// distance may reach SHIN_WINDOW bytes before the span; behind a member start it may not reach before that start.
template <class Src, class Sink>
SHIN_FN void shin_inflate_span(Src &src, uint32_t in_len, bool in_is_end, uint64_t start_bit, bool at_header, uint64_t stop_bit, Sink &sink, uint32_t out_cap,
                               ShinTables *T, ShinSpan *res, ShinMemberEnd *ends)
{
    ShinBits b{0, 0, 0, in_len};
    uint32_t produced = 0, base = 0, back = at_header ? 0 : SHIN_WINDOW, n_ends = 0, status = SHIN_OK, st;
    uint64_t end_bit = start_bit;
#define SHIN_FAIL(code) do { status = (code); goto done; } while (0)
#define SHIN_NEED(k) do { if (b.n < (k)) SHIN_FAIL(SHIN_IN_OVERRUN); } while (0)
    if (at_header) {
        uint32_t data_pos = 0;
        if ((start_bit >> 3) > in_len) SHIN_FAIL(SHIN_IN_OVERRUN);
        if ((st = shin_gzip_header(src, (uint32_t)(start_bit >> 3), in_len, in_is_end, &data_pos)) != SHIN_OK) SHIN_FAIL(st);
        b.pos = data_pos;
    } else if (!shin_seek_bit(&b, src, start_bit)) SHIN_FAIL(SHIN_IN_OVERRUN);
    for (;;) {
        shin_refill(&b, src);
        end_bit = shin_bit_pos(&b);
        if (end_bit >= stop_bit) break;
        SHIN_NEED(3);
        const uint32_t bfinal = shin_peek(&b, 1), btype = shin_peek(&b, 3) >> 1;
        shin_drop(&b, 3);
        if (btype == 3) SHIN_FAIL(SHIN_BAD_BTYPE);
        if (btype == 0) {
            shin_drop(&b, b.n & 7);
            shin_refill(&b, src);
            SHIN_NEED(32);
            const uint32_t len = shin_peek(&b, 16), nlen = (uint32_t)(b.acc >> 16) & 0xffffu;
            shin_drop(&b, 32);
            if ((len ^ 0xffffu) != nlen) SHIN_FAIL(SHIN_STORED_LEN);
            b.pos -= b.n >> 3;
            b.acc = 0; b.n = 0;
            if (len > in_len - b.pos) SHIN_FAIL(SHIN_IN_OVERRUN);
            if (len > out_cap - produced) SHIN_FAIL(SHIN_OUT_OVERRUN);
            if (len) sink.raw(b.pos, len);
            b.pos += len; produced += len;
        } else {
            uint32_t n_lit = SHIN_N_LIT, n_dist = SHIN_N_DIST;
            if (btype == 1) shin_fixed_lengths(T);
            else if ((st = shin_dynamic_lengths(&b, src, T, &n_lit, &n_dist)) != SHIN_OK) SHIN_FAIL(st);
            if ((st = shin_block_tables(T, n_lit, n_dist)) != SHIN_OK) SHIN_FAIL(st);
            if ((st = shin_block_tokens(&b, src, sink, T, &produced, out_cap, base, back)) != SHIN_OK) SHIN_FAIL(st);
        }
        if (bfinal) {
            shin_drop(&b, b.n & 7);
            b.pos -= b.n >> 3;
            b.acc = 0; b.n = 0;
            if (in_len - b.pos < 8) SHIN_FAIL(SHIN_IN_OVERRUN);
            if (n_ends == SHIN_MAX_ENDS) SHIN_FAIL(SHIN_MANY_ENDS);
            uint32_t crc = 0, isize = 0, data_pos = 0;
            for (uint32_t i = 0; i < 4; ++i) { crc |= src.byte(b.pos + i) << (8 * i); isize |= src.byte(b.pos + 4 + i) << (8 * i); }
            b.pos += 8;
            ends[n_ends++] = ShinMemberEnd{produced, crc, isize, b.pos};
            base = produced; back = 0;
            end_bit = 8ull * b.pos;
            if ((st = shin_gzip_header(src, b.pos, in_len, in_is_end, &data_pos)) != SHIN_OK) SHIN_FAIL(st);      // SHIN_SPAN_END among them: the stream is over
            b.pos = data_pos;
        }
    }
done:
#undef SHIN_FAIL
#undef SHIN_NEED
    res->status = status; res->produced = produced; res->n_ends = n_ends; res->pad = 0; res->end_bit = end_bit;
}

// the sink of the size pass: the decoder counts, nothing is stored
struct ShinSizeSink {
    SHIN_FN void lit(uint32_t) {}
    SHIN_FN void match(uint32_t, uint32_t) {}
    SHIN_FN void raw(uint32_t, uint32_t) {}
};

// what a match at distance `dist` gives span byte `pos` when the source lies before the span (pos < dist)
SHIN_FN uint32_t shin_marker(uint32_t pos, uint32_t dist) { return SHIN_MARKER | (SHIN_WINDOW - (dist - pos)); }

// a symbol as a byte: `win` is the 32 KiB before the symbol's span, of which the last `valid` bytes belong to the open member
SHIN_FN uint32_t shin_resolve(uint32_t sym, const uint8_t *win, uint32_t valid, uint32_t *bad)
{
    if (sym < 256) return sym;
    const uint32_t k = sym & (SHIN_WINDOW - 1);
    if (k < SHIN_WINDOW - valid) { *bad = SHIN_DIST_FAR; return 0; }
    return win[k];
}

// the window step: byte i of the 32 KiB that end with the span's last byte.  A span shorter than that keeps the tail of `prev` in front.
SHIN_FN uint32_t shin_window_byte(uint32_t i, const uint8_t *prev, uint32_t valid, const uint16_t *sym, uint32_t produced, uint32_t *bad)
{
    if (produced >= SHIN_WINDOW) return shin_resolve(sym[produced - SHIN_WINDOW + i], prev, valid, bad);
    if (i + produced >= SHIN_WINDOW) return shin_resolve(sym[i + produced - SHIN_WINDOW], prev, valid, bad);
    return prev[i + produced];
}
