// sh_deflate.h — the pure parts of the DEFLATE (RFC 1951) encoder, shared by the device kernels (sh_deflate.hip) and the host
// (tests/deflate_host.cpp): length-limited code lengths from a histogram, canonical codes, the dynamic-block header, and the bits of one
// token.  Nothing here touches the device; the LZ77 matcher lives in sh_deflate.hip.
//
// A token is one uint32_t: a literal (or the end-of-block symbol) is its literal/length symbol 0..256; a match is
// SHD_TOK_MATCH | (distance - 1) << 8 | (length - 3), length 3..258, distance 1..32768.
// Bits go out LSB-first; Huffman codes are stored already bit-reversed, so a code is appended like any other field.
#pragma once
#include <stdint.h>
#include <stddef.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SHD_FN __host__ __device__ inline
#else
#define SHD_FN inline
#endif

#define SHD_N_LIT 286
#define SHD_N_DIST 30
#define SHD_N_CL 19
#define SHD_EOB 256u
#define SHD_TOK_MATCH 0x80000000u
#define SHD_MIN_MATCH 3u
#define SHD_MAX_MATCH 258u
#define SHD_MAX_DIST 32768u
#define SHD_HDR_MAX_BYTES 512      // a dynamic header is at most 17 + 19 * 3 + 316 * 7 bits = 287 bytes

// scratch of shd_code_lengths for alphabets of up to SHD_N_LIT symbols (a workgroup keeps one in LDS)
struct ShdHuffWork {
    uint32_t weight[2 * SHD_N_LIT];      // leaves in sorted order, then the internal nodes in the order they are made
    uint16_t parent[2 * SHD_N_LIT];
    uint16_t order[SHD_N_LIT];           // used symbols by (frequency, symbol) ascending
    uint8_t depth[2 * SHD_N_LIT];
};

// LSB-first bit writer over a byte buffer of `cap` bytes; bits past the capacity are dropped and `overflow` is set
struct ShdBitWriter {
    uint8_t *p;
    size_t cap, pos;
    uint64_t acc;
    uint32_t n_acc;
    uint64_t n_bits;
    bool overflow;
};

SHD_FN void shd_bw_init(ShdBitWriter *w, uint8_t *p, size_t cap)
{
    w->p = p; w->cap = cap; w->pos = 0; w->acc = 0; w->n_acc = 0; w->n_bits = 0; w->overflow = false;
}

// n <= 48
SHD_FN void shd_bw_put(ShdBitWriter *w, uint64_t bits, uint32_t n)
{
    w->acc |= bits << w->n_acc;
    w->n_acc += n; w->n_bits += n;
    while (w->n_acc >= 8) {
        if (w->pos < w->cap) w->p[w->pos++] = (uint8_t)w->acc; else w->overflow = true;
        w->acc >>= 8; w->n_acc -= 8;
    }
}

// pads the last byte with zero bits
SHD_FN void shd_bw_flush(ShdBitWriter *w)
{
    if (w->n_acc) {
        if (w->pos < w->cap) w->p[w->pos++] = (uint8_t)w->acc; else w->overflow = true;
        w->n_bits += 8 - w->n_acc;
        w->acc = 0; w->n_acc = 0;
    }
}

SHD_FN uint32_t shd_ilog2(uint32_t v)      // v >= 1
{
    uint32_t r = 0;
    while (v >>= 1) ++r;
    return r;
}

// length 3..258 -> symbol 257..285, its extra bits and their value
SHD_FN uint32_t shd_len_sym(uint32_t len, uint32_t *n_extra, uint32_t *extra)
{
    const uint32_t l = len - 3;
    if (len == 258) { *n_extra = 0; *extra = 0; return 285; }
    if (l < 8) { *n_extra = 0; *extra = 0; return 257 + l; }
    const uint32_t e = shd_ilog2(l) - 2;
    *n_extra = e; *extra = l & ((1u << e) - 1);
    return 261 + 4 * e + ((l >> e) & 3);
}

// distance 1..32768 -> symbol 0..29
SHD_FN uint32_t shd_dist_sym(uint32_t dist, uint32_t *n_extra, uint32_t *extra)
{
    const uint32_t d = dist - 1;
    if (d < 4) { *n_extra = 0; *extra = 0; return d; }
    const uint32_t e = shd_ilog2(d) - 1;
    *n_extra = e; *extra = d & ((1u << e) - 1);
    return 2 * e + 2 + ((d >> e) & 1);
}

SHD_FN uint32_t shd_lit_extra_bits(uint32_t sym) { return sym < 265 || sym == 285 ? 0 : (sym - 261) >> 2; }
SHD_FN uint32_t shd_dist_extra_bits(uint32_t sym) { return sym < 4 ? 0 : (sym - 2) >> 1; }

// Code lengths of at most `limit` bits for the n <= SHD_N_LIT symbols of a histogram (0 for an unused symbol).  Huffman's tree by the
// two-queue merge over the symbols sorted by (frequency, symbol); depths past the limit are pulled in the way zlib's gen_bitlen does it
// (each step moves one leaf a level down and lifts an overflowing one), and the lengths are dealt again from the rarest symbol up, so the
// Kraft sum stays exactly 1.  No used symbol: every length 0.  One used symbol: that symbol gets length 1 - the incomplete code RFC 1951
// allows for distances; with `complete` a second symbol (0, or 1 if 0 is the used one) gets length 1 too, which is what the
// literal/length and code-length alphabets need.  Returns the number of symbols with a length.
SHD_FN uint32_t shd_code_lengths(const uint32_t *freq, uint32_t n, uint32_t limit, bool complete, uint8_t *lens, ShdHuffWork *w)
{
    uint32_t m = 0;
    for (uint32_t s = 0; s < n; ++s) {
        lens[s] = 0;
        if (!freq[s]) continue;
        uint32_t i = m++;      // insertion by (freq, symbol): symbols arrive in ascending order, so ties keep it
        while (i > 0 && freq[w->order[i - 1]] > freq[s]) { w->order[i] = w->order[i - 1]; --i; }
        w->order[i] = (uint16_t)s;
    }
    if (m == 0) return 0;
    if (m == 1) {
        lens[w->order[0]] = 1;
        if (!complete) return 1;
        lens[w->order[0] == 0 ? 1 : 0] = 1;
        return 2;
    }
    for (uint32_t i = 0; i < m; ++i) w->weight[i] = freq[w->order[i]];
    uint32_t leaf = 0, node = m, made = m;      // queue heads: leaves [leaf, m), internal nodes [node, made)
    while (made < 2 * m - 1) {
        uint32_t pick[2];
        for (int k = 0; k < 2; ++k) {
            const bool take_leaf = leaf < m && (node >= made || w->weight[leaf] <= w->weight[node]);
            pick[k] = take_leaf ? leaf++ : node++;
        }
        w->weight[made] = w->weight[pick[0]] + w->weight[pick[1]];
        w->parent[pick[0]] = (uint16_t)made; w->parent[pick[1]] = (uint16_t)made;
        ++made;
    }
    uint32_t count[32];
    for (uint32_t b = 0; b < 32; ++b) count[b] = 0;
    w->depth[made - 1] = 0;
    uint32_t overflow = 0;      // as in gen_bitlen: every node past the limit counts, internal ones too, and a clamped node clamps its subtree
    for (uint32_t i = made - 1; i-- > 0;) {      // a parent is made after its children, and the leaves come first
        uint32_t d = w->depth[w->parent[i]] + 1u;
        if (d > limit) { d = limit; ++overflow; }
        w->depth[i] = (uint8_t)d;
        if (i < m) ++count[d];
    }
    while ((int32_t)overflow > 0) {
        uint32_t b = limit - 1;
        while (count[b] == 0) --b;
        --count[b]; count[b + 1] += 2; --count[limit];
        overflow -= 2;
    }
    uint32_t i = 0;      // the rarest symbols take the longest codes
    for (uint32_t b = limit; b >= 1; --b)
        for (uint32_t c = count[b]; c > 0; --c) lens[w->order[i++]] = (uint8_t)b;
    return m;
}

SHD_FN uint32_t shd_bit_reverse(uint32_t v, uint32_t n)
{
    uint32_t r = 0;
    for (uint32_t i = 0; i < n; ++i) { r = r << 1 | (v & 1); v >>= 1; }
    return r;
}

// canonical codes (RFC 1951 3.2.2) of lens[0..n), bit-reversed for an LSB-first writer; max length 15
SHD_FN void shd_canonical_codes(const uint8_t *lens, uint32_t n, uint16_t *codes)
{
    uint32_t count[16], next[16];
    for (uint32_t b = 0; b < 16; ++b) count[b] = 0;
    for (uint32_t s = 0; s < n; ++s) ++count[lens[s]];
    count[0] = 0;
    uint32_t code = 0;
    for (uint32_t b = 1; b < 16; ++b) { code = (code + count[b - 1]) << 1; next[b] = code; }
    for (uint32_t s = 0; s < n; ++s) codes[s] = lens[s] ? (uint16_t)shd_bit_reverse(next[lens[s]]++, lens[s]) : 0;
}

// the code-length symbols (0..15 literal lengths, 16 / 17 / 18 runs) of lit_lens[0..hlit) followed by dist_lens[0..hdist), as one
// sequence: counted into cl_freq (w == nullptr) or written with cl_codes / cl_lens
SHD_FN void shd_rle_lengths(const uint8_t *lit_lens, uint32_t hlit, const uint8_t *dist_lens, uint32_t hdist, uint32_t *cl_freq, const uint16_t *cl_codes,
                            const uint8_t *cl_lens, ShdBitWriter *w)
{
    const uint32_t total = hlit + hdist;
    uint32_t i = 0;
    while (i < total) {
        const uint32_t v = i < hlit ? lit_lens[i] : dist_lens[i - hlit];
        uint32_t run = 1;
        while (i + run < total && (i + run < hlit ? lit_lens[i + run] : dist_lens[i + run - hlit]) == v) ++run;
        i += run;
        bool have_prev = false;      // code 16 repeats the length sent just before it
        while (run > 0) {
            uint32_t sym, n_extra = 0, extra = 0, used;
            if (v == 0 && run >= 11) { used = run < 138 ? run : 138; sym = 18; n_extra = 7; extra = used - 11; }
            else if (v == 0 && run >= 3) { used = run; sym = 17; n_extra = 3; extra = used - 3; }
            else if (v != 0 && have_prev && run >= 3) { used = run < 6 ? run : 6; sym = 16; n_extra = 2; extra = used - 3; }
            else { used = 1; sym = v; have_prev = true; }
            if (w) shd_bw_put(w, (uint64_t)cl_codes[sym] | (uint64_t)extra << cl_lens[sym], cl_lens[sym] + n_extra); else ++cl_freq[sym];
            run -= used;
        }
    }
}

// Header of one dynamic block: BFINAL, BTYPE 10, HLIT / HDIST / HCLEN, the code-length code and the run-length coded lengths.
// Returns the number of bits written (the writer is not flushed: the tokens follow in the same byte).
SHD_FN uint64_t shd_write_dynamic_header(ShdBitWriter *w, bool bfinal, const uint8_t *lit_lens, const uint8_t *dist_lens, ShdHuffWork *work)
{
    const uint64_t bits0 = w->n_bits;
    uint32_t hlit = SHD_N_LIT, hdist = SHD_N_DIST;
    while (hlit > 257 && lit_lens[hlit - 1] == 0) --hlit;
    while (hdist > 1 && dist_lens[hdist - 1] == 0) --hdist;
    uint32_t cl_freq[SHD_N_CL];
    uint8_t cl_lens[SHD_N_CL];
    uint16_t cl_codes[SHD_N_CL];
    for (uint32_t s = 0; s < SHD_N_CL; ++s) cl_freq[s] = 0;
    shd_rle_lengths(lit_lens, hlit, dist_lens, hdist, cl_freq, nullptr, nullptr, nullptr);
    shd_code_lengths(cl_freq, SHD_N_CL, 7, true, cl_lens, work);
    shd_canonical_codes(cl_lens, SHD_N_CL, cl_codes);
    const uint8_t perm[SHD_N_CL] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    uint32_t hclen = SHD_N_CL;
    while (hclen > 4 && cl_lens[perm[hclen - 1]] == 0) --hclen;
    shd_bw_put(w, (bfinal ? 1u : 0u) | 2u << 1, 3);
    shd_bw_put(w, hlit - 257, 5);
    shd_bw_put(w, hdist - 1, 5);
    shd_bw_put(w, hclen - 4, 4);
    for (uint32_t i = 0; i < hclen; ++i) shd_bw_put(w, cl_lens[perm[i]], 3);
    shd_rle_lengths(lit_lens, hlit, dist_lens, hdist, nullptr, cl_codes, cl_lens, w);
    return w->n_bits - bits0;
}

// the bits of one token, at most 48: the literal/length code, the length's extra bits, the distance code, its extra bits
SHD_FN uint64_t shd_token_bits(uint32_t tok, const uint16_t *lit_codes, const uint8_t *lit_lens, const uint16_t *dist_codes, const uint8_t *dist_lens, uint32_t *n_bits)
{
    if (!(tok & SHD_TOK_MATCH)) { *n_bits = lit_lens[tok]; return lit_codes[tok]; }
    uint32_t le, lx, de, dx;
    const uint32_t ls = shd_len_sym((tok & 0xffu) + 3, &le, &lx), ds = shd_dist_sym(((tok >> 8) & 0x7fffu) + 1, &de, &dx);
    uint64_t bits = lit_codes[ls];
    uint32_t n = lit_lens[ls];
    bits |= (uint64_t)lx << n; n += le;
    bits |= (uint64_t)dist_codes[ds] << n; n += dist_lens[ds];
    bits |= (uint64_t)dx << n; n += de;
    *n_bits = n;
    return bits;
}

// histograms of a token list (the end-of-block token is counted if it is in the list)
SHD_FN void shd_count_tokens(const uint32_t *tok, size_t n_tok, uint32_t *lit_freq, uint32_t *dist_freq)
{
    for (size_t i = 0; i < n_tok; ++i) {
        if (!(tok[i] & SHD_TOK_MATCH)) { ++lit_freq[tok[i]]; continue; }
        uint32_t e, x;
        ++lit_freq[shd_len_sym((tok[i] & 0xffu) + 3, &e, &x)];
        ++dist_freq[shd_dist_sym(((tok[i] >> 8) & 0x7fffu) + 1, &e, &x)];
    }
}

// the token writer over a given list: every token's bits appended in order
SHD_FN void shd_write_tokens(ShdBitWriter *w, const uint32_t *tok, size_t n_tok, const uint16_t *lit_codes, const uint8_t *lit_lens, const uint16_t *dist_codes,
                             const uint8_t *dist_lens)
{
    for (size_t i = 0; i < n_tok; ++i) {
        uint32_t n;
        const uint64_t bits = shd_token_bits(tok[i], lit_codes, lit_lens, dist_codes, dist_lens, &n);
        shd_bw_put(w, bits, n);
    }
}

// bits of the tokens of a block from its histograms: code lengths plus extra bits
SHD_FN uint64_t shd_body_bits(const uint32_t *lit_freq, const uint32_t *dist_freq, const uint8_t *lit_lens, const uint8_t *dist_lens)
{
    uint64_t bits = 0;
    for (uint32_t s = 0; s < SHD_N_LIT; ++s) bits += (uint64_t)lit_freq[s] * (lit_lens[s] + shd_lit_extra_bits(s));
    for (uint32_t s = 0; s < SHD_N_DIST; ++s) bits += (uint64_t)dist_freq[s] * (dist_lens[s] + shd_dist_extra_bits(s));
    return bits;
}

// output bound: a stored block costs 5 bytes more than its data, and no block is written larger than that
SHD_FN uint64_t shd_bound(uint64_t n, uint32_t block_bytes)
{
    const uint64_t nb = n ? (n + block_bytes - 1) / block_bytes : 1;
    return n + 5 * nb;
}
