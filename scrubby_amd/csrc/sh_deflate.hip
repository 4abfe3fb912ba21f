// sh_deflate.hip — DEFLATE (RFC 1951) on the device: the encoder behind .gz outputs.
//
// The input is cut into blocks of block_bytes; one wave compresses one block on its own and writes it as ONE deflate block that starts
// and ends on a byte boundary, into the block's slot; a second pair of kernels prefix-sums the slot sizes and copies the slots together.
//
//   k_deflate_block   per strip of 64 positions: every lane hashes the 4 bytes at its position and takes ONE candidate: the nearest
//                     earlier lane of the strip with the same hash, else what the table (LDS, u16, position + 1) holds for it from the
//                     strips before, and measures the match.  The lanes are grouped by hash with ballots; the highest lane of a
//                     group writes the table, so the winner of a slot does not depend on the order of LDS writes.  The
//                     greedy parse (a match of >= 4 is taken, else a literal) walks the strip once with the wave's lengths; the chosen
//                     lanes append their tokens to the block's token list in HBM and count their symbols in LDS.
//                     Lane 0 then builds both length-limited codes and the dynamic header (sh_deflate.h, the code the host tests
//                     check); the block's size is known from the histograms, and it is stored instead when that is no larger.
//                     Tokens are packed 64 at a time: bits and length per lane, a prefix sum for the offsets, OR into a staging strip
//                     in LDS, whole words out with vector stores.  A block that is not the last is followed by an empty stored
//                     block, which brings the stream back to a byte boundary.
//   k_deflate_scan    exclusive prefix sum of the slot sizes, the totals.
//   k_deflate_compact slot -> its place in the stream, a byte copy.
#include "sh_common.h"
#include "sh_deflate.h"
#include "sh_wave.h"
#include <zlib.h>
#include <chrono>

namespace {

constexpr uint32_t DF_HASH_BITS = 12;      // 8 KiB of u16: a 32-KiB block of FASTQ loses 0.1 % against 13 bits
constexpr uint32_t DF_MIN_MATCH = 4;       // the hash covers 4 bytes
constexpr uint32_t DF_STAGE_WORDS = 104;   // 31 carried bits + 64 tokens of at most 48 bits = 97 words, and a lane may touch two past its first

struct DfBlockStat { uint32_t size, stored, n_matches, n_literals; };
struct DfTotals { uint64_t n_blocks, n_stored, n_matches, n_literals, out_bytes; };

__device__ inline uint32_t df_hash(uint32_t v) { return (v * 2654435761u) >> (32 - DF_HASH_BITS); }

__global__ __launch_bounds__(64) void k_deflate_block(const uint8_t *__restrict__ in, uint64_t n, uint32_t block_bytes, int32_t flags, uint32_t *__restrict__ tokens,
                                                      uint64_t tok_stride, uint8_t *__restrict__ slots, uint64_t slot_stride, DfBlockStat *__restrict__ bst)
{
    __shared__ uint16_t s_head[1u << DF_HASH_BITS];
    __shared__ uint32_t s_freq[SHD_N_LIT + SHD_N_DIST];
    __shared__ uint8_t s_lens[SHD_N_LIT + SHD_N_DIST];
    __shared__ uint16_t s_codes[SHD_N_LIT + SHD_N_DIST];
    __shared__ ShdHuffWork s_work;
    __shared__ uint32_t s_hdr[SHD_HDR_MAX_BYTES / 4];
    __shared__ uint32_t s_stage[DF_STAGE_WORDS];
    __shared__ uint32_t s_bits[2];      // header bits, body bits

    const uint32_t lane = threadIdx.x;
    const uint64_t blk = blockIdx.x, beg = blk * block_bytes;
    const uint32_t nb = (uint32_t)(n - beg < block_bytes ? n - beg : block_bytes);
    const bool bfinal = beg + nb == n;
    const uint8_t *b = in + beg;
    uint32_t *tok = tokens + blk * tok_stride;
    uint8_t *slot = slots + blk * slot_stride;
    uint32_t *slot32 = (uint32_t *)slot;      // slot_stride is a multiple of 8

    for (uint32_t i = lane; i < (1u << DF_HASH_BITS); i += 64) s_head[i] = 0;
    for (uint32_t i = lane; i < SHD_N_LIT + SHD_N_DIST; i += 64) s_freq[i] = 0;
    for (uint32_t i = lane; i < SHD_HDR_MAX_BYTES / 4; i += 64) s_hdr[i] = 0;
    __syncthreads();

    // ---- LZ77: tokens and histograms ----
    const bool matching = !(flags & SH_DEFLATE_LITERALS_ONLY);
    uint32_t next_free = 0, n_tok = 0, n_match = 0;
    for (uint32_t base = 0; base < nb; base += 64) {
        const uint32_t p = base + lane;
        const bool hashed = matching && p + 4 <= nb;
        uint32_t h = 0, mlen = 0, mdist = 0, c1 = 0;
        if (hashed) {
            h = df_hash((uint32_t)b[p] | (uint32_t)b[p + 1] << 8 | (uint32_t)b[p + 2] << 16 | (uint32_t)b[p + 3] << 24);
            c1 = s_head[h];
        }
        __syncthreads();      // every lane has read the table before any lane writes it
        // the strip by hash, one group per turn (wave-uniform): a lane's candidate is the nearest lane below it in its group, and the
        // group's highest lane leaves its position in the table
        for (uint64_t todo = __ballot(hashed); todo;) {
            const uint32_t hv = (uint32_t)wave_bcast((int32_t)h, __ffsll((unsigned long long)todo) - 1);
            const bool in_group = hashed && h == hv;
            const uint64_t group = __ballot(in_group);
            if (in_group) {
                const uint64_t below = group & ((1ull << lane) - 1);
                if (below) c1 = base + (63 - __clzll((long long)below)) + 1;
                if (!(group >> lane >> 1)) s_head[h] = (uint16_t)(p + 1);
            }
            todo &= ~group;
        }
        if (c1 && p - (c1 - 1) <= SHD_MAX_DIST) {
            const uint32_t c = c1 - 1, max_len = nb - p < SHD_MAX_MATCH ? nb - p : SHD_MAX_MATCH;
            uint32_t l = 0;
            while (l < max_len && b[c + l] == b[p + l]) ++l;
            if (l >= DF_MIN_MATCH) { mlen = l; mdist = p - c; }
        }
        __syncthreads();
        // greedy parse of the strip: wave-uniform
        const uint32_t end = base + 64 < nb ? base + 64 : nb;
        uint32_t cur = next_free > base ? next_free : base;
        uint64_t sel = 0;
        while (cur < end) {
            const uint32_t l = (uint32_t)wave_bcast((int32_t)mlen, (int)(cur - base));
            sel |= 1ull << (cur - base);
            cur += l ? l : 1;
        }
        next_free = cur;
        const bool mine = (sel >> lane) & 1;
        if (mine) {
            uint32_t t;
            if (mlen) {
                uint32_t e, x;
                t = SHD_TOK_MATCH | (mdist - 1) << 8 | (mlen - 3);
                atomicAdd(&s_freq[shd_len_sym(mlen, &e, &x)], 1u);
                atomicAdd(&s_freq[SHD_N_LIT + shd_dist_sym(mdist, &e, &x)], 1u);
            } else {
                t = b[p];
                atomicAdd(&s_freq[t], 1u);
            }
            tok[n_tok + __popcll(sel & ((1ull << lane) - 1))] = t;
        }
        n_tok += __popcll(sel);
        n_match += __popcll(__ballot(mine && mlen));
    }
    if (lane == 0) { tok[n_tok] = SHD_EOB; s_freq[SHD_EOB] = 1; }
    const uint32_t n_lit = n_tok - n_match;
    ++n_tok;
    __syncthreads();

    // ---- codes and header: one lane, the shared code ----
    if (lane == 0) {
        shd_code_lengths(s_freq, SHD_N_LIT, 15, true, s_lens, &s_work);
        shd_code_lengths(s_freq + SHD_N_LIT, SHD_N_DIST, 15, false, s_lens + SHD_N_LIT, &s_work);
        shd_canonical_codes(s_lens, SHD_N_LIT, s_codes);
        shd_canonical_codes(s_lens + SHD_N_LIT, SHD_N_DIST, s_codes + SHD_N_LIT);
        ShdBitWriter bw;
        shd_bw_init(&bw, (uint8_t *)s_hdr, SHD_HDR_MAX_BYTES);
        s_bits[0] = (uint32_t)shd_write_dynamic_header(&bw, bfinal, s_lens, s_lens + SHD_N_LIT, &s_work);
        shd_bw_flush(&bw);
        s_bits[1] = (uint32_t)shd_body_bits(s_freq, s_freq + SHD_N_LIT, s_lens, s_lens + SHD_N_LIT);
    }
    __syncthreads();
    const uint32_t hdr_bits = s_bits[0], total_bits = hdr_bits + s_bits[1];
    // not the last block: an empty stored block (000, pad, 00 00 FF FF) brings the next block to a byte boundary
    const uint32_t coded = bfinal ? (total_bits + 7) / 8 : (total_bits + 3 + 7) / 8 + 4;
    const bool stored = nb + 5 <= coded;
    if (lane == 0) bst[blk] = DfBlockStat{stored ? nb + 5 : coded, stored ? 1u : 0u, n_match, n_lit};

    if (stored) {
        if (lane == 0) {
            slot[0] = bfinal ? 1 : 0;
            slot[1] = (uint8_t)nb; slot[2] = (uint8_t)(nb >> 8);
            slot[3] = (uint8_t)~nb; slot[4] = (uint8_t)(~nb >> 8);
        }
        for (uint32_t i = lane; i < nb; i += 64) slot[5 + i] = b[i];
        return;
    }

    // ---- pack: whole words of the header, then the tokens strip by strip ----
    uint32_t word = hdr_bits >> 5, carry_bits = hdr_bits & 31;      // words already final; bits held in the staging strip's first word
    for (uint32_t i = lane; i < word; i += 64) slot32[i] = s_hdr[i];
    uint32_t carry = s_hdr[word];
    for (uint32_t t0 = 0; t0 < n_tok; t0 += 64) {
        for (uint32_t i = lane; i < DF_STAGE_WORDS; i += 64) s_stage[i] = i == 0 ? carry : 0;
        __syncthreads();
        uint32_t nbits = 0;
        uint64_t bits = 0;
        if (t0 + lane < n_tok) bits = shd_token_bits(tok[t0 + lane], s_codes, s_lens, s_codes + SHD_N_LIT, s_lens + SHD_N_LIT, &nbits);
        const uint32_t incl = (uint32_t)wave_scan_add_incl((int32_t)nbits);
        const uint32_t strip_bits = (uint32_t)wave_bcast((int32_t)incl, 63);
        if (nbits) {
            const uint32_t off = carry_bits + incl - nbits, w = off >> 5, sh = off & 31;
            const uint64_t hi = sh ? bits >> (32 - sh) : bits >> 32;
            atomicOr(&s_stage[w], (uint32_t)(bits << sh));
            if ((uint32_t)hi) atomicOr(&s_stage[w + 1], (uint32_t)hi);
            if (hi >> 32) atomicOr(&s_stage[w + 2], (uint32_t)(hi >> 32));
        }
        __syncthreads();
        const uint32_t have = carry_bits + strip_bits, full = have >> 5;
        for (uint32_t i = lane; i < full; i += 64) slot32[word + i] = s_stage[i];
        carry = s_stage[full];
        word += full; carry_bits = have & 31;
        __syncthreads();
    }
    // ---- the tail: the bytes of the last partial word, and the empty stored block ----
    if (lane == 0) {
        const uint32_t body_end = bfinal ? coded : coded - 4;
        for (uint32_t k = word * 4; k < body_end; ++k) slot[k] = k - word * 4 < 4 ? (uint8_t)(carry >> (8 * (k - word * 4))) : 0;
        if (!bfinal) { slot[coded - 4] = 0; slot[coded - 3] = 0; slot[coded - 2] = 0xff; slot[coded - 1] = 0xff; }
    }
}

// one workgroup: offsets[i] = sum of the sizes before block i, offsets[n_blocks] = the stream's size; the totals
__global__ __launch_bounds__(256) void k_deflate_scan(const DfBlockStat *__restrict__ bst, uint32_t n_blocks, uint64_t *__restrict__ offsets, DfTotals *__restrict__ tot)
{
    __shared__ uint64_t s_sum[256];
    __shared__ unsigned long long s_tot[3];
    const uint32_t t = threadIdx.x, per = (n_blocks + 255) / 256, lo = t * per < n_blocks ? t * per : n_blocks, hi = lo + per < n_blocks ? lo + per : n_blocks;
    if (t < 3) s_tot[t] = 0;
    __syncthreads();
    uint64_t sum = 0, st = 0, nm = 0, nl = 0;
    for (uint32_t i = lo; i < hi; ++i) { sum += bst[i].size; st += bst[i].stored; nm += bst[i].n_matches; nl += bst[i].n_literals; }
    s_sum[t] = sum;
    atomicAdd(&s_tot[0], (unsigned long long)st); atomicAdd(&s_tot[1], (unsigned long long)nm); atomicAdd(&s_tot[2], (unsigned long long)nl);
    __syncthreads();
    if (t == 0) {
        uint64_t run = 0;
        for (uint32_t i = 0; i < 256; ++i) { const uint64_t v = s_sum[i]; s_sum[i] = run; run += v; }
        offsets[n_blocks] = run;
        *tot = DfTotals{n_blocks, s_tot[0], s_tot[1], s_tot[2], run};
    }
    __syncthreads();
    uint64_t run = s_sum[t];
    for (uint32_t i = lo; i < hi; ++i) { offsets[i] = run; run += bst[i].size; }
}

__global__ __launch_bounds__(256) void k_deflate_compact(const uint8_t *__restrict__ slots, uint64_t slot_stride, const DfBlockStat *__restrict__ bst,
                                                         const uint64_t *__restrict__ offsets, uint8_t *__restrict__ out)
{
    const uint8_t *src = slots + (uint64_t)blockIdx.x * slot_stride;
    uint8_t *dst = out + offsets[blockIdx.x];
    const uint32_t size = bst[blockIdx.x].size;
    for (uint32_t i = threadIdx.x; i < size; i += 256) dst[i] = src[i];
}

}      // namespace

struct sh_deflater {
    int32_t device = 0;
    uint64_t max_bytes = 0, max_blocks = 0, tok_stride = 0, slot_stride = 0;
    uint32_t block_bytes = 0;
    uint32_t *d_tokens = nullptr;
    uint8_t *d_slots = nullptr;
    DfBlockStat *d_bst = nullptr;
    uint64_t *d_offsets = nullptr;
    DfTotals *d_tot = nullptr, *h_tot = nullptr;      // pinned
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // sh_gzip_member's staging, allocated by its first call
    uint8_t *d_in = nullptr, *d_out = nullptr, *h_in = nullptr, *h_out = nullptr;      // h_*: pinned
    hipStream_t stream = nullptr;
    double ms_h2d = 0, ms_kernel = 0, ms_d2h = 0;      // of the last sh_gzip_member
};

extern "C" uint64_t sh_deflate_bound(uint64_t n, uint32_t block_bytes)
{
    if (block_bytes == 0) block_bytes = 32768;
    return shd_bound(n, block_bytes);
}

extern "C" sh_status sh_deflater_free(sh_deflater *df)
{
    if (!df) return SH_OK;
    hipSetDevice(df->device);
    if (df->d_tokens) hipFree(df->d_tokens);
    if (df->d_slots) hipFree(df->d_slots);
    if (df->d_bst) hipFree(df->d_bst);
    if (df->d_offsets) hipFree(df->d_offsets);
    if (df->d_tot) hipFree(df->d_tot);
    if (df->h_tot) hipHostFree(df->h_tot);
    if (df->d_in) hipFree(df->d_in);
    if (df->d_out) hipFree(df->d_out);
    if (df->h_in) hipHostFree(df->h_in);
    if (df->h_out) hipHostFree(df->h_out);
    if (df->ev0) hipEventDestroy(df->ev0);
    if (df->ev1) hipEventDestroy(df->ev1);
    if (df->stream) hipStreamDestroy(df->stream);
    delete df;
    return SH_OK;
}

extern "C" sh_status sh_deflater_create(int32_t device, uint64_t max_bytes, uint32_t block_bytes, sh_deflater **out)
{
    SH_CHECK(out, SH_ERR_BAD_ARG, "sh_deflater_create: null argument");
    *out = nullptr;
    if (block_bytes == 0) block_bytes = 32768;
    SH_CHECK(block_bytes >= 1024 && block_bytes <= 65535, SH_ERR_BAD_ARG, "sh_deflater_create: block_bytes %u outside 1024..65535", block_bytes);
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || n_dev <= device) { sh_set_error("no HIP device %d", device); return SH_ERR_NO_DEVICE; }
    SH_HIP(hipSetDevice(device));
    const uint64_t max_blocks = max_bytes ? (max_bytes + block_bytes - 1) / block_bytes : 1;
    SH_CHECK(max_blocks < (1ull << 31), SH_ERR_BAD_ARG, "sh_deflater_create: %llu blocks of %u bytes are more than one launch takes", (unsigned long long)max_blocks, block_bytes);
    sh_deflater *df = new sh_deflater;
    df->device = device; df->max_bytes = max_bytes; df->block_bytes = block_bytes; df->max_blocks = max_blocks;
    df->tok_stride = (uint64_t)block_bytes + 1;                  // one token per byte at most, and the end-of-block token
    df->slot_stride = ((uint64_t)block_bytes + 5 + 7) & ~7ull;   // the last word of a coded block is stored whole
    auto fail = [&](hipError_t e, const char *what, uint64_t bytes) {
        sh_set_error("sh_deflater_create: %s of %llu bytes -> %s", what, (unsigned long long)bytes, hipGetErrorString(e));
        sh_deflater_free(df);
        return e == hipErrorOutOfMemory ? SH_ERR_OOM : SH_ERR_HIP;
    };
    hipError_t e;
    uint64_t bytes = df->max_blocks * df->tok_stride * sizeof(uint32_t);
    if ((e = hipMalloc(&df->d_tokens, bytes)) != hipSuccess) return fail(e, "token scratch", bytes);
    bytes = df->max_blocks * df->slot_stride;
    if ((e = hipMalloc(&df->d_slots, bytes)) != hipSuccess) return fail(e, "block slots", bytes);
    bytes = df->max_blocks * sizeof(DfBlockStat);
    if ((e = hipMalloc(&df->d_bst, bytes)) != hipSuccess) return fail(e, "block sizes", bytes);
    bytes = (df->max_blocks + 1) * sizeof(uint64_t);
    if ((e = hipMalloc(&df->d_offsets, bytes)) != hipSuccess) return fail(e, "block offsets", bytes);
    if ((e = hipMalloc(&df->d_tot, sizeof(DfTotals))) != hipSuccess) return fail(e, "totals", sizeof(DfTotals));
    if ((e = hipHostMalloc(&df->h_tot, sizeof(DfTotals))) != hipSuccess) return fail(e, "pinned totals", sizeof(DfTotals));
    if ((e = hipEventCreate(&df->ev0)) != hipSuccess || (e = hipEventCreate(&df->ev1)) != hipSuccess) return fail(e, "events", 0);
    *out = df;
    return SH_OK;
}

extern "C" sh_status sh_deflate_device(sh_deflater *df, const uint8_t *d_in, uint64_t n, int32_t flags, uint8_t *d_out, uint64_t out_cap, uint64_t *out_len, void *stream,
                                       sh_deflate_stats *stats)
{
    SH_CHECK(df && d_out && out_len && (d_in || n == 0), SH_ERR_BAD_ARG, "sh_deflate_device: null argument");
    SH_CHECK(n <= df->max_bytes, SH_ERR_BAD_ARG, "sh_deflate_device: %llu bytes, the deflater was made for %llu", (unsigned long long)n, (unsigned long long)df->max_bytes);
    const uint64_t bound = shd_bound(n, df->block_bytes);
    SH_CHECK(out_cap >= bound, SH_ERR_BAD_ARG, "sh_deflate_device: room for %llu bytes, %llu bytes in blocks of %u may need %llu", (unsigned long long)out_cap,
             (unsigned long long)n, df->block_bytes, (unsigned long long)bound);
    SH_CHECK((flags & ~SH_DEFLATE_LITERALS_ONLY) == 0, SH_ERR_BAD_ARG, "sh_deflate_device: unknown flags 0x%x", flags);
    hipStream_t hs = (hipStream_t)stream;
    SH_HIP(hipSetDevice(df->device));
    *out_len = 0;
    if (stats) memset(stats, 0, sizeof *stats);
    if (n == 0) {      // the empty final block of the fixed code: BFINAL, BTYPE 01, end-of-block 0000000
        const uint8_t empty[2] = {0x03, 0x00};
        SH_HIP(hipMemcpyAsync(d_out, empty, 2, hipMemcpyHostToDevice, hs));
        SH_HIP(hipStreamSynchronize(hs));
        *out_len = 2;
        if (stats) stats->out_bytes = 2;
        return SH_OK;
    }
    const uint32_t n_blocks = (uint32_t)((n + df->block_bytes - 1) / df->block_bytes);
    SH_HIP(hipEventRecord(df->ev0, hs));
    k_deflate_block<<<n_blocks, 64, 0, hs>>>(d_in, n, df->block_bytes, flags, df->d_tokens, df->tok_stride, df->d_slots, df->slot_stride, df->d_bst);
    k_deflate_scan<<<1, 256, 0, hs>>>(df->d_bst, n_blocks, df->d_offsets, df->d_tot);
    k_deflate_compact<<<n_blocks, 256, 0, hs>>>(df->d_slots, df->slot_stride, df->d_bst, df->d_offsets, d_out);
    SH_HIP(hipGetLastError());
    SH_HIP(hipEventRecord(df->ev1, hs));
    SH_HIP(hipMemcpyAsync(df->h_tot, df->d_tot, sizeof(DfTotals), hipMemcpyDeviceToHost, hs));
    SH_HIP(hipStreamSynchronize(hs));
    float ms = 0;
    SH_HIP(hipEventElapsedTime(&ms, df->ev0, df->ev1));
    *out_len = df->h_tot->out_bytes;
    if (stats) {
        stats->n_blocks = df->h_tot->n_blocks; stats->n_stored = df->h_tot->n_stored; stats->n_matches = df->h_tot->n_matches;
        stats->n_literals = df->h_tot->n_literals; stats->out_bytes = df->h_tot->out_bytes; stats->ms = ms;
    }
    return SH_OK;
}

uint32_t shi_crc32(const uint8_t *in, uint64_t n)
{
    uint32_t crc = (uint32_t)crc32(0L, Z_NULL, 0);
    for (uint64_t done = 0; done < n;) { const uint64_t k = n - done < (1u << 30) ? n - done : (1u << 30); crc = (uint32_t)crc32(crc, in + done, (uInt)k); done += k; }
    return crc;
}

extern "C" sh_status sh_gzip_member(sh_deflater *df, const uint8_t *in, uint64_t n, int32_t flags, uint8_t *out, uint64_t out_cap, uint64_t *out_len, sh_deflate_stats *stats)
{
    SH_CHECK(df && out && out_len && (in || n == 0), SH_ERR_BAD_ARG, "sh_gzip_member: null argument");
    return shi_gzip_member_crc(df, in, n, flags, shi_crc32(in, n), out, out_cap, out_len, stats);
}

sh_status shi_gzip_member_crc(sh_deflater *df, const uint8_t *in, uint64_t n, int32_t flags, uint32_t crc, uint8_t *out, uint64_t out_cap, uint64_t *out_len,
                              sh_deflate_stats *stats)
{
    SH_CHECK(n <= df->max_bytes, SH_ERR_BAD_ARG, "sh_gzip_member: %llu bytes, the deflater was made for %llu", (unsigned long long)n, (unsigned long long)df->max_bytes);
    SH_CHECK(n < (1ull << 32), SH_ERR_BAD_ARG, "sh_gzip_member: %llu bytes do not fit a member's ISIZE check in one piece", (unsigned long long)n);
    const uint64_t bound = shd_bound(n, df->block_bytes);
    SH_CHECK(out_cap >= bound + 18, SH_ERR_BAD_ARG, "sh_gzip_member: room for %llu bytes, %llu bytes in blocks of %u may need %llu", (unsigned long long)out_cap,
             (unsigned long long)n, df->block_bytes, (unsigned long long)(bound + 18));
    SH_HIP(hipSetDevice(df->device));
    {      // the staging of the first call; what a failed call left unallocated is tried again by the next
        const uint64_t cap_in = df->max_bytes + 16, cap_out = shd_bound(df->max_bytes, df->block_bytes) + 16;
        if (!df->stream) SH_HIP(hipStreamCreateWithFlags(&df->stream, hipStreamNonBlocking));
        if (!df->d_in) SH_HIP(hipMalloc(&df->d_in, cap_in));
        if (!df->d_out) SH_HIP(hipMalloc(&df->d_out, cap_out));
        if (!df->h_in) SH_HIP(hipHostMalloc(&df->h_in, cap_in));
        if (!df->h_out) SH_HIP(hipHostMalloc(&df->h_out, cap_out));
    }
    const uint8_t head[10] = {0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 3};
    memcpy(out, head, 10);
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    const auto t0 = now();
    uint64_t zl = 0;
    if (n) {
        memcpy(df->h_in, in, n);
        SH_HIP(hipMemcpyAsync(df->d_in, df->h_in, n, hipMemcpyHostToDevice, df->stream));
        SH_HIP(hipStreamSynchronize(df->stream));
    }
    const auto t1 = now();
    sh_deflate_stats st;
    const sh_status rc = sh_deflate_device(df, df->d_in, n, flags, df->d_out, bound, &zl, df->stream, &st);
    if (rc != SH_OK) return rc;
    const auto t2 = now();
    SH_HIP(hipMemcpyAsync(df->h_out, df->d_out, zl, hipMemcpyDeviceToHost, df->stream));
    SH_HIP(hipStreamSynchronize(df->stream));
    memcpy(out + 10, df->h_out, zl);
    const auto t3 = now();
    const uint32_t isize = (uint32_t)n;
    uint8_t *tail = out + 10 + zl;
    for (int i = 0; i < 4; ++i) { tail[i] = (uint8_t)(crc >> (8 * i)); tail[4 + i] = (uint8_t)(isize >> (8 * i)); }
    df->ms_h2d = ms(t0, t1); df->ms_kernel = ms(t1, t2); df->ms_d2h = ms(t2, t3);
    *out_len = 10 + zl + 8;
    if (stats) *stats = st;
    return SH_OK;
}

// the stages of the last sh_gzip_member call, for pass 2's SCRUBBY_HIP_DBG_HOST line (sh_stream.cpp)
void shi_deflater_stage_ms(const sh_deflater *df, double ms3[3])
{
    ms3[0] = df->ms_h2d; ms3[1] = df->ms_kernel; ms3[2] = df->ms_d2h;
}
