// sh_k2_tx.hip - translated search, front end (DESIGN.md §7 "Translated search"): the six-frame translation of a read batch
// (k_k2_translate, sh_k2_translate_device / _host) and the residue-to-code pass of a protein library (k_k2_aa_encode).
// The rules are in sh_k2_tx.h; aa_translate.cc as recalled: PARITY UNPINNED.
//
// k_k2_translate: one lane per codon.  The codon that ends at base i of a record of n bases depends on three bases only, and
// both its places are closed-form: residue (i-2)/3 of forward frame i % 3, residue n_f-1-(i-2)/3 of reverse frame 3 + i % 3.  A
// record's six frames lie back to back from 2 * (offsets[r] - offsets[0]), so lengths and positions are arithmetic from the
// nucleotide offsets: no prefix sum, no offset array, no carried state.  A wave takes a span of K2_TX_SPAN consecutive bases of
// the batch, 64 at a time; the record of the span's first base is found by one binary search over the offsets (the same
// addresses on every lane; one search per 64 bases made the dependent loads of the search the kernel's whole time), the wave
// then walks the records as it walks the bases, and each lane steps on to its own record (a step or none for reads longer than
// 64 bases).  The bound is memory: per base three cached byte
// reads (and three quality bytes) and two byte writes, which interleave three residues apart within a frame.
#include "sh_common.h"
#include "sh_k2_db.h"
#include "sh_k2_tx.h"
#include <algorithm>

struct K2TxArgs {
    const uint8_t *bases, *quals;        // quals nullable
    const uint64_t *offsets; uint64_t n_records;
    uint64_t beg, n_bases;               // offsets[0], offsets[n_records] - offsets[0]
    int32_t min_qual, as_letters;
    uint8_t *out;                        // 2 * n_bases + 8 bytes
};

// the two output bytes of the codon (c0, c1, c2), base codes 0..3 or 4
__host__ __device__ static inline void k2_tx_codon(uint32_t c0, uint32_t c1, uint32_t c2, int32_t as_letters, uint8_t &fwd, uint8_t &rev)
{
    if ((c0 | c1 | c2) > 3u) { fwd = rev = as_letters ? (uint8_t)'X' : (uint8_t)K2_AA_AMBIG; return; }
    const uint32_t f = k2_tx_residue(16u * c0 + 4u * c1 + c2), r = k2_tx_residue(16u * (3u - c2) + 4u * (3u - c1) + (3u - c0));
    fwd = (uint8_t)(as_letters ? f : k2_aa_code(f)); rev = (uint8_t)(as_letters ? r : k2_aa_code(r));
}

// where the codon that ends at base i of a record of n bases goes, relative to the record's first output byte
__host__ __device__ static inline void k2_tx_place(uint64_t n, uint64_t i, uint64_t &at_fwd, uint64_t &at_rev)
{
    uint64_t n0, n1, n2;
    k2_tx_frame_lens(n, n0, n1, n2);
    const uint32_t f = (uint32_t)(i % 3);
    const uint64_t j = (i - 2) / 3, nf = f == 0 ? n0 : f == 1 ? n1 : n2, start = f == 0 ? 0 : f == 1 ? n0 : n0 + n1;
    at_fwd = start + j; at_rev = (n0 + n1 + n2) + start + (nf - 1 - j);
}

#define K2_TX_SPAN 4096u        // consecutive bases one wave translates per search over the offsets
__global__ __launch_bounds__(256) void k_k2_translate(K2TxArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    const uint64_t n_spans = (a.n_bases + K2_TX_SPAN - 1) / K2_TX_SPAN;
    for (uint64_t span = wave; span < n_spans; span += n_waves) {
        const uint64_t b_beg = span * K2_TX_SPAN, b_end = b_beg + K2_TX_SPAN < a.n_bases ? b_beg + K2_TX_SPAN : a.n_bases;
        // the last record with offsets[r] <= the span's first base (empty records before it are passed over): one search per
        // span, the same addresses on every lane; from there the wave walks the records as it walks the bases
        uint64_t lo = 0, hi = a.n_records;
        while (hi - lo > 1) { const uint64_t mid = (lo + hi) >> 1; if (a.offsets[mid] <= a.beg + b_beg) lo = mid; else hi = mid; }
        for (uint64_t b0 = b_beg; b0 < b_end; b0 += 64) {
            while (a.offsets[lo + 1] <= a.beg + b0) ++lo;        // (wave-uniform) offsets[n_records] > the base: ends at lo < n_records
            const uint64_t p = a.beg + b0 + lane;
            if (b0 + lane >= b_end) continue;
            uint64_t r = lo;
            while (a.offsets[r + 1] <= p) ++r;
            const uint64_t r0 = a.offsets[r], n = a.offsets[r + 1] - r0, i = p - r0;
            if (i < 2) continue;                         // no codon ends at a record's first two bases
            uint32_t c0 = k2_tx_nt(a.bases[p - 2]), c1 = k2_tx_nt(a.bases[p - 1]), c2 = k2_tx_nt(a.bases[p]);
            if (a.quals) {
                c0 = k2_masked(a.quals[p - 2], a.min_qual) ? 4u : c0;
                c1 = k2_masked(a.quals[p - 1], a.min_qual) ? 4u : c1;
                c2 = k2_masked(a.quals[p], a.min_qual) ? 4u : c2;
            }
            uint8_t fwd, rev; uint64_t at_fwd, at_rev;
            k2_tx_codon(c0, c1, c2, a.as_letters, fwd, rev);
            k2_tx_place(n, i, at_fwd, at_rev);
            uint8_t *o = a.out + 2 * (r0 - a.beg);       // at_rev < 2 * (n - 2): inside the record's 2 * n bytes
            o[at_fwd] = fwd; o[at_rev] = rev;
        }
    }
}

// the translation of a batch whose extent the caller knows; enqueued on s, no synchronisation
sh_status shi_k2_translate_device(const uint8_t *d_bases, const uint8_t *d_quals, const uint64_t *d_offsets, uint64_t n_records, uint64_t beg, uint64_t n_bases,
                                  int32_t min_qual, int32_t as_letters, uint8_t *d_out, hipStream_t s)
{
    if (n_records == 0 || n_bases == 0) return SH_OK;
    const K2TxArgs a{d_bases, min_qual > 0 ? d_quals : nullptr, d_offsets, n_records, beg, n_bases, min_qual, as_letters, d_out};
    hipLaunchKernelGGL(k_k2_translate, dim3((uint32_t)std::min<uint64_t>((n_bases + 4 * K2_TX_SPAN - 1) / (4 * K2_TX_SPAN), 8192)), dim3(256), 0, s, a);
    SH_HIP(hipGetLastError());
    return SH_OK;
}

extern "C" sh_status sh_k2_translate_device(const uint8_t *d_bases, const uint8_t *d_quals, const uint64_t *d_offsets, uint64_t n_records, int32_t min_qual,
                                            int32_t as_letters, uint8_t *d_out, void *stream)
{
    SH_CHECK(d_offsets && d_out && (d_bases || n_records == 0), SH_ERR_BAD_ARG, "sh_k2_translate_device: null argument");
    if (n_records == 0) return SH_OK;
    hipStream_t s = (hipStream_t)stream;
    uint64_t ends[2];
    SH_HIP(hipMemcpyAsync(&ends[0], d_offsets, 8, hipMemcpyDeviceToHost, s));
    SH_HIP(hipMemcpyAsync(&ends[1], d_offsets + n_records, 8, hipMemcpyDeviceToHost, s));
    SH_HIP(hipStreamSynchronize(s));
    SH_CHECK(ends[1] >= ends[0], SH_ERR_BAD_ARG, "sh_k2_translate_device: offsets decrease");
    return shi_k2_translate_device(d_bases, d_quals, d_offsets, n_records, ends[0], ends[1] - ends[0], min_qual, as_letters, d_out, s);
}

// the host mirror: the same two helpers, record by record
extern "C" sh_status sh_k2_translate_host(const uint8_t *bases, const uint8_t *quals, const uint64_t *offsets, uint64_t n_records, int32_t min_qual,
                                          int32_t as_letters, uint8_t *out)
{
    SH_CHECK(offsets && out && (bases || n_records == 0), SH_ERR_BAD_ARG, "sh_k2_translate_host: null argument");
    if (min_qual <= 0) quals = nullptr;
    for (uint64_t r = 0; r < n_records; ++r) {
        SH_CHECK(offsets[r + 1] >= offsets[r], SH_ERR_BAD_ARG, "sh_k2_translate_host: offsets decrease");
        const uint64_t r0 = offsets[r], n = offsets[r + 1] - r0;
        uint8_t *o = out + 2 * (r0 - offsets[0]);
        for (uint64_t i = 2; i < n; ++i) {
            uint32_t c[3];
            for (int t = 0; t < 3; ++t) {
                const uint64_t p = r0 + i - 2 + (uint64_t)t;
                c[t] = quals && k2_masked(quals[p], min_qual) ? 4u : k2_tx_nt(bases[p]);
            }
            uint8_t fwd, rev; uint64_t at_fwd, at_rev;
            k2_tx_codon(c[0], c[1], c[2], as_letters, fwd, rev);
            k2_tx_place(n, i, at_fwd, at_rev);
            o[at_fwd] = fwd; o[at_rev] = rev;
        }
    }
    return SH_OK;
}

// ---- a protein library's residues to scanner codes ------------------------------------------------------------------------
// src and dst lie at the same address modulo 8: eight bytes per lane over the aligned words inside [0, n), the bytes before the
// first and after the last such word one each
__global__ __launch_bounds__(256) void k_k2_aa_encode(const uint8_t *src, uint8_t *dst, uint64_t n)
{
    const uint64_t mis = (8 - ((uintptr_t)src & 7)) & 7, head = mis < n ? mis : n, n_words = (n - head) / 8, tail0 = head + n_words * 8;
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t *in = (const uint64_t *)(src + head);
    uint64_t *out = (uint64_t *)(dst + head);
    for (uint64_t i = t; i < n_words; i += stride) {
        const uint64_t v = in[i];
        uint64_t r = 0;
#pragma unroll
        for (int b = 0; b < 8; ++b) r |= (uint64_t)k2_aa_code((uint32_t)(v >> (8 * b)) & 0xffu) << (8 * b);
        out[i] = r;
    }
    if (t < head) dst[t] = (uint8_t)k2_aa_code(src[t]);
    if (t < n - tail0) dst[tail0 + t] = (uint8_t)k2_aa_code(src[tail0 + t]);
}

sh_status shi_k2_aa_encode_device(const uint8_t *d_residues, uint8_t *d_codes, uint64_t n, hipStream_t s)
{
    SH_CHECK((((uintptr_t)d_residues ^ (uintptr_t)d_codes) & 7) == 0, SH_ERR_BAD_ARG, "shi_k2_aa_encode_device: residues and codes must lie at the same address modulo 8");
    if (n == 0) return SH_OK;
    hipLaunchKernelGGL(k_k2_aa_encode, dim3((uint32_t)std::min<uint64_t>((n / 8 + 256) / 256, 8192)), dim3(256), 0, s, d_residues, d_codes, n);
    SH_HIP(hipGetLastError());
    return SH_OK;
}
