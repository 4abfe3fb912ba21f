// sh_k2_mask.hip - low-complexity masking of a library batch in HBM before the database build (DESIGN.md §7 "Low-complexity masking").
// Symmetric DUST in integers: inside a run of ACGT, an interval of triplets [i, j] (at most W - 2 of them) has the score r / l with
// r = sum over codes of c (c - 1) / 2 and l = j - i; it is perfect when 10 r > T l and no interval inside it scores strictly higher;
// the bases [i, j + 2] of every perfect interval are masked.
//
// Pass 1 (k_k2_mask_scan): a wave walks a tile of a record base by base with ONE LANE PER START.  At the step of end triplet j lane k
// holds the interval [j - 1 - k, j], so the per-lane state moves up one lane per step (wave_shr1):
//   trip  the triplet at the lane's start;  the new triplet's count inside the lane's interval is then the number of lanes <= k whose
//         trip equals it - one ballot and a popcount under a mask, no counter arrays at all
//   r     the interval's numerator (r += that count)
//   M     the largest score of any interval inside the lane's interval, as a fraction (Mr / Ml): M(i, j) = max(M(i, j - 1),
//         max over starts a >= i of S(a, j)); the inner maximum is an inclusive prefix maximum over the lanes (DPP scan, fractions
//         compared by cross-multiplication: r <= 1891, l <= 61)
// A lane is perfect when 10 r > T l and S >= M.  Perfect starts of one end are nested, so the step's whole answer is the highest
// perfect lane: one byte per base, the number of bases the masked stretch that ENDS at this base reaches back (0 = none).
// Steps on which no lane exceeds T skip the scan: what they leave out of M is <= T / 10 and can never beat a later candidate.
// A tile warms up over the W bases before it (the oldest start its first end can use lies W - 1 bases back) without emitting.
// Pass 2 (k_k2_mask_apply): base q is masked iff some p >= q has p - reach[p] < q (reach <= W bounds the look-ahead, and a stretch
// never leaves its run, so record borders need no test); 8 bases per thread, rewritten in place.
#include "sh_common.h"
#include <rocprim/rocprim.hpp>
#include <algorithm>
#include <cstdlib>
#include "sh_wave.h"
#include "sh_k2_mask.h"

#define K2M_TILE 4096u         // bases per work item: measured choice
#define K2M_GRID (256 * 32)    // one-wave blocks, grid-stride over the work items

struct K2MaskArgs {
    const uint8_t *bases; const uint64_t *offsets; uint64_t n_records;
    uint64_t *tile_off;        // n_records + 1: exclusive prefix sum of the records' tile counts
    uint8_t *reach;            // one byte per base of the batch, indexed like bases - offsets[0]
    uint32_t tile; int32_t window, threshold;
};

__global__ void k_k2_mask_tilecount(K2MaskArgs a)
{
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r <= a.n_records; r += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t n = 0;
        if (r < a.n_records) { const uint64_t len = a.offsets[r + 1] - a.offsets[r]; n = (len + a.tile - 1) / a.tile; }
        a.tile_off[r] = n;
    }
}

struct K2MaskWave {
    int32_t trip, r, Mr, Ml;                // per lane
    int32_t runlen, tri, nvalid;            // the same on every lane
    __device__ void reset() { trip = 0; r = 0; Mr = 0; Ml = 1; runlen = 0; tri = 0; nvalid = 0; }
    // one base (code 0..3, 4 = not a nucleotide); returns the reach-back of the masked stretch that ends at it
    __device__ int32_t step(uint32_t code, int32_t lane, uint64_t le_mask, int32_t W, int32_t T)
    {
        if (code > 3u) { runlen = 0; nvalid = 0; return 0; }
        const int32_t prev = tri;
        tri = (int32_t)(((uint32_t)tri << 2 | code) & 63u);
        runlen = runlen < 4 ? runlen + 1 : 4;
        if (runlen < 4) return 0;                               // the run's first triplet ends no interval
        trip = wave_shr1(trip, prev);
        r = wave_shr1(r, 0); Mr = wave_shr1(Mr, 0); Ml = wave_shr1(Ml, 1);
        nvalid = nvalid + 1 < W - 3 ? nvalid + 1 : W - 3;
        const bool valid = lane < nvalid;
        const uint64_t same = __ballot(valid && trip == tri);
        r = valid ? r + __popcll(same & le_mask) : 0;
        const int32_t l = lane + 1;
        const bool cand = valid && 10 * r > T * l;
        if (__ballot(cand) == 0) return 0;
        int32_t Pr = r, Pl = valid ? l : 1;                     // inclusive prefix maximum of the scores, lanes in start order
#define K2M_SCAN_STEP(CTRL, ROWS)                                                              \
        { const int32_t tr = dpp_mov<CTRL, ROWS>(0, Pr), tl = dpp_mov<CTRL, ROWS>(1, Pl);      \
          const bool gt = tr * Pl > Pr * tl; Pr = gt ? tr : Pr; Pl = gt ? tl : Pl; }
        K2M_SCAN_STEP(0x111, 0xf) K2M_SCAN_STEP(0x112, 0xf) K2M_SCAN_STEP(0x114, 0xf) K2M_SCAN_STEP(0x118, 0xf)
        K2M_SCAN_STEP(0x142, 0xa) K2M_SCAN_STEP(0x143, 0xc)
#undef K2M_SCAN_STEP
        if (Pr * Ml > Mr * Pl) { Mr = Pr; Ml = Pl; }
        const uint64_t perfect = __ballot(cand && r * Ml >= Mr * l);
        return perfect ? (63 - __clzll((long long)perfect)) + 4 : 0;      // lane k: start j - 1 - k, end base j + 2 -> k + 4 bases
    }
};

__global__ __launch_bounds__(64) void k_k2_mask_scan(K2MaskArgs a)
{
    const int32_t lane = (int32_t)threadIdx.x;
    const uint64_t le_mask = lane == 63 ? ~0ull : (2ull << lane) - 1;
    const uint64_t n_items = a.tile_off[a.n_records];
    const uint64_t base0 = a.offsets[0];
    for (uint64_t item = blockIdx.x; item < n_items; item += gridDim.x) {
        uint64_t lo = 0, hi = a.n_records;       // the last record r with tile_off[r] <= item (empty records are passed over)
        while (hi - lo > 1) { const uint64_t mid = (lo + hi) >> 1; if (a.tile_off[mid] <= item) lo = mid; else hi = mid; }
        const uint64_t r0 = a.offsets[lo], len = a.offsets[lo + 1] - r0;
        const uint64_t e0 = (item - a.tile_off[lo]) * a.tile, e1 = e0 + a.tile < len ? e0 + a.tile : len;
        const uint64_t from = e0 >= (uint64_t)a.window ? e0 - (uint64_t)a.window : 0;
        // absolute byte positions in the batch: walk [g_from, g_end), emit from g_emit on
        const uint64_t g_from = r0 + from, g_emit = r0 + e0, g_end = r0 + e1;
        const uintptr_t p_from = (uintptr_t)(a.bases + g_from), p_end = (uintptr_t)(a.bases + g_end);
        const uintptr_t w_from = p_from & ~(uintptr_t)7;
        const int64_t g_w0 = (int64_t)g_from - (int64_t)(p_from - w_from);      // batch position of the first aligned word's byte 0
        const uint64_t n_words = (p_end - w_from + 7) / 8;                       // only the aligned words that overlap the walk are loaded
        K2MaskWave S; S.reset();
        int32_t mine = 0;                        // lane x keeps the answer of emitted position g_emit + 64 q + x until the flush
        for (uint64_t wb = 0; wb < n_words; wb += 64) {
            const uint64_t wi = wb + (uint64_t)lane;
            const unsigned long long w_lane = wi < n_words ? *(const unsigned long long *)(w_from + wi * 8) : 0ull;
            const int32_t n_here = (int32_t)(n_words - wb < 64 ? n_words - wb : 64);
#pragma nounroll
            for (int32_t wl = 0; wl < n_here; ++wl) {
                unsigned long long w = wave_readlane_u64(w_lane, wl);
                const int64_t g_word = g_w0 + (int64_t)(wb + (uint64_t)wl) * 8;
#pragma unroll
                for (int32_t b = 0; b < 8; ++b, w >>= 8) {
                    const int64_t g = g_word + b;
                    if (g < (int64_t)g_from || g >= (int64_t)g_end) continue;
                    const int32_t reach = S.step(sh_nt4((uint32_t)w & 0xffu), lane, le_mask, a.window, a.threshold);
                    if (g < (int64_t)g_emit) continue;
                    const uint64_t e = (uint64_t)g - g_emit;
                    if ((int32_t)(e & 63) == lane) mine = reach;
                    if ((e & 63) == 63 || (uint64_t)g + 1 == g_end) {
                        const uint64_t first = (uint64_t)g - (e & 63);
                        if ((uint64_t)lane <= (e & 63)) a.reach[first - base0 + (uint64_t)lane] = (uint8_t)mine;
                    }
                }
            }
        }
    }
}

struct K2MaskApply {
    uint8_t *bases; const uint8_t *reach;      // reach: n + 64 + 8 bytes, zero behind n
    uint64_t n;                                // bases of the batch (offsets[n_records] - offsets[0]); bases points at offsets[0]
    int32_t window, replacement;
    uint64_t quiet_head, quiet_tail;           // masked bases in [0, quiet_head) and [n - quiet_tail, n) are not counted
    unsigned long long *n_masked;
};

__global__ __launch_bounds__(256) void k_k2_mask_apply(K2MaskApply a)
{
    unsigned long long count = 0;
    const uint64_t n_groups = (a.n + 7) / 8;
    for (uint64_t gi = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; gi < n_groups; gi += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t q0 = gi * 8;
        // smallest start of any stretch that ends at or behind p, walking p down from q0 + 71: reach <= W <= 64, so nothing
        // further out can start at or before q0 + 7.  Nine aligned words of reach bytes (readable and zero up to n + 72).
        int32_t min_start = INT32_MAX;                          // relative to q0
        uint32_t masked = 0;
        const unsigned long long *rw = (const unsigned long long *)a.reach + gi;
#pragma unroll
        for (int32_t wi = 8; wi >= 0; --wi) {
            const unsigned long long w = rw[wi];
            if (wi > 0 && w == 0) continue;
#pragma unroll
            for (int32_t b = 7; b >= 0; --b) {
                const int32_t d = wi * 8 + b, rb = (int32_t)(w >> (8 * b)) & 0xff;
                if (rb) { const int32_t s = d - rb + 1; min_start = s < min_start ? s : min_start; }
                if (wi == 0 && min_start <= d) masked |= 1u << d;
            }
        }
        for (int32_t d = 0; d < 8; ++d) {
            const uint64_t p = q0 + (uint64_t)d;
            if (p >= a.n) break;
            if (!((masked >> d) & 1u)) continue;
            count += p >= a.quiet_head && p < a.n - a.quiet_tail;
            a.bases[p] = a.replacement ? (uint8_t)a.replacement : (uint8_t)(a.bases[p] | 0x20u);
        }
    }
    // one atomic per wave
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) count += (unsigned long long)__shfl_xor((long long)count, o);
    if ((threadIdx.x & 63) == 0 && count) atomicAdd(a.n_masked, count);
}

static uint32_t k2_mask_tile()
{   // the tile length is a measured choice (scripts/k2_mask_speed.py sweeps it through this switch; the tests use it to put tile
    // borders everywhere)
    const char *e = getenv("SCRUBBY_HIP_K2_MASK_TILE");
    const long v = e && *e ? atol(e) : 0;
    return v >= 64 && v <= (1 << 24) ? (uint32_t)v : K2M_TILE;
}

sh_status shi_k2_mask_params(int32_t *window, int32_t *threshold, int32_t replacement, const char *who)
{
    if (*window == 0) *window = 64;
    if (*threshold == 0) *threshold = 20;
    SH_CHECK(*window >= 8 && *window <= 64, SH_ERR_BAD_ARG, "%s: mask window %d outside [8, 64]", who, *window);
    SH_CHECK(*threshold >= 1 && *threshold <= 10000, SH_ERR_BAD_ARG, "%s: mask threshold %d outside [1, 10000]", who, *threshold);
    SH_CHECK(replacement >= 0 && replacement <= 255, SH_ERR_BAD_ARG, "%s: mask replacement %d is not a byte", who, replacement);
    return SH_OK;
}

sh_status shi_k2_mask_device(uint8_t *d_bases, const uint64_t *d_offsets, uint64_t n_records, int32_t window, int32_t threshold, int32_t replacement,
                             uint64_t quiet_head, uint64_t quiet_tail, hipStream_t s, sh_k2_mask_stats *stats)
{
    SH_CHECK(d_offsets && (d_bases || n_records == 0), SH_ERR_BAD_ARG, "sh_k2_mask_device: null argument");
    sh_status st = shi_k2_mask_params(&window, &threshold, replacement, "sh_k2_mask_device");
    if (st != SH_OK) return st;
    if (stats) memset(stats, 0, sizeof(*stats));
    if (n_records == 0) return SH_OK;
    uint64_t ends[2];
    SH_HIP(hipMemcpyAsync(&ends[0], d_offsets, 8, hipMemcpyDeviceToHost, s));
    SH_HIP(hipMemcpyAsync(&ends[1], d_offsets + n_records, 8, hipMemcpyDeviceToHost, s));
    SH_HIP(hipStreamSynchronize(s));
    SH_CHECK(ends[1] >= ends[0], SH_ERR_BAD_ARG, "sh_k2_mask_device: offsets decrease");
    const uint64_t n = ends[1] - ends[0];
    SH_CHECK(quiet_head <= n && quiet_tail <= n, SH_ERR_BAD_ARG, "sh_k2_mask_device: margins longer than the batch");
    if (n == 0) return SH_OK;
    DevBuf b_tile, b_tmp, b_reach, b_ctr;
    DevEvent e0, e1;
    SH_HIP(b_tile.alloc((n_records + 1) * 8));
    SH_HIP(b_reach.alloc(n + 64 + 8));
    SH_HIP(b_ctr.alloc(8));
    SH_HIP(e0.create()); SH_HIP(e1.create());
    uint64_t *d_tile = b_tile.as<uint64_t>(); uint8_t *d_reach = b_reach.as<uint8_t>(); unsigned long long *d_ctr = b_ctr.as<unsigned long long>();
    SH_HIP(hipMemsetAsync(d_ctr, 0, 8, s));
    SH_HIP(hipMemsetAsync(d_reach + n, 0, 64 + 8, s));
    SH_HIP(hipEventRecord(e0.e, s));
    K2MaskArgs a{d_bases, d_offsets, n_records, d_tile, d_reach, k2_mask_tile(), window, threshold};
    hipLaunchKernelGGL(k_k2_mask_tilecount, dim3((uint32_t)std::min<uint64_t>((n_records + 256) / 256, 4096)), dim3(256), 0, s, a);
    size_t tmp_bytes = 0;
    SH_HIP(rocprim::exclusive_scan(nullptr, tmp_bytes, d_tile, d_tile, (uint64_t)0, n_records + 1, rocprim::plus<uint64_t>(), s));
    SH_HIP(b_tmp.alloc(std::max<size_t>(tmp_bytes, 1)));
    SH_HIP(rocprim::exclusive_scan(b_tmp.p, tmp_bytes, d_tile, d_tile, (uint64_t)0, n_records + 1, rocprim::plus<uint64_t>(), s));
    hipLaunchKernelGGL(k_k2_mask_scan, dim3(K2M_GRID), dim3(64), 0, s, a);
    K2MaskApply ap{d_bases + ends[0], d_reach, n, window, replacement, quiet_head, quiet_tail, d_ctr};
    hipLaunchKernelGGL(k_k2_mask_apply, dim3((uint32_t)std::min<uint64_t>(((n + 7) / 8 + 255) / 256, 1u << 16)), dim3(256), 0, s, ap);
    SH_HIP(hipEventRecord(e1.e, s));
    unsigned long long masked = 0, items = 0;
    SH_HIP(hipMemcpyAsync(&masked, d_ctr, 8, hipMemcpyDeviceToHost, s));
    SH_HIP(hipMemcpyAsync(&items, d_tile + n_records, 8, hipMemcpyDeviceToHost, s));
    SH_HIP(hipStreamSynchronize(s));
    SH_HIP(hipGetLastError());
    if (stats) { stats->n_bases = n; stats->n_masked = masked; stats->n_items = items; hipEventElapsedTime(&stats->ms, e0.e, e1.e); }
    return SH_OK;
}

extern "C" sh_status sh_k2_mask_device(uint8_t *d_bases, const uint64_t *d_offsets, uint64_t n_records, int32_t window, int32_t threshold, int32_t replacement,
                                       void *stream, sh_k2_mask_stats *stats)
{
    return shi_k2_mask_device(d_bases, d_offsets, n_records, window, threshold, replacement, 0, 0, (hipStream_t)stream, stats);
}
