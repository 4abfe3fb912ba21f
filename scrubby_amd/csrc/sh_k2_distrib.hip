// sh_k2_distrib.hip - Kraken arm: Bracken's k-mer distribution on the GPU and its abundance estimate on the host
// (DESIGN.md §7 "Abundance re-estimation").  The method of Lu et al. 2017 as include/scrubby_hip.h states it; Bracken's sources
// were not at hand: PARITY WITH Bracken's OWN PROGRAMS UNPINNED, like the rest of the arm.
//
// bracken-build asks, for every library genome and every read-length window of it, what Kraken 2 would call that window.  Two
// kernels per batch:
//   codes    k_k2_codes_lib (sh_k2.hip, beside the scanner and the probe it needs): one uint32 per k-mer, the hit lists' code;
//   windows  k_k2_distrib_windows (here): a lane takes a stretch of S consecutive window starts of one record, builds the taxon
//            counts of its first window, then slides: one code leaves, one enters; when they are equal the call repeats and
//            nothing is resolved.  Runs of equal calls are tallied, so an atomic is paid per run, not per window: first into a
//            table of the block in LDS, from there (once, at the block's end) into the accumulator's table in HBM.
// The per-lane taxon table holds K2D_CAP entries in LDS.  A window with more distinct taxa stops the lane there: it tallies what
// it has and queues (stretch, window) for the second instance, whose table holds W entries per lane in HBM - a window of W k-mers
// cannot hold more distinct taxa, so that instance drops nothing by construction.
#include "sh_k2_distrib.h"
#include <rocprim/rocprim.hpp>
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <map>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#define K2D_STRETCH 128u        // window starts per work item: a measured choice (DESIGN.md §7 "Abundance re-estimation")
#define K2D_CAP 8               // distinct taxa per lane kept in LDS, as K2_HCAP
#define K2D_TSLOTS 256u         // (genome, call) slots of the block's tally table in LDS
#define K2D_TPROBE 8u           // ... probed before a tally goes to HBM directly
#define K2D_GRID 8192u          // one-wave blocks, 32 per CU, grid-stride over the work items (their number stays on the device)
#define K2D_BIG_GRID 128u       // ... of the second instance: K2D_BIG_GRID * 64 lanes own W entries each in HBM
#define K2D_EMPTY (~0ull)       // no key: genome 0xffffffff is no taxon
#define K2D_MAX_READ_LEN 1024
// ctr words
#define K2D_NBIG 0
#define K2D_FULL 1
#define K2D_NWIN 2
#define K2D_NEED 3
#define K2D_CTR_WORDS 4

struct K2DArgs {
    const uint64_t *offsets; const uint32_t *taxa; uint64_t n_records; uint32_t n_nodes;
    uint64_t *item_off;                         // n_records + 1: items per record, then their exclusive prefix sum
    const uint32_t *codes; uint64_t codes_cap;
    const uint32_t *parent;
    uint32_t L, W, S;
    unsigned long long *keys, *vals; uint32_t lg_slots;        // the accumulator: genome << 32 | call -> windows, open addressing
    unsigned long long *ctr;
    unsigned long long *big_list; uint64_t big_cap;            // item << 16 | first window not yet tallied
    uint32_t *big_tax, *big_cnt;                // W entries per lane of the second instance
};

__global__ void k_k2_distrib_items(K2DArgs a)
{
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r <= a.n_records; r += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t n = 0;
        if (r < a.n_records && a.taxa[r] && a.taxa[r] < a.n_nodes) {
            const uint64_t len = a.offsets[r + 1] - a.offsets[r];
            n = len >= a.L ? (len - a.L + 1 + a.S - 1) / a.S : 0;
        }
        a.item_off[r] = n;
    }
}

// taxon counts of one lane's window: entry j at [j * STRIDE]
template <int STRIDE>
struct K2DCounts {
    uint32_t *tax, *cnt; uint32_t n, cap; bool over;
    __device__ inline void add(uint32_t t)
    {
        uint32_t j = 0;
        while (j < n && tax[j * STRIDE] != t) ++j;
        if (j < n) { ++cnt[j * STRIDE]; return; }
        if (n == cap) { over = true; return; }
        tax[n * STRIDE] = t; cnt[n * STRIDE] = 1; ++n;
    }
    __device__ inline void sub(uint32_t t)
    {
        uint32_t j = 0;
        while (j < n && tax[j * STRIDE] != t) ++j;
        if (j == n) return;
        if (--cnt[j * STRIDE] == 0) { --n; tax[j * STRIDE] = tax[n * STRIDE]; cnt[j * STRIDE] = cnt[n * STRIDE]; }
    }
    // Kraken 2's ResolveTree at confidence 0: the taxon whose root-to-taxon path collects the most k-mers, ties to their LCA
    __device__ inline uint32_t resolve(const uint32_t *__restrict__ parent) const
    {
        if (n <= 1) return n ? tax[0] : 0u;
        uint32_t max_taxon = 0, max_score = 0;
        for (uint32_t i = 0; i < n; ++i) {
            const uint32_t ti = tax[i * STRIDE];
            uint32_t score = 0;
            for (uint32_t j = 0; j < n; ++j) if (k2_is_ancestor(parent, tax[j * STRIDE], ti)) score += cnt[j * STRIDE];
            if (score > max_score) { max_score = score; max_taxon = ti; }
            else if (score == max_score) max_taxon = k2_lca(parent, max_taxon, ti);
        }
        return max_taxon;
    }
};

__device__ static inline uint64_t k2d_mix(uint64_t key) { return key * 0x9E3779B97F4A7C15ULL; }

__device__ static inline void k2d_global_add(const K2DArgs &a, unsigned long long key, unsigned long long n)
{
    const uint64_t mask = (1ull << a.lg_slots) - 1;
    uint64_t h = k2d_mix(key) >> (64 - a.lg_slots);
    for (uint64_t step = 0; step <= mask; ++step) {
        const unsigned long long old = atomicCAS(&a.keys[h], K2D_EMPTY, key);
        if (old == K2D_EMPTY || old == key) { atomicAdd(&a.vals[h], n); return; }
        h = (h + 1) & mask;
    }
    atomicAdd(&a.ctr[K2D_FULL], 1ull);          // never a silent loss: the host turns this into SH_ERR_OOM
}

__device__ static inline void k2d_tally(const K2DArgs &a, unsigned long long *s_key, uint32_t *s_val, uint32_t genome, uint32_t call, uint32_t n)
{
    const unsigned long long key = (unsigned long long)genome << 32 | call;
    uint32_t h = (uint32_t)(k2d_mix(key) >> 40) & (K2D_TSLOTS - 1);
    for (uint32_t step = 0; step < K2D_TPROBE; ++step) {
        const unsigned long long old = atomicCAS(&s_key[h], K2D_EMPTY, key);
        if (old == K2D_EMPTY || old == key) { atomicAdd(&s_val[h], n); return; }
        h = (h + 1) & (K2D_TSLOTS - 1);
    }
    k2d_global_add(a, key, n);
}

__device__ static inline bool k2d_counted(uint32_t code) { return code != 0 && code != SH_K2_HIT_AMBIGUOUS; }

template <bool BIG>
__global__ __launch_bounds__(64) void k_k2_distrib_windows(K2DArgs a)
{
    __shared__ uint32_t s_tax[BIG ? 1 : 64 * K2D_CAP], s_cnt[BIG ? 1 : 64 * K2D_CAP];
    __shared__ unsigned long long s_key[K2D_TSLOTS];
    __shared__ uint32_t s_val[K2D_TSLOTS];
    const uint32_t lane = threadIdx.x;
    if (a.offsets[a.n_records] > a.codes_cap) return;          // the codes kernel wrote nothing: the host grows the scratch and repeats the batch
    for (uint32_t i = lane; i < K2D_TSLOTS; i += 64) { s_key[i] = K2D_EMPTY; s_val[i] = 0; }
    __syncthreads();
    constexpr int STRIDE = BIG ? 1 : 64;
    K2DCounts<STRIDE> H;
    if constexpr (BIG) {
        const uint64_t gl = (uint64_t)blockIdx.x * 64 + lane;
        H.tax = a.big_tax + gl * a.W; H.cnt = a.big_cnt + gl * a.W; H.cap = a.W;
    } else {
        H.tax = s_tax + lane; H.cnt = s_cnt + lane; H.cap = K2D_CAP;
    }
    unsigned long long n_win = 0;
    const uint64_t n_queued = a.ctr[K2D_NBIG] < a.big_cap ? a.ctr[K2D_NBIG] : a.big_cap;
    const uint64_t n_work = BIG ? n_queued : a.item_off[a.n_records];
    for (uint64_t base = (uint64_t)blockIdx.x * 64; base < n_work; base += (uint64_t)gridDim.x * 64) {
        const uint64_t idx = base + lane;
        if (idx >= n_work) continue;
        uint64_t item = idx; uint32_t p = 0;
        if constexpr (BIG) { const unsigned long long e = a.big_list[idx]; item = e >> 16; p = (uint32_t)(e & 0xffffu); }
        uint64_t lo = 0, hi = a.n_records;       // the last record r with item_off[r] <= item (records without items are passed over)
        while (hi - lo > 1) { const uint64_t mid = (lo + hi) >> 1; if (a.item_off[mid] <= item) lo = mid; else hi = mid; }
        const uint64_t r0 = a.offsets[lo], len = a.offsets[lo + 1] - r0;
        const uint64_t p0 = (item - a.item_off[lo]) * a.S, left = len - a.L + 1 - p0;
        const uint32_t nw = left < a.S ? (uint32_t)left : a.S;
        const uint32_t genome = a.taxa[lo];
        const uint32_t *c = a.codes + r0 + p0;  // k-mers of window q of the stretch: c[q .. q + W - 1], all inside the record
        if constexpr (!BIG) n_win += nw;
        H.n = 0; H.over = false;
        for (uint32_t i = 0; i < a.W; ++i) { const uint32_t code = c[p + i]; if (k2d_counted(code)) H.add(code); }
        if (H.over) {
            const unsigned long long at = atomicAdd(&a.ctr[K2D_NBIG], 1ull);
            if (at < a.big_cap) a.big_list[at] = (unsigned long long)item << 16 | p;
            continue;
        }
        uint32_t call = H.resolve(a.parent), run = 1;
        for (uint32_t q = p + 1; q < nw; ++q) {
            const uint32_t out = c[q - 1], in = c[q + a.W - 1];
            if (out != in) {
                const bool co = k2d_counted(out), ci = k2d_counted(in);
                if (co || ci) {
                    if (co) H.sub(out);
                    if (ci) H.add(in);
                    if (H.over) {                // exact from here on only with the larger table: the windows so far stand
                        k2d_tally(a, s_key, s_val, genome, call, run);
                        run = 0;
                        const unsigned long long at = atomicAdd(&a.ctr[K2D_NBIG], 1ull);
                        if (at < a.big_cap) a.big_list[at] = (unsigned long long)item << 16 | q;
                        break;
                    }
                    const uint32_t now = H.resolve(a.parent);
                    if (now != call) { k2d_tally(a, s_key, s_val, genome, call, run); call = now; run = 0; }
                }
            }
            ++run;
        }
        if (run) k2d_tally(a, s_key, s_val, genome, call, run);
    }
    __syncthreads();
    for (uint32_t i = lane; i < K2D_TSLOTS; i += 64)
        if (s_key[i] != K2D_EMPTY && s_val[i]) k2d_global_add(a, s_key[i], s_val[i]);
    if constexpr (!BIG) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) n_win += (unsigned long long)__shfl_xor((long long)n_win, o);
        if (lane == 0 && n_win) atomicAdd(&a.ctr[K2D_NWIN], n_win);
    }
}

// ---- the accumulator ----------------------------------------------------------------------------------------------------------
struct sh_k2_distrib {
    const sh_k2_db *db = nullptr;
    int device = 0;
    uint32_t read_len = 0, W = 0;
    unsigned long long *d_keys = nullptr, *d_vals = nullptr; uint32_t lg_slots = 0;
    uint32_t *d_codes = nullptr; uint64_t codes_cap = 0;
    unsigned long long *d_big = nullptr; uint64_t big_cap = 0;
    uint32_t *d_big_tax = nullptr, *d_big_cnt = nullptr;
    unsigned long long *d_ctr = nullptr;
    bool full = false;
    float ms_codes = 0, ms_windows = 0;
};

static uint32_t k2d_stretch()
{   // the stretch is a measured choice (scripts/k2_bracken_speed.py sweeps it through this switch)
    const char *e = getenv("SCRUBBY_HIP_K2_DISTRIB_STRETCH");
    const long v = e && *e ? atol(e) : 0;
    return v >= 16 && v <= 32768 ? (uint32_t)v : K2D_STRETCH;
}

extern "C" uint32_t sh_k2_distrib_stretch(void) { return k2d_stretch(); }

extern "C" sh_status sh_k2_distrib_free(sh_k2_distrib *d)
{
    if (!d) return SH_OK;
    hipSetDevice(d->device);
    hipFree(d->d_keys); hipFree(d->d_vals); hipFree(d->d_codes); hipFree(d->d_big); hipFree(d->d_big_tax); hipFree(d->d_big_cnt); hipFree(d->d_ctr);
    delete d;
    return SH_OK;
}

extern "C" sh_status sh_k2_distrib_reset(sh_k2_distrib *d)
{
    SH_CHECK(d, SH_ERR_BAD_ARG, "sh_k2_distrib_reset: null argument");
    SH_HIP(hipSetDevice(d->device));
    SH_HIP(hipMemset(d->d_keys, 0xff, 8ull << d->lg_slots));
    SH_HIP(hipMemset(d->d_vals, 0, 8ull << d->lg_slots));
    d->full = false;
    return SH_OK;
}

extern "C" sh_status sh_k2_distrib_create(const sh_k2_db *db, int32_t read_len, sh_k2_distrib **out)
{
    SH_CHECK(db && out, SH_ERR_BAD_ARG, "sh_k2_distrib_create: null argument");
    SH_CHECK(!db->opts.protein, SH_ERR_BAD_ARG, "sh_k2_distrib_create: Bracken's k-mer distribution is not supported on a protein database");
    SH_CHECK(read_len >= db->opts.k && read_len <= K2D_MAX_READ_LEN, SH_ERR_BAD_ARG, "sh_k2_distrib_create: read length %d outside [k = %d, %d]", read_len,
             db->opts.k, K2D_MAX_READ_LEN);
    SH_HIP(hipSetDevice(db->device));
    sh_k2_distrib *d = new sh_k2_distrib;
    d->db = db; d->device = db->device; d->read_len = (uint32_t)read_len; d->W = (uint32_t)(read_len - db->opts.k + 1);
    // a genome maps to its own lineage and to what it shares sequence with: 32 slots per taxon, 2^16 at least
    d->lg_slots = 16;
    while ((1ull << d->lg_slots) < 32ull * db->nodes.size() && d->lg_slots < 30) ++d->lg_slots;
    d->codes_cap = 1ull << 22;
    const uint64_t big_lanes = (uint64_t)K2D_BIG_GRID * 64;
    const uint64_t bytes = (16ull << d->lg_slots) + d->codes_cap * 4 + 2 * big_lanes * d->W * 4 + K2D_CTR_WORDS * 8;
    if (hipMalloc(&d->d_keys, 8ull << d->lg_slots) != hipSuccess || hipMalloc(&d->d_vals, 8ull << d->lg_slots) != hipSuccess ||
        hipMalloc(&d->d_codes, d->codes_cap * 4) != hipSuccess || hipMalloc(&d->d_big_tax, big_lanes * d->W * 4) != hipSuccess ||
        hipMalloc(&d->d_big_cnt, big_lanes * d->W * 4) != hipSuccess || hipMalloc(&d->d_ctr, K2D_CTR_WORDS * 8) != hipSuccess) {
        (void)hipGetLastError();
        sh_k2_distrib_free(d);
        sh_set_error("sh_k2_distrib_create: %llu bytes of device memory for %zu taxa at read length %d", (unsigned long long)bytes, db->nodes.size(), read_len);
        return SH_ERR_OOM;
    }
    sh_status st = sh_k2_distrib_reset(d);
    if (st != SH_OK) { sh_k2_distrib_free(d); return st; }
    *out = d;
    return SH_OK;
}

extern "C" sh_status sh_k2_distrib_add_device(sh_k2_distrib *d, const uint8_t *d_bases, const uint64_t *d_offsets, const uint32_t *d_taxa, uint64_t n_records,
                                              void *stream, sh_k2_distrib_stats *stats)
{
    SH_CHECK(d && d_offsets && d_taxa && (d_bases || n_records == 0), SH_ERR_BAD_ARG, "sh_k2_distrib_add_device: null argument");
    if (stats) memset(stats, 0, sizeof(*stats));
    SH_CHECK(!d->full, SH_ERR_OOM, "sh_k2_distrib_add_device: the (genome, mapped) table of %llu slots overflowed in an earlier call: reset the accumulator",
             1ull << d->lg_slots);
    if (n_records == 0) return SH_OK;
    SH_HIP(hipSetDevice(d->device));
    hipStream_t s = (hipStream_t)stream;
    DevEvent e0, e1, e2;
    SH_HIP(e0.create()); SH_HIP(e1.create()); SH_HIP(e2.create());
    K2DArgs a{};
    a.offsets = d_offsets; a.taxa = d_taxa; a.n_records = n_records; a.n_nodes = (uint32_t)d->db->nodes.size();
    a.parent = d->db->d_parent; a.L = d->read_len; a.W = d->W; a.S = k2d_stretch();
    a.keys = d->d_keys; a.vals = d->d_vals; a.lg_slots = d->lg_slots; a.ctr = d->d_ctr;
    a.big_tax = d->d_big_tax; a.big_cnt = d->d_big_cnt;
    unsigned long long c[K2D_CTR_WORDS] = {0}, n_items = 0;
    for (int attempt = 0;; ++attempt) {
        DevBuf b_seg, b_item, b_tmp, b_tmp2;
        SH_HIP(b_seg.alloc((n_records + 1) * 8));
        SH_HIP(b_item.alloc((n_records + 1) * 8));
        // every stretch is queued at most once, and a batch the scratch holds has at most codes_cap / S + n_records of them
        const uint64_t big_need = d->codes_cap / a.S + n_records + 1;
        if (d->big_cap < big_need) {
            hipFree(d->d_big); d->d_big = nullptr; d->big_cap = 0;
            SH_HIP(hipMalloc(&d->d_big, big_need * 8));
            d->big_cap = big_need;
        }
        a.item_off = b_item.as<uint64_t>(); a.codes = d->d_codes; a.codes_cap = d->codes_cap; a.big_list = d->d_big; a.big_cap = d->big_cap;
        SH_HIP(hipMemsetAsync(d->d_ctr, 0, K2D_CTR_WORDS * 8, s));
        SH_HIP(hipEventRecord(e0.e, s));
        sh_status st = shi_k2_codes_device(d->db, d_bases, d_offsets, d_taxa, n_records, b_seg.as<uint64_t>(), b_tmp, d->d_codes, d->codes_cap,
                                           d->d_ctr + K2D_NEED, s);
        if (st != SH_OK) return st;
        SH_HIP(hipEventRecord(e1.e, s));
        hipLaunchKernelGGL(k_k2_distrib_items, dim3((uint32_t)std::min<uint64_t>((n_records + 256) / 256, 4096)), dim3(256), 0, s, a);
        size_t tmp_bytes = 0;
        SH_HIP(rocprim::exclusive_scan(nullptr, tmp_bytes, a.item_off, a.item_off, (uint64_t)0, n_records + 1, rocprim::plus<uint64_t>(), s));
        SH_HIP(b_tmp2.alloc(std::max<size_t>(tmp_bytes, 1)));
        SH_HIP(rocprim::exclusive_scan(b_tmp2.p, tmp_bytes, a.item_off, a.item_off, (uint64_t)0, n_records + 1, rocprim::plus<uint64_t>(), s));
        hipLaunchKernelGGL(k_k2_distrib_windows<false>, dim3(K2D_GRID), dim3(64), 0, s, a);
        hipLaunchKernelGGL(k_k2_distrib_windows<true>, dim3(K2D_BIG_GRID), dim3(64), 0, s, a);
        SH_HIP(hipEventRecord(e2.e, s));
        SH_HIP(hipMemcpyAsync(c, d->d_ctr, sizeof(c), hipMemcpyDeviceToHost, s));
        SH_HIP(hipMemcpyAsync(&n_items, a.item_off + n_records, 8, hipMemcpyDeviceToHost, s));
        SH_HIP(hipStreamSynchronize(s));       // the one synchronisation of the batch
        SH_HIP(hipGetLastError());
        if (c[K2D_NEED] <= d->codes_cap) break;
        // more bases than the code scratch holds: nothing was tallied.  A larger one, and the batch again
        SH_CHECK(attempt == 0, SH_ERR_HIP, "sh_k2_distrib_add_device: the code scratch of %llu entries is too small again", (unsigned long long)d->codes_cap);
        const uint64_t cap = std::max<uint64_t>(c[K2D_NEED], 2 * d->codes_cap);
        hipFree(d->d_codes); d->d_codes = nullptr; d->codes_cap = 0;
        if (hipMalloc(&d->d_codes, cap * 4) != hipSuccess) {
            (void)hipGetLastError();
            sh_set_error("sh_k2_distrib_add_device: %llu bytes of device memory for the codes of a batch of %llu bases", (unsigned long long)(cap * 4), c[K2D_NEED]);
            return SH_ERR_OOM;
        }
        d->codes_cap = cap;
    }
    hipEventElapsedTime(&d->ms_codes, e0.e, e1.e);
    hipEventElapsedTime(&d->ms_windows, e1.e, e2.e);
    if (stats) {
        stats->n_records = n_records; stats->n_windows = c[K2D_NWIN]; stats->n_items = n_items; stats->n_big = c[K2D_NBIG];
        stats->ms = d->ms_codes + d->ms_windows;
    }
    if (c[K2D_FULL]) {
        d->full = true;
        sh_set_error("sh_k2_distrib_add_device: the (genome, mapped) table of %llu slots (%llu bytes) is full", 1ull << d->lg_slots, 16ull << d->lg_slots);
        return SH_ERR_OOM;
    }
    return SH_OK;
}

extern "C" sh_status sh_k2_distrib_last_ms(const sh_k2_distrib *d, float *ms_codes, float *ms_windows)
{
    SH_CHECK(d, SH_ERR_BAD_ARG, "sh_k2_distrib_last_ms: null argument");
    if (ms_codes) *ms_codes = d->ms_codes;
    if (ms_windows) *ms_windows = d->ms_windows;
    return SH_OK;
}

static bool k2d_entry_less(const sh_k2_distrib_entry &x, const sh_k2_distrib_entry &y)
{
    return x.genome != y.genome ? x.genome < y.genome : x.mapped < y.mapped;
}

static sh_status k2d_download(sh_k2_distrib *d, std::vector<sh_k2_distrib_entry> &v)
{
    SH_HIP(hipSetDevice(d->device));
    const uint64_t slots = 1ull << d->lg_slots;
    std::vector<unsigned long long> keys(slots), vals(slots);
    SH_HIP(hipMemcpy(keys.data(), d->d_keys, slots * 8, hipMemcpyDeviceToHost));
    SH_HIP(hipMemcpy(vals.data(), d->d_vals, slots * 8, hipMemcpyDeviceToHost));
    v.clear();
    for (uint64_t i = 0; i < slots; ++i)
        if (keys[i] != K2D_EMPTY && vals[i]) v.push_back(sh_k2_distrib_entry{(uint32_t)(keys[i] >> 32), (uint32_t)keys[i], vals[i]});
    std::sort(v.begin(), v.end(), k2d_entry_less);
    return SH_OK;
}

extern "C" sh_status sh_k2_distrib_count(sh_k2_distrib *d, uint64_t *n_entries)
{
    SH_CHECK(d && n_entries, SH_ERR_BAD_ARG, "sh_k2_distrib_count: null argument");
    std::vector<sh_k2_distrib_entry> v;
    sh_status st = k2d_download(d, v);
    *n_entries = v.size();
    return st;
}

extern "C" sh_status sh_k2_distrib_copy(sh_k2_distrib *d, sh_k2_distrib_entry *entries, uint64_t *totals)
{
    SH_CHECK(d, SH_ERR_BAD_ARG, "sh_k2_distrib_copy: null argument");
    std::vector<sh_k2_distrib_entry> v;
    sh_status st = k2d_download(d, v);
    if (st != SH_OK) return st;
    if (entries && !v.empty()) memcpy(entries, v.data(), v.size() * sizeof(sh_k2_distrib_entry));
    if (totals) {
        const size_t n = d->db->nodes.size();
        memset(totals, 0, n * 8);
        for (const auto &e : v) if (e.genome < n) totals[e.genome] += e.windows;
    }
    return SH_OK;
}

// ---- host only from here on: the distribution file, the estimate, the table ------------------------------------------------------
static const char K2D_HEADER[] = "mapped_taxid\tgenome_taxids:kmers_mapped:total_genome_kmers";

extern "C" sh_status sh_k2_distrib_write(const sh_k2_distrib_entry *entries, uint64_t n, const uint64_t *totals, const uint32_t *external, uint64_t n_nodes,
                                         int32_t read_len, const char *path)
{
    SH_CHECK((entries || n == 0) && totals && external && path, SH_ERR_BAD_ARG, "sh_k2_distrib_write: null argument");
    SH_CHECK(read_len >= 1 && read_len <= K2D_MAX_READ_LEN, SH_ERR_BAD_ARG, "sh_k2_distrib_write: read length %d", read_len);
    struct Row { uint32_t mapped, genome; uint64_t windows, total; };
    std::vector<Row> rows;
    for (uint64_t i = 0; i < n; ++i) {
        const sh_k2_distrib_entry &e = entries[i];
        SH_CHECK(e.genome != 0 && e.genome < n_nodes && e.mapped < n_nodes, SH_ERR_BAD_ARG, "sh_k2_distrib_write: entry %llu (%u, %u) is outside the taxonomy of %llu nodes",
                 (unsigned long long)i, e.genome, e.mapped, (unsigned long long)n_nodes);
        if (e.mapped == 0 || e.windows == 0) continue;          // unclassified windows count in the totals only
        rows.push_back(Row{external[e.mapped], external[e.genome], e.windows, totals[e.genome]});
    }
    std::sort(rows.begin(), rows.end(), [](const Row &x, const Row &y) { return x.mapped != y.mapped ? x.mapped < y.mapped : x.genome < y.genome; });
    FILE *f = fopen(path, "w");
    SH_CHECK(f, SH_ERR_IO, "cannot write %s", path);
    fprintf(f, "%s\n", K2D_HEADER);
    for (size_t i = 0; i < rows.size(); ++i) {
        const bool first = i == 0 || rows[i - 1].mapped != rows[i].mapped;
        if (first) fprintf(f, "%s%u\t", i ? "\n" : "", rows[i].mapped);
        fprintf(f, "%s%u:%llu:%llu", first ? "" : " ", rows[i].genome, (unsigned long long)rows[i].windows, (unsigned long long)rows[i].total);
    }
    if (!rows.empty()) fputc('\n', f);
    const bool bad = ferror(f) != 0;
    SH_CHECK(fclose(f) == 0 && !bad, SH_ERR_IO, "write to %s failed", path);
    return SH_OK;
}

// an unsigned decimal number at *p that ends at `stop`; advances *p behind the stop character
static bool k2d_number(const char *&p, char stop, uint64_t &v)
{
    if (*p < '0' || *p > '9') return false;
    v = 0;
    int digits = 0;
    for (; *p >= '0' && *p <= '9'; ++p, ++digits) v = v * 10 + (uint64_t)(*p - '0');
    if (digits > 19 || *p != stop) return false;
    if (stop) ++p;
    return true;
}

// the file into entries sorted by (genome, mapped) and the totals of the genomes it names
static sh_status k2d_read_file(const char *path, const uint32_t *external, uint64_t n_nodes, std::vector<sh_k2_distrib_entry> &v,
                               std::unordered_map<uint32_t, uint64_t> &total_of)
{
    std::unordered_map<uint64_t, uint32_t> ext2int;
    for (uint64_t i = 1; i < n_nodes; ++i) ext2int.emplace(external[i], (uint32_t)i);
    std::unordered_set<uint64_t> unknown;
    auto internal = [&](uint64_t ext) -> uint32_t {
        auto it = ext2int.find(ext);
        if (it != ext2int.end()) return it->second;
        if (unknown.insert(ext).second) fprintf(stderr, "[scrubby-hip] %s: taxid %llu is not in the taxonomy: skipped\n", path, (unsigned long long)ext);
        return 0;
    };
    FILE *f = fopen(path, "r");
    SH_CHECK(f, SH_ERR_IO, "cannot open %s", path);
    v.clear(); total_of.clear();
    char *line = nullptr; size_t lcap = 0; ssize_t got;
    uint64_t ln = 0;
    bool ok = true;
    while (ok && (got = getline(&line, &lcap, f)) > 0) {
        ++ln;
        while (got > 0 && (line[got - 1] == '\n' || line[got - 1] == '\r')) line[--got] = 0;
        if (ln == 1) { ok = strcmp(line, K2D_HEADER) == 0; continue; }
        const char *p = line;
        uint64_t mapped_ext;
        ok = k2d_number(p, '\t', mapped_ext) && *p != 0;
        if (!ok) break;
        const uint32_t mapped = internal(mapped_ext);
        while (ok && *p) {
            uint64_t g_ext, w, t;
            ok = k2d_number(p, ':', g_ext) && k2d_number(p, ':', w);
            if (!ok) break;
            const char *q = p;
            while (*q >= '0' && *q <= '9') ++q;
            ok = q > p && (*q == 0 || (*q == ' ' && q[1] != 0)) && k2d_number(p, *q, t);
            if (!ok) break;
            const uint32_t g = internal(g_ext);
            if (!g) continue;
            auto it = total_of.emplace(g, t);
            ok = it.first->second == t;      // a genome has one total
            if (mapped) v.push_back(sh_k2_distrib_entry{g, mapped, w});
        }
    }
    free(line);
    fclose(f);
    SH_CHECK(ln >= 1, SH_ERR_IO, "%s: line 1: the header line is missing", path);
    SH_CHECK(ok, SH_ERR_IO, "%s: line %llu is malformed", path, (unsigned long long)ln);
    std::sort(v.begin(), v.end(), k2d_entry_less);
    for (size_t i = 1; i < v.size(); ++i)
        SH_CHECK(k2d_entry_less(v[i - 1], v[i]), SH_ERR_IO, "%s: genome %u maps to taxon %u twice", path, external[v[i].genome], external[v[i].mapped]);
    return SH_OK;
}

extern "C" sh_status sh_k2_distrib_read(const char *path, const uint32_t *external, uint64_t n_nodes, sh_k2_distrib_entry *entries, uint64_t cap,
                                        uint64_t *n_entries, uint64_t *totals)
{
    SH_CHECK(path && external && n_entries, SH_ERR_BAD_ARG, "sh_k2_distrib_read: null argument");
    *n_entries = 0;
    std::vector<sh_k2_distrib_entry> v;
    std::unordered_map<uint32_t, uint64_t> total_of;
    sh_status st = k2d_read_file(path, external, n_nodes, v, total_of);
    if (st != SH_OK) return st;
    *n_entries = v.size();
    if (totals) {
        memset(totals, 0, n_nodes * 8);
        for (const auto &t : total_of) totals[t.first] = t.second;
    }
    if (entries && cap >= v.size() && !v.empty()) memcpy(entries, v.data(), v.size() * sizeof(sh_k2_distrib_entry));
    return SH_OK;
}

static const char *k2d_level_rank(int32_t level)
{
    switch (level) {
    case 'D': return "superkingdom";
    case 'K': return "kingdom";
    case 'P': return "phylum";
    case 'C': return "class";
    case 'O': return "order";
    case 'F': return "family";
    case 'G': return "genus";
    case 'S': return "species";
    default: return nullptr;
    }
}

extern "C" sh_status sh_k2_bracken_estimate(const sh_k2_taxnode *nodes, uint64_t n_nodes, const char *ranks, uint64_t ranks_len, const uint64_t *direct_reads,
                                            const sh_k2_distrib_entry *entries, uint64_t n, const uint64_t *totals, int32_t level, uint64_t threshold,
                                            sh_k2_bracken_row *rows, sh_k2_bracken_summary *summary)
{
    SH_CHECK(nodes && n_nodes >= 2 && ranks && direct_reads && (entries || n == 0) && totals && summary, SH_ERR_BAD_ARG, "sh_k2_bracken_estimate: null argument");
    const char *rank = k2d_level_rank(level);
    SH_CHECK(rank, SH_ERR_BAD_ARG, "sh_k2_bracken_estimate: level '%c' is not one of D K P C O F G S", level > 32 && level < 127 ? level : '?');
    memset(summary, 0, sizeof(*summary));
    const size_t rl = strlen(rank);
    auto at_level = [&](uint64_t i) {
        const uint64_t o = nodes[i].rank_offset;
        return o + rl < ranks_len && memcmp(ranks + o, rank, rl + 1) == 0;
    };
    std::vector<uint32_t> lvl(n_nodes, 0);
    std::vector<uint64_t> clade(direct_reads, direct_reads + n_nodes);
    clade[0] = 0;
    for (uint64_t i = 1; i < n_nodes; ++i) {
        SH_CHECK(i == 1 || (nodes[i].parent >= 1 && nodes[i].parent < i), SH_ERR_BAD_ARG, "sh_k2_bracken_estimate: node %llu has parent %llu (ids must be breadth-first)",
                 (unsigned long long)i, (unsigned long long)nodes[i].parent);
        lvl[i] = at_level(i) ? (uint32_t)i : (i == 1 ? 0u : lvl[nodes[i].parent]);
        summary->reads_total += direct_reads[i];
    }
    for (uint64_t i = n_nodes - 1; i >= 2; --i) clade[nodes[i].parent] += clade[i];
    const uint64_t floor_reads = std::max<uint64_t>(threshold, 1);
    std::vector<uint8_t> kept(n_nodes, 0);
    for (uint64_t i = 1; i < n_nodes; ++i) {
        if (lvl[i] != i) continue;
        if (clade[i] >= floor_reads) { kept[i] = 1; summary->reads_at_level += clade[i]; }
        else summary->reads_below_threshold += clade[i];
    }
    // per kept taxon: the windows of its genomes in all; per (mapped node, kept taxon): the windows of its genomes that map there
    std::vector<uint64_t> T(n_nodes, 0);
    for (uint64_t g = 1; g < n_nodes; ++g) if (kept[lvl[g]]) T[lvl[g]] += totals[g];
    std::map<uint32_t, std::map<uint32_t, uint64_t>> M;
    for (uint64_t i = 0; i < n; ++i) {
        const sh_k2_distrib_entry &e = entries[i];
        SH_CHECK(e.genome != 0 && e.genome < n_nodes && e.mapped < n_nodes, SH_ERR_BAD_ARG, "sh_k2_bracken_estimate: entry %llu (%u, %u) is outside the taxonomy of %llu nodes",
                 (unsigned long long)i, e.genome, e.mapped, (unsigned long long)n_nodes);
        if (e.mapped && kept[lvl[e.genome]]) M[e.mapped][lvl[e.genome]] += e.windows;
    }
    std::vector<double> added(n_nodes, 0.0);
    std::vector<std::pair<uint32_t, double>> w;
    for (uint64_t x = 1; x < n_nodes; ++x) {
        if (direct_reads[x] == 0 || lvl[x] != 0) continue;
        w.clear();
        double sum = 0.0;
        auto it = M.find((uint32_t)x);
        if (it != M.end())
            for (const auto &ms : it->second) {      // ascending s
                const uint32_t s = ms.first;
                const double ws = T[s] ? (double)ms.second / (double)T[s] * (double)clade[s] : 0.0;
                w.emplace_back(s, ws);
                sum += ws;
            }
        if (!(sum > 0.0)) { summary->reads_undistributed += direct_reads[x]; continue; }
        summary->reads_distributed += direct_reads[x];
        for (const auto &sw : w) added[sw.first] += (double)direct_reads[x] * sw.second / sum;
    }
    std::vector<sh_k2_bracken_row> out;
    for (uint64_t s = 1; s < n_nodes; ++s) {
        if (!kept[s]) continue;
        sh_k2_bracken_row r{};
        r.taxon = (uint32_t)s; r.assigned = clade[s]; r.added = added[s];
        r.new_est = (uint64_t)floor((double)clade[s] + added[s] + 0.5);
        summary->new_est_total += r.new_est;
        out.push_back(r);
    }
    for (auto &r : out) r.fraction = summary->new_est_total ? (double)r.new_est / (double)summary->new_est_total : 0.0;
    summary->n_rows = out.size();
    if (rows && !out.empty()) memcpy(rows, out.data(), out.size() * sizeof(sh_k2_bracken_row));
    return SH_OK;
}

extern "C" sh_status sh_k2_bracken_write(const sh_k2_taxnode *nodes, uint64_t n_nodes, const char *names, uint64_t names_len, const sh_k2_bracken_row *rows,
                                         uint64_t n_rows, int32_t level, const char *path)
{
    SH_CHECK(nodes && names && (rows || n_rows == 0), SH_ERR_BAD_ARG, "sh_k2_bracken_write: null argument");
    SH_CHECK(k2d_level_rank(level), SH_ERR_BAD_ARG, "sh_k2_bracken_write: level '%c' is not one of D K P C O F G S", level > 32 && level < 127 ? level : '?');
    std::vector<const sh_k2_bracken_row *> order;
    for (uint64_t i = 0; i < n_rows; ++i) {
        SH_CHECK(rows[i].taxon >= 1 && rows[i].taxon < n_nodes, SH_ERR_BAD_ARG, "sh_k2_bracken_write: row %llu names taxon %u of %llu", (unsigned long long)i, rows[i].taxon,
                 (unsigned long long)n_nodes);
        order.push_back(rows + i);
    }
    std::sort(order.begin(), order.end(), [&](const sh_k2_bracken_row *x, const sh_k2_bracken_row *y) { return nodes[x->taxon].external_id < nodes[y->taxon].external_id; });
    const bool to_stdout = !path || strcmp(path, "-") == 0;
    FILE *f = to_stdout ? stdout : fopen(path, "w");
    SH_CHECK(f, SH_ERR_IO, "cannot write %s", path);
    fprintf(f, "name\ttaxonomy_id\ttaxonomy_lvl\tkraken_assigned_reads\tadded_reads\tnew_est_reads\tfraction_total_reads\n");
    for (const sh_k2_bracken_row *r : order) {
        const uint64_t no = nodes[r->taxon].name_offset;
        const std::string name = no < names_len ? std::string(names + no, strnlen(names + no, names_len - no)) : std::string();
        fprintf(f, "%s\t%llu\t%c\t%llu\t%lld\t%llu\t%.5f\n", name.c_str(), (unsigned long long)nodes[r->taxon].external_id, (char)level, (unsigned long long)r->assigned,
                (long long)r->new_est - (long long)r->assigned, (unsigned long long)r->new_est, r->fraction);
    }
    const bool bad = ferror(f) != 0;
    if (to_stdout) fflush(f);
    else SH_CHECK(fclose(f) == 0 && !bad, SH_ERR_IO, "write to %s failed", path);
    return SH_OK;
}

// taxo.k2d on the host alone (sh_k2_open reads it on its way to HBM)
static sh_status k2d_read_taxonomy(const char *dir, std::vector<sh_k2_taxnode> &nodes, std::string &names, std::string &ranks)
{
    const std::string p = std::string(dir) + "/taxo.k2d";
    FILE *f = fopen(p.c_str(), "rb");
    SH_CHECK(f, SH_ERR_IO, "cannot open %s", p.c_str());
    char magic[8]; uint64_t hdr[3];
    bool ok = fread(magic, 8, 1, f) == 1 && memcmp(magic, "K2TAXDAT", 8) == 0 && fread(hdr, 8, 3, f) == 3 && hdr[0] < (1ull << 31) && hdr[1] < (1ull << 40) && hdr[2] < (1ull << 40);
    if (ok) {
        nodes.resize(hdr[0]); names.resize(hdr[1]); ranks.resize(hdr[2]);
        ok = fread(nodes.data(), sizeof(sh_k2_taxnode), hdr[0], f) == hdr[0];
        ok = ok && (hdr[1] == 0 || fread(&names[0], 1, hdr[1], f) == hdr[1]);
        ok = ok && (hdr[2] == 0 || fread(&ranks[0], 1, hdr[2], f) == hdr[2]);
    }
    fclose(f);
    SH_CHECK(ok && nodes.size() >= 2, SH_ERR_IO, "%s is not a Kraken 2 taxonomy", p.c_str());
    return SH_OK;
}

extern "C" sh_status sh_k2_bracken_run(const sh_k2_bracken_config *c, sh_k2_bracken_result *res)
{
    SH_CHECK(c && res, SH_ERR_BAD_ARG, "sh_k2_bracken_run: null argument");
    SH_CHECK(c->db && c->report && c->output, SH_ERR_BAD_ARG, "k2-bracken: a database (-d), a report (-r) and an output (-o) are required");
    SH_CHECK(c->kmer_distrib || (c->read_len >= 1 && c->read_len <= K2D_MAX_READ_LEN), SH_ERR_BAD_ARG, "k2-bracken: a read length (-l) in [1, %d] or a distribution file (-k)",
             K2D_MAX_READ_LEN);
    memset(res, 0, sizeof(*res));
    const int32_t level = c->level ? c->level : 'S';
    SH_CHECK(k2d_level_rank(level), SH_ERR_BAD_ARG, "k2-bracken: level '%c' is not one of D K P C O F G S", level > 32 && level < 127 ? level : '?');
    std::vector<sh_k2_taxnode> nodes; std::string names, ranks;
    sh_status st = k2d_read_taxonomy(c->db, nodes, names, ranks);
    if (st != SH_OK) return st;
    const uint64_t n = nodes.size();
    std::vector<uint32_t> ext(n);
    std::unordered_map<uint64_t, uint32_t> ext2int;
    for (uint64_t i = 0; i < n; ++i) { ext[i] = (uint32_t)nodes[i].external_id; if (i) ext2int.emplace(nodes[i].external_id, (uint32_t)i); }
    // kraken.report: percent, clade reads, direct reads, rank code, taxid, name
    std::vector<uint64_t> direct(n, 0);
    uint64_t lost = 0;
    {
        FILE *f = fopen(c->report, "r");
        SH_CHECK(f, SH_ERR_IO, "cannot open %s", c->report);
        char *line = nullptr; size_t lcap = 0; uint64_t ln = 0; bool ok = true;
        std::unordered_set<uint64_t> unknown;
        while (ok && getline(&line, &lcap, f) > 0) {
            ++ln;
            if (line[0] == '\n' || line[0] == '\r' || line[0] == '#') continue;
            const char *p = strchr(line, '\t');
            uint64_t clade_reads, direct_reads, taxid;
            ok = p != nullptr;
            if (ok) { ++p; while (*p == ' ') ++p; ok = k2d_number(p, '\t', clade_reads); }
            if (ok) { while (*p == ' ') ++p; ok = k2d_number(p, '\t', direct_reads); }
            if (ok) { p = strchr(p, '\t'); ok = p != nullptr; }
            if (ok) { ++p; while (*p == ' ') ++p; ok = k2d_number(p, '\t', taxid); }
            if (!ok) break;
            ++res->n_report_rows;
            if (taxid == 0) { direct[0] += direct_reads; continue; }
            auto it = ext2int.find(taxid);
            if (it != ext2int.end()) { direct[it->second] += direct_reads; continue; }
            if (unknown.insert(taxid).second) fprintf(stderr, "[scrubby-hip] k2-bracken: taxid %llu of %s is not in the database: its reads stay undistributed\n",
                                                      (unsigned long long)taxid, c->report);
            lost += direct_reads;
        }
        free(line);
        fclose(f);
        SH_CHECK(ok, SH_ERR_IO, "%s: line %llu is not a row of a Kraken report", c->report, (unsigned long long)ln);
        res->n_unknown_taxa = unknown.size();
    }
    const std::string dist = c->kmer_distrib ? std::string(c->kmer_distrib) : std::string(c->db) + "/database" + std::to_string(c->read_len) + "mers.kmer_distrib";
    std::vector<uint64_t> totals(n, 0);
    std::vector<sh_k2_distrib_entry> entries;
    std::unordered_map<uint32_t, uint64_t> total_of;
    st = k2d_read_file(dist.c_str(), ext.data(), n, entries, total_of);
    if (st != SH_OK) return st;
    for (const auto &t : total_of) totals[t.first] = t.second;
    const uint64_t ne = entries.size();
    std::vector<sh_k2_bracken_row> rows(n);
    st = sh_k2_bracken_estimate(nodes.data(), n, ranks.data(), ranks.size(), direct.data(), entries.data(), ne, totals.data(), level,
                                c->threshold < 0 ? 10 : (uint64_t)c->threshold, rows.data(), &res->summary);
    if (st != SH_OK) return st;
    res->summary.reads_total += lost; res->summary.reads_undistributed += lost;
    return sh_k2_bracken_write(nodes.data(), n, names.data(), names.size(), rows.data(), res->summary.n_rows, level, c->output);
}
