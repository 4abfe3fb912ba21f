// sh_bam.hip — BAM records filtered on the device: the reader behind `scrubby alignment -a x.bam` when SCRUBBY_HIP_GUNZIP_DEVICE is on
// (DESIGN.md §6 "SAM / BAM").
//
// The inflated record stream lies in HBM (sh_inflate.hip put it there).  Record starts form a chain of dependent loads - a record's
// length word says where the next one begins - and one wave following it would pay HBM latency once per record.  So the window is cut
// into segments of SHB_SEGMENT bytes at fixed offsets, and every dependency is a launch boundary:
//
//   k_bam_probe   one wave per segment.  The segment and the SHB_HALO bytes behind it are staged in LDS; the lanes test 64 positions at a
//                 time with shb_record_ok (sh_bam.h, the code the host tests check) and a ballot appends the plausible starts to the
//                 segment's table, SHB_SEGMENT_CAP entries, one per lane.  Then from the highest start down each gets its exit: the
//                 first chain position at or past the segment's end, or BROKEN (the chain from it meets a position inside the segment
//                 that is no record), or OPEN (it meets a record the window cuts off).  A start's successor inside the segment is a
//                 higher entry of the same table, found by a ballot, so every start costs one step.  A segment with more plausible
//                 starts than the table holds keeps only the count: it has overflowed.
//   k_bam_chain   ONE wave goes from segment to segment: it looks its position up in the segment's table (lanes compare, a ballot),
//                 notes it as the segment's entry and takes the exit.  A record longer than a segment skips segments.  It stops at the
//                 window's end, at OPEN, at BROKEN, or in front of an overflowed segment.
//   k_bam_filter  one wave per entered segment walks its records from the entry (their starts into LDS), then lane r decides record r with
//                 shb_fields / shb_qalen / shb_select; a record with more than SHB_LANE_CIGAR ops is summed by the whole wave, lanes over
//                 CIGAR words and a wave reduction.  Launched twice: it counts the name bytes of a segment, rocPRIM scans the counts,
//                 and the second launch writes each selected name behind the ones before it, so the names leave in record order.
//
// Overflowed segments are walked on the host (shb_walk over a copy of the window, taken once per call) from the chain's entry to the
// first segment that has not overflowed; their names go up to their place behind the scan.  The answer is the same either way.
//
// Bounds: every load is below n (shb_record_ok and shb_complete are asked before a record is read, and the filter reads only records the
// chain has passed); a table write is below SHB_SEGMENT_CAP, a record-start write below FILTER_MAX_RECORDS, a name write below
// names_cap; every chain step is forward by SHB_MIN_STEP bytes at least, so no input makes a loop.
#include "sh_common.h"
#include "sh_codec.h"
#include "sh_bam.h"
#include "sh_wave.h"
#include <rocprim/rocprim.hpp>
#include <algorithm>
#include <chrono>
#include <string>
#include <unordered_set>

static_assert(sizeof(ShbRule) == sizeof(sh_bam_rule) && offsetof(ShbRule, min_cov) == offsetof(sh_bam_rule, min_cov) && offsetof(ShbRule, n_ref) == offsetof(sh_bam_rule, n_ref),
              "ShbRule is sh_bam_rule");
static_assert(SHB_SEGMENT % 64 == 0 && SHB_SEGMENT_CAP == 64, "one table entry per lane");

namespace {

constexpr uint32_t NONE = 0xffffffffu;
constexpr uint32_t FILTER_MAX_RECORDS = SHB_SEGMENT / SHB_MIN_STEP + 2;      // record starts of one segment
constexpr uint32_t PROBE_LDS = (SHB_SEGMENT + SHB_HALO + 7) / 4 * 4;
enum : uint32_t { RES_EXIT = 0, RES_BROKEN = 1, RES_OPEN = 2 };              // a table entry's result: kind << 32 | position
enum : uint32_t { CHAIN_END = 0, CHAIN_OPEN = 1, CHAIN_BROKEN = 2, CHAIN_OVERFLOW = 3 };

struct ChainOut { uint32_t status, pos; };
struct DevCounts { unsigned long long n_records, n_unmapped, n_selected, n_cg, n_segments, n_plausible; };

// the window through an LDS copy of text[base, base + len); what lies outside comes from HBM
struct LdsSrc {
    const uint8_t *text;
    const uint8_t *lds;
    uint32_t base, len;
    __device__ uint32_t byte(uint64_t pos) const
    {
        const uint32_t off = (uint32_t)pos - base;
        return off < len ? lds[off] : text[pos];
    }
};

__global__ __launch_bounds__(64) void k_bam_probe(const uint8_t *__restrict__ text, uint32_t n, int32_t n_ref, uint32_t *__restrict__ cnt, uint32_t *__restrict__ tab_start,
                                                  unsigned long long *__restrict__ tab_res, DevCounts *counts)
{
    __shared__ __attribute__((aligned(8))) uint8_t s_text[PROBE_LDS];
    __shared__ uint32_t s_start[SHB_SEGMENT_CAP];
    __shared__ unsigned long long s_res[SHB_SEGMENT_CAP];
    const uint32_t lane = threadIdx.x, seg = blockIdx.x;
    const uint32_t lo = seg * SHB_SEGMENT, hi = min(lo + SHB_SEGMENT, n), len = min(hi + SHB_HALO, n) - lo;
    if (((uintptr_t)text & 3) == 0) {
        const uint32_t *src4 = (const uint32_t *)(text + lo);
        uint32_t *dst4 = (uint32_t *)s_text;
        for (uint32_t i = lane; i < len / 4; i += 64) dst4[i] = src4[i];
        for (uint32_t i = (len & ~3u) + lane; i < len; i += 64) s_text[i] = text[lo + i];
    } else
        for (uint32_t i = lane; i < len; i += 64) s_text[i] = text[lo + i];
    __syncthreads();
    const LdsSrc src{text, s_text, lo, len};
    uint32_t total = 0;
    for (uint32_t it = 0; it < SHB_SEGMENT / 64; ++it) {
        const uint32_t p = lo + it * 64 + lane;
        const bool ok = p < hi && shb_record_ok(src, p, n, n_ref);
        const unsigned long long mask = __ballot(ok);
        if (ok) {
            const uint32_t idx = total + __popcll(mask & ((1ull << lane) - 1));
            if (idx < SHB_SEGMENT_CAP) s_start[idx] = p;
        }
        total += __popcll(mask);
    }
    __syncthreads();
    if (lane == 0) { cnt[seg] = total; atomicAdd(&counts->n_plausible, (unsigned long long)total); }
    if (total > SHB_SEGMENT_CAP) return;      // overflowed: the count says so
    const uint32_t mine = lane < total ? s_start[lane] : NONE;
    for (uint32_t i = total; i-- > 0;) {      // wave-uniform: every lane follows start i
        const uint32_t s = s_start[i];
        unsigned long long res;
        if (!shb_complete(src, s, n)) res = (unsigned long long)RES_OPEN << 32 | s;
        else {
            const uint32_t q = s + 4 + shb_u32(src, s);      // <= n, and n < 2^31
            const unsigned long long hit = __ballot(lane > i && mine == q);
            if (q >= hi) res = (unsigned long long)RES_EXIT << 32 | q;
            else if (hit == 0) res = (unsigned long long)RES_BROKEN << 32 | q;
            else res = s_res[__ffsll(hit) - 1];
        }
        __syncthreads();
        if (lane == 0) s_res[i] = res;
        __syncthreads();
    }
    if (lane < total) {
        tab_start[(size_t)seg * SHB_SEGMENT_CAP + lane] = mine;
        tab_res[(size_t)seg * SHB_SEGMENT_CAP + lane] = s_res[lane];
    }
}

__global__ __launch_bounds__(64) void k_bam_chain(uint32_t n, uint32_t from, const uint32_t *__restrict__ cnt, const uint32_t *__restrict__ tab_start,
                                                  const unsigned long long *__restrict__ tab_res, uint32_t *__restrict__ entry, ChainOut *out)
{
    const uint32_t lane = threadIdx.x;
    uint32_t pos = from, status = CHAIN_END;
    while (pos < n) {
        const uint32_t seg = pos / SHB_SEGMENT;
        const uint32_t c = cnt[seg];
        if (c > SHB_SEGMENT_CAP) { status = CHAIN_OVERFLOW; break; }
        const unsigned long long hit = __ballot(lane < c && tab_start[(size_t)seg * SHB_SEGMENT_CAP + lane] == pos);
        if (hit == 0) { status = CHAIN_BROKEN; break; }
        const unsigned long long res = tab_res[(size_t)seg * SHB_SEGMENT_CAP + (__ffsll(hit) - 1)];
        const uint32_t kind = (uint32_t)(res >> 32);
        if (lane == 0) entry[seg] = pos;
        pos = (uint32_t)res;      // an exit lies at or past the segment's end: forward
        if (kind == RES_BROKEN) { status = CHAIN_BROKEN; break; }
        if (kind == RES_OPEN) { status = CHAIN_OPEN; break; }
    }
    if (lane == 0) { out->status = status; out->pos = pos; }
}

// write == 0: bytes[seg] = the name bytes of the segment's selected records, and the counts; write != 0: the names at off[seg]
__global__ __launch_bounds__(64) void k_bam_filter(const uint8_t *__restrict__ text, uint32_t stop, ShbRule rule, const uint32_t *__restrict__ entry, uint32_t *__restrict__ bytes,
                                                   const unsigned long long *__restrict__ off, uint8_t *__restrict__ names, unsigned long long names_cap, DevCounts *counts,
                                                   int write)
{
    __shared__ uint32_t s_pos[FILTER_MAX_RECORDS], s_len[FILTER_MAX_RECORDS];
    const uint32_t lane = threadIdx.x, seg = blockIdx.x;
    const uint32_t e = entry[seg];
    if (e == NONE) { if (!write && lane == 0) bytes[seg] = 0; return; }
    const uint32_t hi = min((seg + 1) * SHB_SEGMENT, stop);
    const ShbPtrSrc src{text};
    uint32_t n_rec = 0;
    for (uint32_t p = e; p < hi && n_rec < FILTER_MAX_RECORDS; ++n_rec) {      // wave-uniform; every record here is one the chain has passed
        if (lane == 0) s_pos[n_rec] = p;
        p += 4 + shb_u32(src, p);
    }
    __syncthreads();
    uint32_t n_unmapped = 0, n_cg = 0;
    for (uint32_t r0 = 0; r0 < n_rec; r0 += 64) {
        const uint32_t r = r0 + lane;
        bool big = false;
        if (r < n_rec) {
            const ShbRec rec = shb_fields(src, s_pos[r]);
            uint32_t len = 0;
            if (rec.flag & 4u) ++n_unmapped;
            else {
                n_cg += rec.cg;
                if (rec.cig_n > SHB_LANE_CIGAR) big = true;
                else if (shb_select(rec, shb_qalen(src, rec, 0, 1), rule)) len = rec.name_len + 1;
            }
            s_len[r] = len;
        }
        for (unsigned long long todo = __ballot(big); todo; todo &= todo - 1) {      // the whole wave on one record
            const uint32_t rr = r0 + (uint32_t)__ffsll(todo) - 1;
            const ShbRec rec = shb_fields(src, s_pos[rr]);
            const uint64_t qalen = wave_all_add_u64(shb_qalen(src, rec, lane, 64));
            if (lane == 0) s_len[rr] = shb_select(rec, qalen, rule) ? rec.name_len + 1 : 0;
        }
    }
    __syncthreads();
    if (!write) {
        uint32_t sum = 0, sel = 0;
        for (uint32_t r = lane; r < n_rec; r += 64) { sum += s_len[r]; sel += s_len[r] != 0; }
        sum = wave_sum_u32(sum); sel = wave_sum_u32(sel); n_unmapped = wave_sum_u32(n_unmapped); n_cg = wave_sum_u32(n_cg);
        if (lane == 0) {
            bytes[seg] = sum;
            atomicAdd(&counts->n_records, (unsigned long long)n_rec);
            atomicAdd(&counts->n_unmapped, (unsigned long long)n_unmapped);
            atomicAdd(&counts->n_selected, (unsigned long long)sel);
            atomicAdd(&counts->n_cg, (unsigned long long)n_cg);
            if (n_rec) atomicAdd(&counts->n_segments, 1ull);
        }
        return;
    }
    unsigned long long at = off[seg];
    for (uint32_t r0 = 0; r0 < n_rec; r0 += 64) {
        const uint32_t r = r0 + lane, len = r < n_rec ? s_len[r] : 0;
        const uint32_t incl = (uint32_t)wave_scan_add_incl((int32_t)len);
        if (len) {
            const unsigned long long dst = at + incl - len;
            const uint64_t name = (uint64_t)s_pos[r] + 36;
            for (uint32_t i = 0; i < len && dst + i < names_cap; ++i) names[dst + i] = i + 1 < len ? text[name + i] : 0;
        }
        at += rdlane(incl, 63);
    }
}

struct DeviceScope {      // the scanner's device for the length of a call, the caller's afterwards
    int prev = 0;
    bool have = false;
    hipError_t err;
    explicit DeviceScope(int device) { have = hipGetDevice(&prev) == hipSuccess; err = hipSetDevice(device); }
    ~DeviceScope() { if (have) hipSetDevice(prev); }
    DeviceScope(const DeviceScope &) = delete;
};

}      // namespace

struct sh_bam_scanner {
    int32_t device = 0;
    uint64_t max_bytes = 0, max_seg = 0;
    uint32_t *d_cnt = nullptr, *d_tab_start = nullptr, *d_entry = nullptr, *d_bytes = nullptr;
    unsigned long long *d_tab_res = nullptr, *d_off = nullptr;
    DevCounts *d_counts = nullptr;
    ChainOut *d_chain = nullptr;
    void *d_scan_tmp = nullptr;
    size_t scan_tmp_bytes = 0;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    std::vector<uint8_t> h_text;      // the window on the host, taken when a call first meets an overflowed segment
    std::vector<uint32_t> h_cnt;
};

extern "C" uint32_t sh_bam_segment(void) { return SHB_SEGMENT; }
extern "C" uint32_t sh_bam_segment_cap(void) { return SHB_SEGMENT_CAP; }
extern "C" uint64_t sh_bam_names_bound(uint64_t n) { return shb_names_bound(n); }

extern "C" sh_status sh_bam_header(const uint8_t *text, uint64_t n, int32_t *n_ref, uint64_t *first_record, int32_t *stopped)
{
    SH_CHECK((text || n == 0) && n_ref && first_record && stopped, SH_ERR_BAD_ARG, "sh_bam_header: null argument");
    *n_ref = 0; *first_record = 0;
    *stopped = shb_header(ShbPtrSrc{text}, n, n_ref, first_record);
    return SH_OK;
}

extern "C" sh_status sh_bam_plausible_host(const uint8_t *text, uint64_t n, int32_t n_ref, uint32_t *counts, uint64_t n_counts)
{
    const uint64_t n_seg = (n + SHB_SEGMENT - 1) / SHB_SEGMENT;
    SH_CHECK((text || n == 0) && (counts || n_seg == 0), SH_ERR_BAD_ARG, "sh_bam_plausible_host: null argument");
    SH_CHECK(n_counts >= n_seg, SH_ERR_BAD_ARG, "sh_bam_plausible_host: room for %llu counts, %llu bytes are %llu segments", (unsigned long long)n_counts, (unsigned long long)n,
             (unsigned long long)n_seg);
    const ShbPtrSrc src{text};
    for (uint64_t s = 0; s < n_seg; ++s) {
        uint32_t c = 0;
        for (uint64_t p = s * SHB_SEGMENT; p < std::min<uint64_t>((s + 1) * SHB_SEGMENT, n); ++p) c += shb_record_ok(src, p, n, n_ref);
        counts[s] = c;
    }
    return SH_OK;
}

static sh_status bam_check_args(const char *who, const void *text, uint64_t n, uint64_t entry, const sh_bam_rule *rule, const void *names, uint64_t names_cap, const uint64_t *names_len,
                                const uint64_t *next_entry)
{
    SH_CHECK((text || n == 0) && rule && names_len && next_entry && (names || names_cap == 0), SH_ERR_BAD_ARG, "%s: null argument", who);
    SH_CHECK(entry <= n, SH_ERR_BAD_ARG, "%s: entry %llu lies behind the window of %llu bytes", who, (unsigned long long)entry, (unsigned long long)n);
    SH_CHECK(rule->n_ref >= 0, SH_ERR_BAD_ARG, "%s: n_ref %d", who, rule->n_ref);
    SH_CHECK(names_cap >= shb_names_bound(n - entry), SH_ERR_BAD_ARG, "%s: room for %llu name bytes, %llu bytes of records may hold %llu", who, (unsigned long long)names_cap,
             (unsigned long long)(n - entry), (unsigned long long)shb_names_bound(n - entry));
    return SH_OK;
}

static sh_status bam_chain_end(int how, uint64_t pos, uint64_t n, uint64_t base, int32_t last)
{
    SH_CHECK(how != SHB_WALK_BROKEN, SH_ERR_IO, "not a BAM record at %llu", (unsigned long long)(base + pos));
    SH_CHECK(!last || pos == n, SH_ERR_IO, "truncated BAM record at %llu", (unsigned long long)(base + pos));
    return SH_OK;
}

extern "C" sh_status sh_bam_filter_host(const uint8_t *text, uint64_t n, uint64_t base, uint64_t entry, int32_t last, const sh_bam_rule *rule, uint8_t *names, uint64_t names_cap,
                                        uint64_t *names_len, uint64_t *next_entry, sh_bam_stats *stats)
{
    if (stats) memset(stats, 0, sizeof *stats);
    const sh_status ok = bam_check_args("sh_bam_filter_host", text, n, entry, rule, names, names_cap, names_len, next_entry);
    if (ok != SH_OK) return ok;
    *names_len = 0; *next_entry = entry;
    const auto t0 = std::chrono::steady_clock::now();
    ShbRule r; memcpy(&r, rule, sizeof r);
    ShbCounts c{};
    uint64_t pos = entry, len = 0, last_seg = ~0ull;
    const int how = shb_walk(ShbPtrSrc{text}, n, entry, n, r, names, names_cap, &len, &pos, &c, &last_seg);
    SH_CHECK(how != SHB_WALK_CAP, SH_ERR_BAD_ARG, "sh_bam_filter_host: the names leave their %llu bytes", (unsigned long long)names_cap);
    const sh_status end = bam_chain_end(how, pos, n, base, last);
    if (end != SH_OK) return end;
    *names_len = len; *next_entry = pos;
    if (stats) {
        stats->n_records = c.n_records; stats->n_unmapped = c.n_unmapped; stats->n_selected = c.n_selected; stats->n_cg = c.n_cg; stats->n_segments = c.n_segments;
        stats->name_bytes = c.name_bytes;
        stats->ms = stats->ms_filter = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    return SH_OK;
}

extern "C" sh_status sh_bam_scanner_free(sh_bam_scanner *sc)
{
    if (!sc) return SH_OK;
    DeviceScope scope(sc->device);
    for (void *p : {(void *)sc->d_cnt, (void *)sc->d_tab_start, (void *)sc->d_entry, (void *)sc->d_bytes, (void *)sc->d_tab_res, (void *)sc->d_off, (void *)sc->d_counts,
                    (void *)sc->d_chain, sc->d_scan_tmp})
        if (p) hipFree(p);
    for (hipEvent_t e : sc->ev) if (e) hipEventDestroy(e);
    delete sc;
    return SH_OK;
}

extern "C" sh_status sh_bam_scanner_create(int32_t device, uint64_t max_bytes, sh_bam_scanner **out)
{
    SH_CHECK(out, SH_ERR_BAD_ARG, "sh_bam_scanner_create: null argument");
    *out = nullptr;
    SH_CHECK(max_bytes >= 1 && max_bytes < (1ull << 31), SH_ERR_BAD_ARG, "sh_bam_scanner_create: windows of %llu bytes, 1 .. 2^31 - 1 are taken", (unsigned long long)max_bytes);
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || n_dev <= device) { sh_set_error("no HIP device %d", device); return SH_ERR_NO_DEVICE; }
    DeviceScope scope(device);
    SH_HIP(scope.err);
    sh_bam_scanner *sc = new sh_bam_scanner;
    sc->device = device; sc->max_bytes = max_bytes; sc->max_seg = (max_bytes + SHB_SEGMENT - 1) / SHB_SEGMENT;
    const uint64_t s = sc->max_seg;
    hipError_t e = hipSuccess;
    auto take = [&](void **p, uint64_t bytes) { if (e == hipSuccess) e = hipMalloc(p, bytes); };
    take((void **)&sc->d_cnt, s * 4); take((void **)&sc->d_tab_start, s * SHB_SEGMENT_CAP * 4); take((void **)&sc->d_tab_res, s * SHB_SEGMENT_CAP * 8);
    take((void **)&sc->d_entry, s * 4); take((void **)&sc->d_bytes, (s + 1) * 4); take((void **)&sc->d_off, (s + 1) * 8);
    take((void **)&sc->d_counts, sizeof(DevCounts)); take((void **)&sc->d_chain, sizeof(ChainOut));
    if (e == hipSuccess) e = rocprim::exclusive_scan(nullptr, sc->scan_tmp_bytes, sc->d_bytes, sc->d_off, 0ull, (size_t)(s + 1), rocprim::plus<unsigned long long>(), (hipStream_t) nullptr);
    take(&sc->d_scan_tmp, std::max<size_t>(sc->scan_tmp_bytes, 16));
    for (hipEvent_t &ev : sc->ev) if (e == hipSuccess) e = hipEventCreate(&ev);
    if (e != hipSuccess) {
        sh_set_error("sh_bam_scanner_create: scratch for windows of %llu bytes -> %s", (unsigned long long)max_bytes, hipGetErrorString(e));
        sh_bam_scanner_free(sc);
        return e == hipErrorOutOfMemory ? SH_ERR_OOM : SH_ERR_HIP;
    }
    *out = sc;
    return SH_OK;
}

extern "C" sh_status sh_bam_filter_device(sh_bam_scanner *sc, const uint8_t *d_text, uint64_t n, uint64_t base, uint64_t entry, int32_t last, const sh_bam_rule *rule,
                                          uint8_t *d_names, uint64_t names_cap, uint64_t *names_len, uint64_t *next_entry, void *stream, sh_bam_stats *stats)
{
    if (stats) memset(stats, 0, sizeof *stats);
    SH_CHECK(sc, SH_ERR_BAD_ARG, "sh_bam_filter_device: null argument");
    const sh_status ok = bam_check_args("sh_bam_filter_device", d_text, n, entry, rule, d_names, names_cap, names_len, next_entry);
    if (ok != SH_OK) return ok;
    SH_CHECK(n <= sc->max_bytes, SH_ERR_BAD_ARG, "sh_bam_filter_device: a window of %llu bytes, the scanner was made for %llu", (unsigned long long)n,
             (unsigned long long)sc->max_bytes);
    *names_len = 0; *next_entry = entry;
    if (entry == n) return SH_OK;
    const auto t0 = std::chrono::steady_clock::now();
    hipStream_t hs = (hipStream_t)stream;
    DeviceScope scope(sc->device);
    SH_HIP(scope.err);
    ShbRule r; memcpy(&r, rule, sizeof r);
    const uint32_t n32 = (uint32_t)n, n_seg = (uint32_t)((n + SHB_SEGMENT - 1) / SHB_SEGMENT);

    SH_HIP(hipMemsetAsync(sc->d_counts, 0, sizeof(DevCounts), hs));
    SH_HIP(hipMemsetAsync(sc->d_entry, 0xff, (size_t)n_seg * 4, hs));
    SH_HIP(hipEventRecord(sc->ev[0], hs));
    k_bam_probe<<<n_seg, 64, 0, hs>>>(d_text, n32, r.n_ref, sc->d_cnt, sc->d_tab_start, sc->d_tab_res, sc->d_counts);
    SH_HIP(hipGetLastError());
    SH_HIP(hipEventRecord(sc->ev[1], hs));

    // the chain; in front of an overflowed segment the host walks on to the first segment that has not overflowed
    struct Stretch { uint32_t seg; uint64_t at, len; };
    std::vector<Stretch> stretches;
    std::vector<uint8_t> h_names;
    ShbCounts hc{};
    uint64_t n_fallback = 0, pos = entry;
    bool have_host = false;
    for (;;) {
        k_bam_chain<<<1, 64, 0, hs>>>(n32, (uint32_t)pos, sc->d_cnt, sc->d_tab_start, sc->d_tab_res, sc->d_entry, sc->d_chain);
        SH_HIP(hipGetLastError());
        ChainOut co;
        SH_HIP(hipMemcpyAsync(&co, sc->d_chain, sizeof co, hipMemcpyDeviceToHost, hs));
        SH_HIP(hipStreamSynchronize(hs));
        pos = co.pos;
        int how = co.status == CHAIN_BROKEN ? SHB_WALK_BROKEN : co.status == CHAIN_OPEN ? SHB_WALK_OPEN : SHB_WALK_END;
        if (co.status == CHAIN_OVERFLOW) {
            if (!have_host) {
                sc->h_text.resize(n); sc->h_cnt.resize(n_seg);
                SH_HIP(hipMemcpyAsync(sc->h_text.data(), d_text, n, hipMemcpyDeviceToHost, hs));
                SH_HIP(hipMemcpyAsync(sc->h_cnt.data(), sc->d_cnt, (size_t)n_seg * 4, hipMemcpyDeviceToHost, hs));
                SH_HIP(hipStreamSynchronize(hs));
                have_host = true;
            }
            uint32_t seg = (uint32_t)(pos / SHB_SEGMENT), run_end = seg;
            while (run_end < n_seg && sc->h_cnt[run_end] > SHB_SEGMENT_CAP) ++run_end;
            n_fallback += run_end - seg;
            const uint64_t stop = std::min<uint64_t>((uint64_t)run_end * SHB_SEGMENT, n), at = h_names.size();
            h_names.resize(at + shb_names_bound(stop - pos) + 256);      // the records that lie in the stretch, and the one that leaves it
            uint64_t len = 0, last_seg = ~0ull, here = pos;
            how = shb_walk(ShbPtrSrc{sc->h_text.data()}, n, pos, stop, r, h_names.data() + at, h_names.size() - at, &len, &here, &hc, &last_seg);
            h_names.resize(at + len);
            SH_CHECK(how != SHB_WALK_CAP, SH_ERR_BAD_ARG, "sh_bam_filter_device: the names of the segments walked on the host leave their bound");
            stretches.push_back(Stretch{seg, at, len});
            pos = here;
            if (how == SHB_WALK_END && pos < n) continue;      // on with the tables
        }
        const sh_status end = bam_chain_end(how, pos, n, base, last);
        if (end != SH_OK) return end;
        break;
    }
    SH_HIP(hipEventRecord(sc->ev[2], hs));

    // count, scan, write
    k_bam_filter<<<n_seg, 64, 0, hs>>>(d_text, (uint32_t)pos, r, sc->d_entry, sc->d_bytes, sc->d_off, d_names, names_cap, sc->d_counts, 0);
    SH_HIP(hipGetLastError());
    SH_HIP(hipMemsetAsync(sc->d_bytes + n_seg, 0, 4, hs));
    for (const Stretch &s : stretches) {      // a stretch's names stand where its first segment's would
        const uint32_t len32 = (uint32_t)s.len;
        SH_HIP(hipMemcpyAsync(sc->d_bytes + s.seg, &len32, 4, hipMemcpyHostToDevice, hs));
        SH_HIP(hipStreamSynchronize(hs));
    }
    size_t tmp = sc->scan_tmp_bytes;
    SH_HIP(rocprim::exclusive_scan(sc->d_scan_tmp, tmp, sc->d_bytes, sc->d_off, 0ull, (size_t)n_seg + 1, rocprim::plus<unsigned long long>(), hs));
    unsigned long long total = 0;
    SH_HIP(hipMemcpyAsync(&total, sc->d_off + n_seg, 8, hipMemcpyDeviceToHost, hs));
    SH_HIP(hipStreamSynchronize(hs));
    SH_CHECK(total <= names_cap, SH_ERR_BAD_ARG, "sh_bam_filter_device: %llu name bytes, room for %llu", total, (unsigned long long)names_cap);
    k_bam_filter<<<n_seg, 64, 0, hs>>>(d_text, (uint32_t)pos, r, sc->d_entry, sc->d_bytes, sc->d_off, d_names, names_cap, sc->d_counts, 1);
    SH_HIP(hipGetLastError());
    for (const Stretch &s : stretches) {
        unsigned long long at = 0;
        SH_HIP(hipMemcpyAsync(&at, sc->d_off + s.seg, 8, hipMemcpyDeviceToHost, hs));
        SH_HIP(hipStreamSynchronize(hs));
        SH_CHECK(at + s.len <= names_cap, SH_ERR_BAD_ARG, "sh_bam_filter_device: %llu name bytes, room for %llu", at + (unsigned long long)s.len, (unsigned long long)names_cap);
        if (s.len) SH_HIP(hipMemcpyAsync(d_names + at, h_names.data() + s.at, s.len, hipMemcpyHostToDevice, hs));
        SH_HIP(hipStreamSynchronize(hs));
    }
    SH_HIP(hipEventRecord(sc->ev[3], hs));
    DevCounts dc;
    SH_HIP(hipMemcpyAsync(&dc, sc->d_counts, sizeof dc, hipMemcpyDeviceToHost, hs));
    SH_HIP(hipStreamSynchronize(hs));
    *names_len = total; *next_entry = pos;
    if (stats) {
        stats->n_records = dc.n_records + hc.n_records; stats->n_unmapped = dc.n_unmapped + hc.n_unmapped; stats->n_selected = dc.n_selected + hc.n_selected;
        stats->n_cg = dc.n_cg + hc.n_cg; stats->n_segments = dc.n_segments + hc.n_segments; stats->n_plausible = dc.n_plausible; stats->n_fallback_segments = n_fallback;
        stats->name_bytes = total;
        SH_HIP(hipEventElapsedTime(&stats->ms_probe, sc->ev[0], sc->ev[1]));
        SH_HIP(hipEventElapsedTime(&stats->ms_chain, sc->ev[1], sc->ev[2]));
        SH_HIP(hipEventElapsedTime(&stats->ms_filter, sc->ev[2], sc->ev[3]));
        stats->ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    return SH_OK;
}

// ---- the BAM reader of `scrubby alignment` (alignment_ids, sh_host.cpp) ---------------------------------------------------------------------
namespace {

constexpr uint64_t BAM_HOST_WINDOW = 16ull << 20;      // inflated bytes per call of the host path; grows for a longer record or header
constexpr uint64_t BAM_TEXT_BYTES = 160ull << 20;      // the device path's window of inflated bytes, the tail carried over included

void names_into(const uint8_t *names, uint64_t len, std::unordered_set<std::string> &ids)
{
    for (uint64_t i = 0; i < len;) {
        const char *s = (const char *)names + i;
        const size_t k = strnlen(s, len - i);
        ids.emplace(s, k);
        i += k + 1;
    }
}

sh_status bam_fail(const char *path, sh_status rc)
{
    const std::string why = sh_last_error();
    sh_set_error("%s: %s", path, why.c_str());
    return rc;
}

// zlib (shc::In) and sh_bam_filter_host, window by window
sh_status bam_ids_host(const char *path, sh_bam_rule rule, std::unordered_set<std::string> &ids)
{
    shc::In f;
    SH_CHECK(f.open(path), SH_ERR_IO, "cannot open %s", path);
    std::vector<uint8_t> win, names;
    uint64_t have = 0, base = 0;
    size_t want = BAM_HOST_WINDOW;
    bool eof = false, header = false;
    for (;;) {
        if (win.size() < want) win.resize(want);
        while (have < want && !eof) {
            const long got = f.read(win.data() + have, want - have);
            SH_CHECK(got >= 0, SH_ERR_IO, "cannot read %s: %s", path, f.error.c_str());
            if (got == 0) eof = true;
            have += (uint64_t)got;
        }
        uint64_t entry = 0;
        if (!header) {
            uint64_t first = 0;
            const int st = shb_header(ShbPtrSrc{win.data()}, have, &rule.n_ref, &first);
            SH_CHECK(st != SHB_HDR_NOT_BAM, SH_ERR_IO, "%s: not a BAM file", path);
            SH_CHECK(st == SHB_HDR_OK || !eof, SH_ERR_IO, "%s: truncated BAM header", path);
            if (st == SHB_HDR_MORE) { want *= 2; continue; }
            header = true; entry = first;
        }
        names.resize(shb_names_bound(have - entry));
        uint64_t len = 0, next = 0;
        const sh_status rc = sh_bam_filter_host(win.data(), have, base, entry, eof ? 1 : 0, &rule, names.data(), names.size(), &len, &next, nullptr);
        if (rc != SH_OK) return bam_fail(path, rc);
        names_into(names.data(), len, ids);
        if (eof) return SH_OK;
        if (next == 0) want *= 2;      // a record longer than the window
        memmove(win.data(), win.data() + next, have - next);
        have -= next; base += next;
    }
}

// Windows of the compressed file: sh_bgzf_scan, the members inflated into HBM behind the carried-over tail, sh_bam_filter_device, the
// names down.  *taken = false with *why / *why_off: the host path reads the file from its start (the ids are a set: what the device
// path added before stays right).
sh_status bam_ids_device(const char *path, sh_bam_rule rule, std::unordered_set<std::string> &ids, bool *taken, const char **why, uint64_t *why_off)
{
    *taken = false; *why = nullptr; *why_off = 0;
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev < 1) { *why = "no device"; return SH_OK; }
    FILE *fp = fopen(path, "rb");
    SH_CHECK(fp, SH_ERR_IO, "cannot open %s", path);
    struct Closer { FILE *f; ~Closer() { fclose(f); } } closer{fp};
    sh_inflater *inf = shc::gunzip_pool_acquire(0);
    if (!inf) { *why = "no device inflater"; return SH_OK; }
    struct Releaser { sh_inflater *inf; ~Releaser() { shc::gunzip_pool_release(inf); } } releaser{inf};
    sh_bam_scanner *sc = nullptr;
    if (sh_bam_scanner_create(0, BAM_TEXT_BYTES, &sc) != SH_OK) { *why = "no memory for the BAM scanner"; return SH_OK; }
    struct Freer { sh_bam_scanner *sc; ~Freer() { sh_bam_scanner_free(sc); } } freer{sc};
    DeviceScope scope(0);
    SH_HIP(scope.err);
    DevBuf d_text, d_names;
    const uint64_t names_cap = shb_names_bound(BAM_TEXT_BYTES);
    if (d_text.alloc(BAM_TEXT_BYTES + 64) != hipSuccess || d_names.alloc(names_cap) != hipSuccess) { *why = "no memory for the BAM window"; return SH_OK; }
    std::vector<uint8_t> win(shc::GUNZIP_WINDOW_BYTES), names, head;
    std::vector<sh_gz_member> members(shc::GUNZIP_READER_MEMBERS);
    uint64_t foff = 0, win_n = 0, have = 0, base = 0, n_windows = 0, n_records = 0, n_selected = 0, n_fallback = 0;
    bool eof = false, header = false;
    for (;;) {
        while (win_n < win.size() && !eof) {
            const size_t got = fread(win.data() + win_n, 1, win.size() - win_n, fp);
            if (got == 0) { SH_CHECK(!ferror(fp), SH_ERR_IO, "cannot read %s", path); eof = true; }
            win_n += got;
        }
        uint64_t n_m = 0, consumed = 0, k = 0, bytes = 0;
        const int stopped = shin_bgzf_scan(win.data(), win_n, (ShinMember *)members.data(), members.size(), &n_m, &consumed);
        while (k < n_m && have + bytes + members[k].out_len <= BAM_TEXT_BYTES) bytes += members[k++].out_len;
        if (k < n_m) consumed = members[k].file_off;
        *why_off = foff + consumed;
        if (k == n_m && stopped == 2 && consumed < win_n) { *why = "a gzip member that is not BGZF"; return SH_OK; }
        if (k == n_m && stopped == 1 && (eof || n_m == 0)) { *why = "a member that is cut short"; return SH_OK; }
        if (k == 0 && n_m > 0) { *why = header ? "a record above the scanner's size" : "a header that does not fit the first window"; return SH_OK; }
        for (uint64_t i = 0; i < k; ++i) members[i].file_off += foff;
        if (k) {
            const sh_status rc = shc::gunzip_window(inf, win.data(), members.data(), k, nullptr, d_text.as<uint8_t>() + have);
            if (rc != SH_OK) return bam_fail(path, rc);
        }
        have += bytes;
        memmove(win.data(), win.data() + consumed, win_n - consumed);
        win_n -= consumed; foff += consumed;
        const bool last = eof && win_n == 0;
        uint64_t entry = 0;
        if (!header) {
            int st = SHB_HDR_MORE;
            uint64_t first = 0;
            for (uint64_t h : {std::min<uint64_t>(have, 64u << 10), have}) {
                if (st != SHB_HDR_MORE) break;
                head.resize(h);
                if (h) SH_HIP(hipMemcpy(head.data(), d_text.p, h, hipMemcpyDeviceToHost));
                st = shb_header(ShbPtrSrc{head.data()}, h, &rule.n_ref, &first);
            }
            SH_CHECK(st != SHB_HDR_NOT_BAM, SH_ERR_IO, "%s: not a BAM file", path);
            SH_CHECK(st == SHB_HDR_OK || !last, SH_ERR_IO, "%s: truncated BAM header", path);
            if (st == SHB_HDR_MORE) continue;      // more members behind what is there; a full window ends at k == 0 above
            header = true; entry = first;
        }
        uint64_t len = 0, next = 0;
        sh_bam_stats st;
        const sh_status rc = sh_bam_filter_device(sc, d_text.as<uint8_t>(), have, base, entry, last ? 1 : 0, &rule, d_names.as<uint8_t>(), names_cap, &len, &next, nullptr, &st);
        if (rc != SH_OK) return bam_fail(path, rc);
        ++n_windows; n_records += st.n_records; n_selected += st.n_selected; n_fallback += st.n_fallback_segments;
        names.resize(len);
        if (len) SH_HIP(hipMemcpy(names.data(), d_names.p, len, hipMemcpyDeviceToHost));
        names_into(names.data(), len, ids);
        if (last) break;
        // the tail goes to the front, in pieces no longer than the distance it moves, so that no copy overlaps itself
        const uint64_t tail = have - next;
        for (uint64_t done = 0; next && done < tail;) {
            const uint64_t piece = std::min(tail - done, next);
            SH_HIP(hipMemcpy(d_text.as<uint8_t>() + done, d_text.as<uint8_t>() + next + done, piece, hipMemcpyDeviceToDevice));
            done += piece;
        }
        have = tail; base += next;
    }
    if (const char *e = getenv("SCRUBBY_HIP_DBG_HOST")) if (*e == '1')
        fprintf(stderr, "[scrubby-hip] BAM on the device: %llu windows, %llu records, %llu selected, %llu segments walked on the host\n", (unsigned long long)n_windows,
                (unsigned long long)n_records, (unsigned long long)n_selected, (unsigned long long)n_fallback);
    *taken = true;
    return SH_OK;
}

}      // namespace

sh_status shi_bam_ids(const char *path, uint64_t min_len, double min_cov, uint32_t min_mapq, std::unordered_set<std::string> &ids)
{
    const sh_bam_rule rule{min_len, min_cov, min_mapq, 0};
    if (shc::gunzip_device_wanted()) {
        bool taken = false;
        const char *why = nullptr;
        uint64_t why_off = 0;
        const sh_status rc = bam_ids_device(path, rule, ids, &taken, &why, &why_off);
        if (rc != SH_OK) return rc;
        if (taken) return SH_OK;
        shc::gunzip_note_zlib(path, why_off, why);
    }
    return bam_ids_host(path, rule, ids);
}
