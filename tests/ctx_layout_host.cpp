// The sizes and layouts of a classify context's device memory (scrubby_amd/csrc/sh_ctx_layout.h) on the host: no HIP, plain g++.
// For every combination of the inputs below: count mode and place mode of each layout ask for the same sizes in the same order and place
// mode ends at the counted total; every array is 256-byte aligned, inside the allocation and apart from the others (placed over a block of
// exactly the counted size, first and last byte of every array written: under AddressSanitizer that is the check of the extents); the
// capacities and totals equal the closed forms sh_ctx_create held before the layouts were written once (restated below); and the arena's
// layout fits what the arena leaves it whenever there are 1024 anchor slots.
// tests/test_ctx_layout_cpu.py builds this with -DCTX_LAYOUT_MAIN and the sanitizers and runs it as a program of its own.
#include "../scrubby_amd/csrc/sh_ctx_layout.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <set>

namespace {

// stand-ins for the element types of the device headers, of the same sizes
struct Rec { uint32_t next, cnt; int32_t score; uint32_t key_f, key_i, yfl; unsigned long long off, z; };
struct Item { uint32_t w, n, qlen, pad; unsigned long long off; };
struct Meta { uint32_t r, n_a; int32_t rep_len; uint32_t state; };
struct Tabs { Item *sort_items[CL_SORT_CLS]; Item *cl_items[4]; uint32_t cl_cap[4]; };
struct U4 { uint32_t x, y, z, w; };
const CtxElem ELEM = {sizeof(Rec), sizeof(Item), sizeof(Meta), sizeof(Tabs)};

struct Big {
    uint64_t *ax, *bx, *az; uint32_t *aq, *bq; int32_t *af; uint64_t *hz; unsigned long long anchor_cap;
    Meta *meta; int32_t *acc_nu, *acc_best; Item *sort_items[CL_SORT_CLS]; uint32_t *tile_base, *tile_split, *giant_order;
    Item *cl_items[4]; uint32_t cl_cap[4]; const Tabs *tabs;
};
struct Ctx {
    uint32_t *d_seg_base, *d_seg_cnt, *d_mz_y; unsigned long long *d_seg_off, *d_seed_off, *d_scan_tot; uint64_t *d_mz_hash; U4 *d_lrec;
    struct { Rec *recs; uint64_t *cx; uint32_t *cq, *head; unsigned long long *best; uint32_t *tie; } sink;
    uint32_t *d_ext_list, *d_ext_redo, *d_ext_unres[2];
};

int g_line = 0;
#define CHECK(c) do { if (!(c)) { if (!g_line) g_line = __LINE__; return false; } } while (0)

const uint64_t BLOCK_MAX = 1ull << 30;
long long n_layouts = 0, n_skipped = 0, n_repeats = 0;
std::set<std::vector<uint64_t>> g_placed;

// One layout (id: 0 arena, 1 long-read front end, 2 hand-over) in both modes.  `arrays` lists the struct's pointers in the order the layout takes them.
template <class F, class P> bool both_modes(int id, F layout, P arrays, uint64_t *total_out)
{
    std::vector<uint64_t> asked0, asked1;
    Carve count;
    count.sizes = &asked0;
    layout(count);
    *total_out = count.off;
    ++n_layouts;
    if (count.off > BLOCK_MAX) { ++n_skipped; return true; }
    // many combinations differ only in inputs a layout does not read: a sequence of sizes that has been placed and checked is not placed
    // again (the sanitizer's book-keeping for a block of hundreds of MB is what this program's time goes to)
    std::vector<uint64_t> key = asked0;
    key.push_back((uint64_t)id);
    if (!g_placed.insert(key).second) { ++n_repeats; return true; }
    CHECK(count.off > 0 && count.off % 256 == 0);
    uint8_t *block = (uint8_t *)aligned_alloc(256, count.off);
    CHECK(block != nullptr);
    Carve place;
    place.base = block; place.sizes = &asked1;
    layout(place);
    bool ok = asked0 == asked1 && place.off == count.off && count.off % 256 == 0;
    std::vector<const uint8_t *> ptr = arrays();
    ok = ok && ptr.size() == asked1.size();
    const uint8_t *prev_end = block;
    for (size_t i = 0; ok && i < ptr.size(); ++i) {
        uint8_t *p = (uint8_t *)ptr[i];
        ok = p != nullptr && (uintptr_t)(p - block) % 256 == 0 && p >= prev_end && (uint64_t)(p - block) + asked1[i] <= count.off;
        if (ok && asked1[i]) { p[0] = 1; p[asked1[i] - 1] = 2; }
        prev_end = p + asked1[i];
    }
    free(block);
    CHECK(ok);
    return true;
}

bool one(uint64_t max_reads, uint32_t max_read_len, int mode, int w, int64_t sw_arena, int64_t sw_ext, int64_t sw_stage)
{
    const int k = 15;
    const bool cigar = mode != 0, is_sr = mode != 2;
    const uint64_t max_bases = max_reads * (uint64_t)max_read_len;
    const CtxCaps K = ctx_caps(max_reads, max_bases, max_read_len, k, w, cigar, is_sr, sw_arena, sw_ext, ELEM);

    // ---- sh_ctx_create of commit 2dac421 (the parent of the change that introduced sh_ctx_layout.h), restated: its names, its expressions ----
    struct { bool ext, ext_long, use_k1, use_long; uint64_t arena_bytes, legacy_bytes, max_segs, mz_cap, long_bytes, ext_bytes, stage_cap; unsigned long long larena_bytes; } c{};
    struct { int64_t arena_bytes, ext_bytes, stage_bytes; } sw = {sw_arena, sw_ext, sw_stage};
    struct { int w; } opts_v = {w}, *opts = &opts_v;
    using SortItem = Item; using BigMeta = Meta; using ChainRec = Rec;
    const int N_SORT_CLS = 6; const uint64_t SINK_SHARDS = 64, LSEG = 256u;
    uint64_t old_cap = 0, old_cap_recs = 0, old_cap_anch = 0;
    auto w_supported = [](int w) { return w == 5 || w == 10 || w == 11 || w == 19; };      // (its own copy: hides the header's)
    c.ext = cigar;
    c.ext_long = c.ext && !is_sr;
    c.use_k1 = k <= 23 && max_read_len <= 1024 && w_supported(opts->w);
    const uint64_t n_tiles = (max_reads + 63) / 64;
    c.arena_bytes = std::max<uint64_t>(4ull << 30, max_reads * 4096ull);
    if (!c.use_k1) c.arena_bytes = std::max<uint64_t>(c.arena_bytes, std::min<uint64_t>(max_reads * (uint64_t)max_read_len * 48ull, (c.ext_long ? 32ull : 64ull) << 30));
    if (sw.arena_bytes != SW_UNSET) c.arena_bytes = (uint64_t)sw.arena_bytes;
    uint64_t old_sort_cap[6];
    {
        const uint64_t big_min = (64ull << 20) + max_reads * 160;
        const bool long_fe = !c.use_k1 && w_supported(opts->w);
        c.legacy_bytes = (c.use_k1 || long_fe) ? std::min<uint64_t>(c.arena_bytes / 8, 1ull << 30)
                                               : (c.arena_bytes > 2 * big_min ? c.arena_bytes - big_min : c.arena_bytes / 2);
        uint64_t left = c.arena_bytes - c.legacy_bytes;
        const uint64_t waves = 3 * std::min<uint64_t>(std::max<uint64_t>(n_tiles, 1), 256 * 8);
        const uint64_t sort_cap[N_SORT_CLS] = {max_reads + 32 * waves, max_reads + 32 * waves, max_reads + 8 * waves, max_reads + 8 * waves, max_reads + waves, max_reads + waves};
        uint64_t sort_cap_sum = 0;
        for (int i = 0; i < N_SORT_CLS; ++i) sort_cap_sum += sort_cap[i];
        uint64_t fixed = 4 * 64 * sizeof(SortItem) + 4096 + max_reads * (sizeof(BigMeta) + 8 + 16) + sort_cap_sum * sizeof(SortItem) + sort_cap[N_SORT_CLS - 1] * 4 + 16384;
        uint64_t per_anchor = 8 + 8 + 8 + 4 + 4 + 4 + 2 + (c.ext ? 8 + 3 : 0);
        uint64_t cap = left > fixed ? (left - fixed) / per_anchor : 0;
        cap &= ~15ull;
        old_cap = cap;
        for (int i = 0; i < N_SORT_CLS; ++i) old_sort_cap[i] = sort_cap[i];
    }
    c.use_long = !c.use_k1 && w_supported(opts->w);
    if (c.use_long) {
        const uint64_t cb = std::min<uint64_t>(max_bases + 64, max_reads * (uint64_t)max_read_len + 64);
        c.max_segs = cb / LSEG + max_reads + 2;
        c.mz_cap = cb * 5 / (2 * ((uint64_t)opts->w + 1)) + 4096;
        auto al = [](uint64_t b) { return (b + 255) & ~255ull; };
        c.long_bytes = al((max_reads + 1) * 4) + al(c.max_segs * 4) + al((c.max_segs + 1) * 8) + al((c.max_segs / 16384 + 2) * 8) + al(c.mz_cap * 8) + al(c.mz_cap * 4) + al(c.mz_cap * 16) + al(max_reads * 8);
    }
    if (c.ext) {
        uint64_t cap_recs = std::max<uint64_t>(1ull << 20, 2 * max_reads), cap_anch = std::max<uint64_t>(1ull << 24, 32 * max_reads);
        if (c.ext_long) {
            const uint64_t cb = std::min<uint64_t>({max_bases + 64, max_reads * (uint64_t)max_read_len + 64, max_reads * 8192ull + (64ull << 20)});
            cap_anch = std::max<uint64_t>(cap_anch, cb / 8);
            cap_recs = std::max<uint64_t>(cap_recs, std::min<uint64_t>(cb / 64, 1ull << 28) + 8 * max_reads);
        }
        if (sw.ext_bytes != SW_UNSET) { cap_anch = std::max<uint64_t>(1 << 16, (uint64_t)sw.ext_bytes / 16); cap_recs = std::max<uint64_t>(1 << 12, cap_anch / 16); }
        cap_recs = std::min<uint64_t>((cap_recs + SINK_SHARDS - 1) / SINK_SHARDS, 0xfffffff0ull / SINK_SHARDS);
        cap_anch = (cap_anch + SINK_SHARDS - 1) / SINK_SHARDS;
        auto al = [](uint64_t b) { return (b + 255) & ~255ull; };
        c.ext_bytes = al(SINK_SHARDS * cap_recs * sizeof(ChainRec)) + al(SINK_SHARDS * cap_anch * 8) + al(SINK_SHARDS * cap_anch * 4) + 3 * al(max_reads * 4) + al(max_reads * 8) + al(max_reads * 4) + (c.ext_long ? 0 : 2 * al(max_reads * 4));
        old_cap_recs = cap_recs; old_cap_anch = cap_anch;
        if (c.ext_long) {
            c.larena_bytes = SINK_SHARDS * cap_anch * 32 + SINK_SHARDS * cap_recs * 12 + max_reads * 48 + (1ull << 20);
            // what hipMemGetInfo says at that point: plenty (the 64 GiB ceiling binds), 1 GiB and 8 MiB (the 45 % and its 2^20 floor bind), or nothing
            for (int64_t free_bytes : {(int64_t)200 << 30, (int64_t)1 << 30, (int64_t)8 << 20, (int64_t)-1}) {
                const bool info_ok = free_bytes >= 0;
                const uint64_t cb = std::min<uint64_t>({max_bases + 64, max_reads * (uint64_t)max_read_len + 64, max_reads * 8192ull + (64ull << 20)});
                c.stage_cap = std::min<uint64_t>(cb + cb / 4 + (1ull << 20), (64ull << 30) / 12);
                {
                    size_t fr = info_ok ? (size_t)free_bytes : 0;
                    if (info_ok) c.stage_cap = std::min<uint64_t>(c.stage_cap, std::max<uint64_t>(1ull << 20, (uint64_t)((double)fr * 0.45) / 12));
                }
                if (sw.stage_bytes != SW_UNSET) c.stage_cap = std::max<uint64_t>(1ull << 16, (uint64_t)sw.stage_bytes / 12);
                CHECK(ctx_stage_cap(max_reads, max_bases, max_read_len, info_ok, info_ok ? (uint64_t)free_bytes : 0, sw_stage) == c.stage_cap);
            }
        }
    }
    // ---- end of the restatement ----

    CHECK(K.ext == c.ext && K.ext_long == c.ext_long && K.use_k1 == c.use_k1 && K.use_long == c.use_long && K.n_tiles == n_tiles);
    CHECK(K.arena_bytes == c.arena_bytes && K.legacy_bytes == c.legacy_bytes);
    CHECK(K.anchor_cap == old_cap);
    for (int i = 0; i < CL_SORT_CLS; ++i) CHECK(K.sort_cap[i] == old_sort_cap[i]);
    CHECK(K.max_segs == c.max_segs && K.mz_cap == c.mz_cap);
    CHECK(K.cap_recs == old_cap_recs && K.cap_anch == old_cap_anch && K.larena_bytes == c.larena_bytes);

    uint64_t total = 0;
    if (K.anchor_cap >= 1024) {
        Big b{};
        CHECK(both_modes(0, [&](Carve &cv) { big_layout(cv, b, K, max_reads, ELEM); }, [&]() {
            std::vector<const uint8_t *> v = {(uint8_t *)b.ax, (uint8_t *)b.bx, (uint8_t *)b.az, (uint8_t *)b.aq, (uint8_t *)b.bq, (uint8_t *)b.af};
            if (K.ext) v.push_back((uint8_t *)b.hz);
            for (void *p : {(void *)b.meta, (void *)b.acc_nu, (void *)b.acc_best}) v.push_back((uint8_t *)p);
            for (Item *p : b.sort_items) v.push_back((uint8_t *)p);
            for (void *p : {(void *)b.tile_base, (void *)b.giant_order, (void *)b.tile_split}) v.push_back((uint8_t *)p);
            for (Item *p : b.cl_items) v.push_back((uint8_t *)p);
            v.push_back((const uint8_t *)b.tabs);
            return v; }, &total));
        CHECK(total <= K.arena_bytes - K.legacy_bytes);      // what "internal arena carve overflow" guarded at run time
        CHECK(b.anchor_cap == old_cap && (K.ext || b.hz == nullptr));
        const uint64_t div[4] = {4096, 1024, 256, c.ext ? 8u : 64u};
        for (int i = 0; i < 4; ++i) CHECK(b.cl_cap[i] == (uint32_t)std::min<uint64_t>(old_cap / div[i] + 64, UINT32_MAX));
    }
    Ctx x{};
    if (K.use_long) {
        CHECK(both_modes(1, [&](Carve &cv) { long_layout(cv, x, K, max_reads); }, [&]() {
            return std::vector<const uint8_t *>{(uint8_t *)x.d_seg_base, (uint8_t *)x.d_seg_cnt, (uint8_t *)x.d_seg_off, (uint8_t *)x.d_scan_tot, (uint8_t *)x.d_mz_hash,
                                                (uint8_t *)x.d_mz_y, (uint8_t *)x.d_lrec, (uint8_t *)x.d_seed_off}; }, &total));
        CHECK(total == c.long_bytes);
    }
    if (K.ext) {
        CHECK(both_modes(2, [&](Carve &cv) { ext_layout(cv, x, K, max_reads, ELEM); }, [&]() {
            std::vector<const uint8_t *> v = {(uint8_t *)x.sink.recs, (uint8_t *)x.sink.cx, (uint8_t *)x.sink.cq, (uint8_t *)x.sink.head, (uint8_t *)x.d_ext_list, (uint8_t *)x.d_ext_redo};
            if (!K.ext_long) { v.push_back((uint8_t *)x.d_ext_unres[0]); v.push_back((uint8_t *)x.d_ext_unres[1]); }
            v.push_back((uint8_t *)x.sink.best); v.push_back((uint8_t *)x.sink.tie);
            return v; }, &total));
        CHECK(total == c.ext_bytes);
    }
    return true;
}

// 0 when every combination holds, else the line of the first check that failed; counts: combinations, layouts run, layouts skipped for their size
int ctxl_run(long long *counts)
{
    long long n = 0;
    for (uint64_t max_reads : {1ull, 63ull, 64ull, 65ull, 4096ull, 1ull << 22})
        for (uint32_t max_read_len : {1u, 150u, 1024u, 1025u, 50000u})
            for (int mode = 0; mode < 3; ++mode)      // flag-only, SH_F_CIGAR short reads, SH_F_CIGAR long reads
                for (int w : {5, 11, 19})
                    for (int64_t arena : {(int64_t)8 << 20, (int64_t)96 << 20, SW_UNSET})
                        for (int over = 0; over < 2; ++over) {      // SCRUBBY_HIP_EXT_MB=64 and SCRUBBY_HIP_STAGE_MB=16, or neither
                            ++n;
                            if (!one(max_reads, max_read_len, mode, w, arena, over ? (int64_t)64 << 20 : SW_UNSET, over ? (int64_t)16 << 20 : SW_UNSET)) {
                                fprintf(stderr, "max_reads %llu, max_read_len %u, mode %d, w %d, arena %lld, overrides %d: check in line %d\n",
                                        (unsigned long long)max_reads, max_read_len, mode, w, (long long)arena, over, g_line);
                                return g_line;
                            }
                        }
    counts[0] = n; counts[1] = n_layouts; counts[2] = n_skipped;
    return 0;
}

}      // namespace

#ifdef CTX_LAYOUT_MAIN
int main()
{
    long long counts[3] = {0, 0, 0};
    const int rc = ctxl_run(counts);
    if (rc) return 1;
    printf("%lld combinations, %lld layouts, %lld skipped (more than 1 GiB), %lld placed before with the same sizes\n", counts[0], counts[1], counts[2], n_repeats);
    if (counts[2] * 4 > counts[1]) { printf("more than a quarter of the layouts were skipped\n"); return 1; }
    // Sequences of sizes that must differ, and so be placed each: the arena of 96 MiB for the five max_reads whose fixed part it holds, with
    // and without hz (10); the hand-over under EXT_MB for six max_reads, short and long reads (12); the long-read front end at 1025 bases
    // for the five max_reads that stay under 1 GiB and three w (15)
    const long long placed = counts[1] - counts[2] - n_repeats;
    printf("%lld layouts placed\n", placed);
    if (placed < 37) { printf("fewer distinct layouts were placed than the inputs hold\n"); return 1; }
    printf("ok\n");
    return 0;
}
#endif
