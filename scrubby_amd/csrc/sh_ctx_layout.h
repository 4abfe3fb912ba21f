// sh_ctx_layout.h — what sh_ctx_create (sh_classify.hip) works out before it allocates: the capacities of a classify context and the layout
// of every allocation that holds more than one array, each written once.  Host only: no HIP (tests/ctx_layout_host.cpp builds it with g++).
//   Carve        walks an allocation in 256-byte-aligned steps.  Without a base it hands out null pointers and only counts, with one it
//                places: a layout routine is run once to size the hipMalloc and once more to set the pointers.
//   ctx_caps     the capacities, from sh_ctx_create's arguments and the two switches that override them.
//   *_layout     the arrays of the arena's repeat-path slice (BigBufs), of the long-read front end (d_long) and of the extension stage's
//                chain hand-over (d_ext).  Templates over the struct that holds the pointers, so that the device headers stay out of here;
//                the sizes of their element types come in as CtxElem.
#pragma once
#include "sh_switches.h"
#include <algorithm>
#include <cstdint>
#include <vector>

struct Carve {
    uint8_t *base = nullptr;
    uint64_t off = 0;                            // bytes handed out so far
    std::vector<uint64_t> *sizes = nullptr;      // tests: every size asked for, in order
    static constexpr uint64_t al(uint64_t b) { return (b + 255) & ~255ull; }
    template <class T> void take(T *&dst, uint64_t bytes)
    {
        dst = base ? (T *)(base + off) : nullptr;
        off += al(bytes);
        if (sizes) sizes->push_back(bytes);
    }
};

// sizeof of ChainRec, SortItem, BigMeta, BigTables (sh_align.h, sh_classify.hip)
struct CtxElem { uint64_t chain_rec, sort_item, big_meta, big_tables; };
// N_SORT_CLS, SINK_SHARDS, LSEG, GT of the device headers: sh_classify.hip asserts it
constexpr int CL_SORT_CLS = 6;
constexpr uint64_t CL_SINK_SHARDS = 64, CL_LSEG = 256, CL_GT = 2048;

inline bool w_supported(int w) { return w == 5 || w == 10 || w == 11 || w == 19; }

struct CtxCaps {
    bool use_k1, use_long, ext, ext_long;
    uint64_t n_tiles, arena_bytes, legacy_bytes;
    uint64_t sort_cap[CL_SORT_CLS], anchor_cap;      // anchor_cap < 1024: the arena is too small
    uint64_t max_segs, mz_cap;                       // use_long
    uint64_t cap_recs, cap_anch, larena_bytes;       // ext: per shard of the chain sink; ext_long: the chains between the two kernels
};

inline CtxCaps ctx_caps(uint64_t max_reads, uint64_t max_bases, uint32_t max_read_len, int k, int w, bool cigar, bool is_sr,
                        int64_t sw_arena_bytes, int64_t sw_ext_bytes, const CtxElem &z)
{
    CtxCaps c{};
    c.ext = cigar;
    c.ext_long = cigar && !is_sr;
    // K1 stages a tile of 64 reads in LDS; it needs k <= 23 (hash and position share 64 bits),
    // read positions < 2^17 and a supported compile-time window
    c.use_k1 = k <= 23 && max_read_len <= 1024 && w_supported(w);
    c.use_long = !c.use_k1 && w_supported(w);      // the long-read front end feeds the repeat path
    c.n_tiles = (max_reads + 63) / 64;
    // arena: anchors (+ sort buffer) and DP state of reads with > 64 anchors (36 B per anchor slot) + a slice for
    // the legacy re-sketch path.  Default 4 KiB per read of the batch (~110 anchor slots per read; the CHM13-sized
    // workload averages 72), at least 4 GiB; reads that find no room are deferred and re-run.
    c.arena_bytes = std::max<uint64_t>(4ull << 30, max_reads * 4096ull);      // floor: a small batch still meets reads with 10^5 anchors (4 MB each); a starved arena means deferral rounds of ~1.5 ms
    // without K1 every read takes the legacy path, whose sketch buffers and anchors live in the arena: ~48 B per base
    if (!c.use_k1) c.arena_bytes = std::max<uint64_t>(c.arena_bytes, std::min<uint64_t>(max_reads * (uint64_t)max_read_len * 48ull, (c.ext_long ? 32ull : 64ull) << 30));      // long-read presets with the extension filter: the raw anchors have their own buffer (d_stage_*)
    if (sw_arena_bytes != SW_UNSET) c.arena_bytes = (uint64_t)sw_arena_bytes;
    {
        const uint64_t big_min = (64ull << 20) + max_reads * 160;
        c.legacy_bytes = (c.use_k1 || c.use_long) ? std::min<uint64_t>(c.arena_bytes / 8, 1ull << 30)
                                                  : (c.arena_bytes > 2 * big_min ? c.arena_bytes - big_min : c.arena_bytes / 2);
        const uint64_t left = c.arena_bytes - c.legacy_bytes;
        // k_expand's waves reserve sort-list entries in chunks (<= 32): up to one abandoned chunk per wave and class
        const uint64_t waves = 3 * std::min<uint64_t>(std::max<uint64_t>(c.n_tiles, 1), 256 * 8);      // k_expand's grid (big_pass)
        const uint64_t sort_cap[CL_SORT_CLS] = {max_reads + 32 * waves, max_reads + 32 * waves, max_reads + 8 * waves, max_reads + 8 * waves, max_reads + waves, max_reads + waves};
        uint64_t sort_cap_sum = 0;
        for (int i = 0; i < CL_SORT_CLS; ++i) sort_cap_sum += c.sort_cap[i] = sort_cap[i];
        // anchor slots: what the arrays that do not grow with them leave, over the bytes of one slot.  big_layout below is what places them;
        // sh_ctx_create runs it in count mode to see that it fits
        const uint64_t fixed = 4 * 64 * z.sort_item + 4096 + max_reads * (z.big_meta + 8 + 16) + sort_cap_sum * z.sort_item + sort_cap[CL_SORT_CLS - 1] * 4 + 16384;
        const uint64_t per_anchor = 8 + 8 + 8 + 4 + 4 + 4 + 2 + (c.ext ? 8 + 3 : 0);   // ax bx az aq bq af (+ tile_split and cluster queue shares) (+ hz)
        c.anchor_cap = (left > fixed ? (left - fixed) / per_anchor : 0) & ~15ull;
    }
    if (c.use_long) {
        const uint64_t cb = std::min<uint64_t>(max_bases + 64, max_reads * (uint64_t)max_read_len + 64);     // bases of one chunk, at most
        c.max_segs = cb / CL_LSEG + max_reads + 2;
        c.mz_cap = cb * 5 / (2 * ((uint64_t)w + 1)) + 4096;   // minimizer density is ~2/(w+1), + 25 %; reads beyond the cap take the legacy path
    }
    if (c.ext) {
        // chain hand-over: 32-B records, 12 B per chain anchor, one list head per read; sized for ~2 chains and ~32 chain anchors per
        // read of the chunk (a chunk that needs more is cut in two and re-run: classify_chunk returns SH_SPLIT)
        uint64_t cap_recs = std::max<uint64_t>(1ull << 20, 2 * max_reads), cap_anch = std::max<uint64_t>(1ull << 24, 32 * max_reads);
        if (c.ext_long) {      // a long read's chains hold most of its minimizers (~2 / (w + 1) per base), secondary chains as many again
            // bases of one chunk: max_bases may describe a whole batch of many chunks; ~8 kb per read is what long-read sets average - a
            // chunk that holds more is cut in two when its chains do not fit (SH_SPLIT)
            const uint64_t cb = std::min<uint64_t>({max_bases + 64, max_reads * (uint64_t)max_read_len + 64, max_reads * 8192ull + (64ull << 20)});
            // flag-only calls hand over the chains of the loci that can hold regs[0] (k_lr_locus: ~100 chain anchors and a dozen chains per read
            // of the bench workload); a call with a trace hands over every chain (thousands of anchors, hundreds of chains per read) and is
            // cut into smaller chunks when they do not fit
            cap_anch = std::max<uint64_t>(cap_anch, cb / 8);
            cap_recs = std::max<uint64_t>(cap_recs, std::min<uint64_t>(cb / 64, 1ull << 28) + 8 * max_reads);
        }
        if (sw_ext_bytes != SW_UNSET) { cap_anch = std::max<uint64_t>(1 << 16, (uint64_t)sw_ext_bytes / 16); cap_recs = std::max<uint64_t>(1 << 12, cap_anch / 16); }
        c.cap_recs = std::min<uint64_t>((cap_recs + CL_SINK_SHARDS - 1) / CL_SINK_SHARDS, 0xfffffff0ull / CL_SINK_SHARDS);      // per shard
        c.cap_anch = (cap_anch + CL_SINK_SHARDS - 1) / CL_SINK_SHARDS;
        // the chains between the two kernels of the long-read stage: what the hand-over buffers can hold, twice (the long join re-orders, it
        // adds nothing; a read with one chain kept may leave that chain beside the join's outcome: lr_chains_wave, `both`)
        if (c.ext_long) c.larena_bytes = CL_SINK_SHARDS * c.cap_anch * 32 + CL_SINK_SHARDS * c.cap_recs * 12 + max_reads * 48 + (1ull << 20);
    }
    return c;
}

// k_expand's raw anchors wait here for k_lr_locus (12 B each; ~1.1 anchors per base on a repeat-rich reference); reads that find no room
// come back in the pass's next iteration.  The last of the context's allocations: at most 45 % of what the device still has (`free_bytes`;
// 0 when it could not be asked) - a million-read context fits that way: its launches pay the stage's longest reads once where two
// half-size ones pay them twice; what finds no room is deferred
inline uint64_t ctx_stage_cap(uint64_t max_reads, uint64_t max_bases, uint32_t max_read_len, bool have_free, uint64_t free_bytes, int64_t sw_stage_bytes)
{
    const uint64_t cb = std::min<uint64_t>({max_bases + 64, max_reads * (uint64_t)max_read_len + 64, max_reads * 8192ull + (64ull << 20)});
    uint64_t cap = std::min<uint64_t>(cb + cb / 4 + (1ull << 20), (64ull << 30) / 12);
    if (have_free) cap = std::min<uint64_t>(cap, std::max<uint64_t>(1ull << 20, (uint64_t)((double)free_bytes * 0.45) / 12));
    if (sw_stage_bytes != SW_UNSET) cap = std::max<uint64_t>(1ull << 16, (uint64_t)sw_stage_bytes / 12);
    return cap;
}

// BigBufs: the repeat path's slice of the arena, behind the legacy slice
template <class B> inline void big_layout(Carve &cv, B &b, const CtxCaps &k, uint64_t max_reads, const CtxElem &z)
{
    const uint64_t cap = b.anchor_cap = k.anchor_cap;
    cv.take(b.ax, cap * 8); cv.take(b.bx, cap * 8); cv.take(b.az, cap * 8);
    cv.take(b.aq, cap * 4); cv.take(b.bq, cap * 4);
    cv.take(b.af, cap * 4);
    if (k.ext) cv.take(b.hz, cap * 8); else b.hz = nullptr;
    cv.take(b.meta, max_reads * z.big_meta);
    cv.take(b.acc_nu, max_reads * 4); cv.take(b.acc_best, max_reads * 4);
    for (int i = 0; i < CL_SORT_CLS; ++i) cv.take(b.sort_items[i], k.sort_cap[i] * z.sort_item);
    cv.take(b.tile_base, (max_reads + 1) * 4);
    cv.take(b.giant_order, k.sort_cap[CL_SORT_CLS - 1] * 4);
    cv.take(b.tile_split, (cap / CL_GT + max_reads + 2) * 12);      // three words per tile
    const uint64_t div[4] = {4096, 1024, 256, k.ext ? 8u : 64u};      // a cluster of class c has more than {4096, 1024, 256, 64} anchors
    for (int i = 0; i < 4; ++i) { b.cl_cap[i] = (uint32_t)std::min<uint64_t>(cap / div[i] + 64, UINT32_MAX); cv.take(b.cl_items[i], (uint64_t)b.cl_cap[i] * z.sort_item); }
    cv.take(b.tabs, z.big_tables);
}

// d_long: segment table, minimizers and seed records of the long-read front end
template <class C> inline void long_layout(Carve &cv, C &c, const CtxCaps &k, uint64_t max_reads)
{
    cv.take(c.d_seg_base, (max_reads + 1) * 4); cv.take(c.d_seg_cnt, k.max_segs * 4);
    cv.take(c.d_seg_off, (k.max_segs + 1) * 8); cv.take(c.d_scan_tot, (k.max_segs / 16384 + 2) * 8); cv.take(c.d_mz_hash, k.mz_cap * 8);
    cv.take(c.d_mz_y, k.mz_cap * 4); cv.take(c.d_lrec, k.mz_cap * 16); cv.take(c.d_seed_off, max_reads * 8);
}

// d_ext: the chain sink's shards and the per-read lists of the extension stage
template <class C> inline void ext_layout(Carve &cv, C &c, const CtxCaps &k, uint64_t max_reads, const CtxElem &z)
{
    cv.take(c.sink.recs, CL_SINK_SHARDS * k.cap_recs * z.chain_rec);
    cv.take(c.sink.cx, CL_SINK_SHARDS * k.cap_anch * 8); cv.take(c.sink.cq, CL_SINK_SHARDS * k.cap_anch * 4);
    cv.take(c.sink.head, max_reads * 4);
    cv.take(c.d_ext_list, max_reads * 4);
    cv.take(c.d_ext_redo, max_reads * 4);
    if (!k.ext_long) { cv.take(c.d_ext_unres[0], max_reads * 4); cv.take(c.d_ext_unres[1], max_reads * 4); }
    cv.take(c.sink.best, max_reads * 8);
    cv.take(c.sink.tie, max_reads * 4);
}
