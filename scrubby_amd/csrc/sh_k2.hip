// sh_k2.hip — Kraken2-style taxid classifier on MI355X (BASELINE configs[4]).
//
// Replaces the external `kraken2` process of Cleaner::run_kraken (/root/reference/src/cleaner.rs:288-330).
// HBM layout: the compact hash table is one array of 32-bit cells (high 32 - value_bits bits = truncated hash,
// low value_bits bits = internal taxid, value 0 = empty), the taxonomy two u32 arrays (parent, external id).
//
// k_k2_classify: one lane per read / pair, 64 units per wave.
//   scan     rolling forward / reverse-complement l-mers, canonical, spaced-seed mask, toggle; the window minimum over
//            the k-l+1 most recent candidates lives in registers (W = 5 for k = 35, l = 31);
//   runs     consecutive k-mers with the same minimizer form one run = one table probe worth `len` k-mer counts;
//            runs queue up per lane in LDS and the whole wave drains its queues together, four probes in flight
//            per lane, so the random 4-B gathers overlap instead of stalling the scan one at a time;
//   resolve  per-lane hit list in LDS (<= HCAP distinct taxa; the rare unit beyond that is redone by the same kernel
//            with its list in HBM), ResolveTree over BFS-ordered parent links.
// Three compile-time switches, off in the default instance (which compiles to the code it had before they existed):
//   QMASK    kraken2 --minimum-base-quality: quality words ride beside the base words, a base whose Phred score is below
//            the threshold enters the scanner as a non-ACGT code (kraken2 masks it to 'x'); quality byte 0xFF = never masked;
//   QUICK    kraken2 --quick: pass 2 of the drain walks each lane's runs in read order and stops the unit at the first hit
//            run that brings the hit groups to the threshold (its taxon is the call, no hit list, no ResolveTree); the wave
//            leaves the character loop once every lane has stopped or read its last character;
//   HITS     kraken2's per-k-mer hit list (column 5 of its output), run-length encoded over taxa: a queue entry also carries
//            the ambiguous k-mers before it, a run that resumes after such a span is cut there (the piece after it reuses
//            the run's taxon: no probe, no hit group), and the fragment's trailing ambiguous k-mers and the mate border go
//            in an entry without k-mers.  Pass 2 of the drain emits each lane's entries in read order into an RLE state
//            held in registers.  HITS 1 writes K2_HIT_INLINE entries per unit and counts them all (a longer unit goes on a
//            list); HITS 2 redoes the listed units and writes their whole lists at their final offsets, nothing else.
// A fourth switch, MIND (kraken2 --report-minimizer-data), exists for the pass-1 instances only (default, QUICK, HITS 1): every
// lookup that adds a hit group also counts for its taxon in a sh_k2_mindata accumulator (a counter and 4096 HyperLogLog
// registers per taxon).  The BIG and HITS 2 passes redo units pass 1 already counted, so they have no MIND form.
// The bound is the HBM gather rate: one 32-B sector per probe, ~40 probes per 150-bp read.
//
// k_k2_classify_wave: one wave per unit, for the units of at least opts.long_unit_bases bases (long reads): the 64 lanes scan 64
// consecutive segments of the read side by side.  Same answers, hit lists, minimizer data and counters; its own comment says why.
#include "sh_common.h"
#include "sh_k2_db.h"
#include "sh_k2_inspect.h"
#include "sh_k2_distrib.h"
#include "sh_k2_tx.h"
#include "sh_wave.h"
#include <rocprim/rocprim.hpp>
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <string>
#include <type_traits>
#include <vector>

#define K2_QCAP 8           // pending runs per lane
#define K2_HCAP 8           // distinct taxa per unit kept in LDS (10 KiB of LDS per wave with the queue: 16 waves per CU)
#define K2_BIG_CAP 4096     // ... in HBM for the overflow pass
#define K2_HIT_INLINE 16    // hit-list entries per unit written in place by the HITS 1 instances (8 B each)
#define K2_HIT_NONE 0xfffffffdu          // RLE state before the unit's first entry (never a code)
// HITS queue entry word (s_qamb): the entry starts a run (probe it), the mate border follows it, ambiguous k-mers before it
#define K2Q_PROBE 0x80000000u
#define K2Q_BORDER 0x40000000u
#define K2Q_AMB 0x3fffffffu

// ---- device helpers ----------------------------------------------------------------------------------------------
__host__ __device__ static inline uint64_t k2_fmix64(uint64_t k)
{
    k ^= k >> 33; k *= 0xff51afd7ed558ccdULL;
    k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ULL;
    k ^= k >> 33;
    return k;
}

struct K2Table { const uint32_t *cells; uint64_t capacity; int32_t value_bits; double inv_capacity; };

// hc % capacity without the 64-bit division sequence: the double-precision quotient estimate is off by at most one for
// capacity >= 2^20 (q < 2^44, relative error 2^-52), which one conditional add / subtract repairs
__device__ static inline uint64_t k2_mod(uint64_t hc, uint64_t capacity, double inv_capacity)
{
    if (capacity < (1ull << 20)) return hc % capacity;
    const uint64_t q = (uint64_t)((double)hc * inv_capacity);
    int64_t r = (int64_t)(hc - q * capacity);
    if (r < 0) r += (int64_t)capacity;
    else if (r >= (int64_t)capacity) r -= (int64_t)capacity;
    return (uint64_t)r;
}

// rolling scanner state of one lane; the window holds k - l + 1 candidates (<= W; the instantiations are W = 1, 5 and,
// for every other (k, l), 16 with the live part given at run time; the amino-acid form has W = 4 for k = 15, l = 12, and 16).
// AA: the amino-acid form (mmscanner.cc as recalled: PARITY UNPINNED): the code byte is taken as given, 0..15 (anything above is
// ambiguous), the l-mer is the last l codes at 4 bits each, and there is no reverse complement and no canonical form.
template <int W, bool AA = false>
struct K2Scan {
    uint64_t fw, rc, c[W];
    int32_t loaded;
    __device__ inline void reset()
    {
        fw = rc = 0; loaded = 0;
#pragma unroll
        for (int i = 0; i < W; ++i) c[i] = ~0ull;
    }
    // consumes one base code (0..3, > 3 = ambiguous); pos = characters consumed so far in this fragment (after this one).
    // Returns 0 nothing to report (no full k-mer yet), 1 ambiguous k-mer, 2 minimizer in `m`.
    __device__ inline int step(uint32_t code, int32_t pos, int32_t k, int32_t l, uint64_t lmask, uint64_t spaced, uint64_t toggle, uint64_t &m)
    {
        return step_w(code, pos, k, l, lmask, spaced, toggle, m, k - l + 1);
    }
    __device__ inline int step_w(uint32_t code, int32_t pos, int32_t k, int32_t l, uint64_t lmask, uint64_t spaced, uint64_t toggle, uint64_t &m, int32_t wlim)
    {   // branch-free: 64 lanes scan 64 different reads
        const bool amb = code > (AA ? 15u : 3u);
        fw = amb ? 0ull : ((fw << (AA ? 4 : 2)) | code) & lmask;
        if constexpr (!AA) rc = amb ? 0ull : (rc >> 2) | ((uint64_t)(3u - code) << (2 * (l - 1)));
        loaded = amb ? 0 : (loaded < l ? loaded + 1 : l);
        const bool full = loaded == l;
        uint64_t canon = AA ? fw : (fw < rc ? fw : rc);
        if (spaced) canon &= spaced;
        const uint64_t cand = canon ^ toggle;
#pragma unroll
        for (int i = W - 1; i > 0; --i) c[i] = amb ? ~0ull : (full ? c[i - 1] : c[i]);
        c[0] = amb ? ~0ull : (full ? cand : c[0]);
        uint64_t mn = c[0];
#pragma unroll
        for (int i = 1; i < W; ++i) mn = (i < wlim && c[i] < mn) ? c[i] : mn;
        m = mn ^ toggle;
        return pos >= k ? (full ? 2 : 1) : 0;
    }
};

struct K2Args {
    const uint8_t *bases; const uint64_t *offsets; uint64_t n_units; int32_t paired;
    K2Table T; const uint32_t *parent, *ext; uint32_t n_nodes;
    int32_t k, l; uint64_t spaced, toggle, min_hash; int32_t min_hit_groups; double confidence;
    sh_k2_result *out;
    uint32_t *over_list; unsigned long long *ctr;      // ctr: [0] n_over, [1..] sharded stats
    const uint32_t *unit_list; uint32_t n_list;        // BIG pass: units to redo
    uint32_t *big_tax, *big_cnt;                       // BIG pass: K2_BIG_CAP entries per listed unit
};
// the QMASK instances' arguments (the others keep the kernel arguments they had)
struct K2QArgs : K2Args {
    const uint8_t *quals; int32_t min_qual;            // one byte per base at the bases' offsets (same address mod 8)
};
// ... and the HITS instances' (with or without qualities)
struct K2HArgs : K2QArgs {
    uint2 *hits;                                       // HITS 1: K2_HIT_INLINE (code, count) per unit; HITS 2: the compacted lists
    uint32_t *n_hits;                                  // HITS 1: entries of each unit
    uint32_t *hit_over;                                // HITS 1: units with more than K2_HIT_INLINE entries
    const uint64_t *hit_off;                           // HITS 2: first entry of each unit in `hits` (n_units + 1)
};
// ... and the MIND instances'
struct K2MArgs : K2HArgs {
    uint32_t *md_regs;                                 // K2_MD_WORDS words per taxon: the HLL registers, four to a word
    unsigned long long *md_cnt;                        // n_minimizers per taxon
};
template <bool QMASK, int HITS = 0, bool MIND = false>
using K2ArgsOf = std::conditional_t<MIND, K2MArgs, std::conditional_t<HITS != 0, K2HArgs, std::conditional_t<QMASK, K2QArgs, K2Args>>>;
// ctr layout
#define K2C_OVER 0
#define K2C_HOVER 1
#define K2C_PROBES 8
#define K2C_KMERS 72
#define K2C_CLASSIFIED 136
#define K2C_MASKED 200
#define K2C_WORDS 264

// hit list of one lane: entry j at [j * STRIDE]
template <int STRIDE, int CAP>
struct K2Hits {
    uint32_t *tax, *cnt; int32_t n; bool over;
    __device__ inline void add(uint32_t t, uint32_t c)
    {
        int32_t j = 0;
        while (j < n && tax[j * STRIDE] != t) ++j;
        if (j < n) { cnt[j * STRIDE] += c; return; }
        if (n == CAP) { over = true; return; }
        tax[n * STRIDE] = t; cnt[n * STRIDE] = c; ++n;
    }
};

template <int STRIDE, int CAP>
__device__ static inline uint32_t k2_resolve(const K2Hits<STRIDE, CAP> &H, const uint32_t *__restrict__ parent, uint32_t total_kmers, double confidence)
{
    uint32_t max_taxon = 0, max_score = 0;
    const uint32_t required = (uint32_t)ceil(confidence * (double)total_kmers);
    for (int32_t i = 0; i < H.n; ++i) {
        const uint32_t ti = H.tax[i * STRIDE];
        uint32_t score = 0;
        for (int32_t j = 0; j < H.n; ++j) if (k2_is_ancestor(parent, H.tax[j * STRIDE], ti)) score += H.cnt[j * STRIDE];
        if (score > max_score) { max_score = score; max_taxon = ti; }
        else if (score == max_score) max_taxon = k2_lca(parent, max_taxon, ti);
    }
    max_score = 0;
    for (int32_t i = 0; i < H.n; ++i) if (H.tax[i * STRIDE] == max_taxon) max_score = H.cnt[i * STRIDE];
    while (max_taxon && max_score < required) {
        max_score = 0;
        for (int32_t i = 0; i < H.n; ++i) if (k2_is_ancestor(parent, max_taxon, H.tax[i * STRIDE])) max_score += H.cnt[i * STRIDE];
        if (max_score >= required) return max_taxon;
        max_taxon = parent[max_taxon];
    }
    return max_taxon;
}

__device__ static inline uint32_t k2_finish_probe(const K2Table &T, uint64_t idx, uint32_t cell, uint32_t compacted)
{
    const uint32_t vmask = (1u << T.value_bits) - 1;
    const uint64_t first = idx;
    for (;;) {
        if (!(cell & vmask)) return 0;
        if ((cell >> T.value_bits) == compacted) return cell & vmask;
        idx = idx + 1 == T.capacity ? 0 : idx + 1;
        if (idx == first) return 0;
        cell = T.cells[idx];
    }
}

// Linear probing walks consecutive cells, so a probe reads whole 32-B groups of 8 cells (one HBM sector) instead of one
// cell per dependent load: at load 0.7 a miss inspects ~6 cells = 1-2 groups, and the slowest lane of a wave (which every
// other lane waits for) needs 3-4 steps instead of 30.
struct K2Group { uint4 lo, hi; };
__device__ static inline K2Group k2_load_group(const uint32_t *cells, uint64_t g)
{
    const uint4 *p = (const uint4 *)(cells + 8 * g);
    return K2Group{p[0], p[1]};
}
// first terminating cell (empty, or same truncated key) at or after `start`; returns false if the group has none
__device__ static inline bool k2_scan_group(const K2Group &G, uint32_t start, uint32_t vmask, int32_t vb, uint32_t comp, uint32_t &taxon)
{
    const uint32_t c[8] = {G.lo.x, G.lo.y, G.lo.z, G.lo.w, G.hi.x, G.hi.y, G.hi.z, G.hi.w};
    uint32_t term = 0, match = 0;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const bool e = !(c[t] & vmask), mm = (c[t] >> vb) == comp;
        term |= (uint32_t)(e || mm) << t; match |= (uint32_t)(mm && !e) << t;
    }
    term &= 0xffu << start;
    if (!term) return false;
    const int t0 = __ffs((int)term) - 1;
    uint32_t v = 0;
#pragma unroll
    for (int t = 0; t < 8; ++t) v = t == t0 ? c[t] : v;
    taxon = ((match >> t0) & 1u) ? v & vmask : 0u;
    return true;
}
// the rest of a probe whose first group did not decide it
__device__ static inline uint32_t k2_probe_rest(const K2Table &T, uint64_t g, uint32_t comp)
{
    const uint32_t vmask = (1u << T.value_bits) - 1;
    const uint64_t n_full = T.capacity / 8;          // groups [0, n_full) lie entirely inside the table
    for (uint64_t step = 0; step <= n_full + 1; ++step) {
        ++g;
        if (g >= n_full) {                            // the ragged tail group and the wrap to cell 0: cell by cell
            uint64_t idx = g * 8 < T.capacity ? g * 8 : 0;
            for (; idx < T.capacity && idx >= n_full * 8; ++idx) {
                const uint32_t c = T.cells[idx];
                if (!(c & vmask)) return 0;
                if ((c >> T.value_bits) == comp) return c & vmask;
            }
            g = 0;
            if (n_full == 0) continue;
            const K2Group G0 = k2_load_group(T.cells, 0);
            uint32_t taxon;
            if (k2_scan_group(G0, 0, vmask, T.value_bits, comp, taxon)) return taxon;
            continue;
        }
        const K2Group G = k2_load_group(T.cells, g);
        uint32_t taxon;
        if (k2_scan_group(G, 0, vmask, T.value_bits, comp, taxon)) return taxon;
    }
    return 0;
}

// the whole probe of minimizer v whose home group did not decide it (HITS instances; the others keep this code inline)
__device__ static inline uint32_t k2_probe_long(const K2Table &T, uint64_t v, uint64_t n_full)
{
    const uint64_t hc = k2_fmix64(v);
    const uint32_t comp = (uint32_t)(hc >> (32 + T.value_bits));
    const uint64_t idx = k2_mod(hc, T.capacity, T.inv_capacity);
    return (idx >> 3) < n_full ? k2_probe_rest(T, idx >> 3, comp) : k2_finish_probe(T, idx, T.cells[idx], comp);
}

// HITS: one lane's hit-list state, kept in registers across drains: the open piece (ambiguous k-mers before it, K2Q_PROBE
// if it starts a run), the ambiguous k-mers after its last k-mer, the taxon of the run the drain last looked up, and the RLE
// state (the code and count not yet written, the entries so far, where they go and how many fit)
struct K2HitState {
    uint32_t pamb = 0, namb = 0, pflag = 0, run_taxon = 0;
    uint32_t code = K2_HIT_NONE, cnt = 0, n = 0, cap = 0;
    uint2 *out = nullptr;
    __device__ inline void put(uint32_t c, uint32_t k)
    {
        if (n < cap) out[n] = make_uint2(c, k);
        ++n;
    }
    __device__ inline void emit(uint32_t c, uint32_t k)
    {   // runs of one code merge; the border never does
        if (c == code && c != SH_K2_HIT_BORDER) { cnt += k; return; }
        if (code != K2_HIT_NONE) put(code, cnt);
        code = c; cnt = k;
    }
};
struct K2NoHits {};

// ---- minimizer data (kraken2 --report-minimizer-data; hyperloglogplus.cc as recalled: PARITY UNPINNED) ----
// Dense HyperLogLog, precision 12: the hash is the table's k2_fmix64(minimizer), the register index its top 12 bits, the rank
// the leading zeros of the other 52 bits + 1 (53 when they are all zero).  One byte per register, four to a 32-bit word.
#define K2_MD_P 12
#define K2_MD_M (1u << K2_MD_P)
#define K2_MD_WORDS (K2_MD_M / 4)
#define K2_MD_BINS 54       // register values 0 .. 64 - K2_MD_P + 1
// (register index << 6 | rank) of a hashed minimizer: 18 bits
__host__ __device__ static inline uint32_t k2_md_code(uint64_t h)
{
    const uint64_t w = h << K2_MD_P;
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t rank = w ? (uint32_t)__clzll((long long)w) + 1u : 64u - K2_MD_P + 1u;
#else
    const uint32_t rank = w ? (uint32_t)__builtin_clzll(w) + 1u : 64u - K2_MD_P + 1u;
#endif
    return (uint32_t)(h >> (64 - K2_MD_P)) << 6 | rank;
}
// bytewise maximum of two packed words
__host__ __device__ static inline uint32_t k2_md_max4(uint32_t x, uint32_t y)
{
    uint32_t r = 0;
#pragma unroll
    for (int b = 0; b < 32; b += 8) { const uint32_t p = (x >> b) & 0xffu, q = (y >> b) & 0xffu; r |= (p > q ? p : q) << b; }
    return r;
}
// One lane's share of the accumulator.  A single-taxon (host depletion) database sends every hit of a batch to one counter
// and one 4-KiB register file, so neither gets an unconditional atomic per hit: the register word is read first and a CAS
// loop runs only while the rank is larger than what is there (after warm-up nearly every update is that one cached read);
// the count stays in the lane, (taxon, pending), across its units and is added when the taxon changes and when the lane is done.
struct K2MdState {
    uint32_t tax = 0, n = 0;
    __device__ inline void flush(unsigned long long *cnt)
    {
        if (n) atomicAdd(&cnt[tax], (unsigned long long)n);
        n = 0;
    }
    __device__ inline void hit(const K2MArgs &a, uint32_t taxon, uint32_t code)
    {
        if (taxon >= a.n_nodes) return;                 // a value outside the taxonomy (a damaged table) has no registers
        if (taxon != tax) { flush(a.md_cnt); tax = taxon; }
        ++n;
        uint32_t *w = a.md_regs + (uint64_t)taxon * K2_MD_WORDS + (code >> 8);
        const uint32_t sh = ((code >> 6) & 3u) * 8, rank = code & 63u;
        uint32_t cur = __atomic_load_n(w, __ATOMIC_RELAXED);      // registers only grow: a stale word costs a CAS, never a rank
        while (((cur >> sh) & 0xffu) < rank) {
            const uint32_t prev = atomicCAS(w, cur, (cur & ~(0xffu << sh)) | rank << sh);
            if (prev == cur) break;
            cur = prev;
        }
    }
};
struct K2NoMd {};

// SUB: pass 1 over the units of a.unit_list only (the others went the wave route: k_k2_classify_wave)
// PROT: translated search over a protein database (DESIGN.md §7 "Translated search"; classify.cc as recalled: PARITY UNPINNED).
// a.bases is k_k2_translate's output (scanner codes), a.offsets the nucleotide offsets.  A unit has 6 or 12 fragments, frames
// 0..5 of mate 1 and then of mate 2, whose extents in the code array are arithmetic from the mates' nucleotide extents
// (k2_tx_frame_lens); they run through the same character loop, so last_minimizer is forgotten at the start of every frame, and
// hit groups and taxon counts pool over all of them.  total_kmers is the number of k-mers over all frames; ResolveTree's
// threshold takes K2_TX_S_READ / K2_TX_S_PAIR more (sh_k2_tx.h).  Forms: pass 1 and BIG only.
template <int W, bool BIG, bool QMASK, bool QUICK, int HITS = 0, bool MIND = false, bool SUB = false, bool PROT = false>
__global__ __launch_bounds__(64) void k_k2_classify(K2ArgsOf<QMASK, HITS, MIND> a)
{
    static_assert(!PROT || !(QMASK || QUICK || HITS != 0 || MIND || SUB), "translated search: qualities mask at translation; no --quick, hit list, minimizer data or subset form");
    static_assert(!SUB || !(BIG || QUICK || HITS == 2), "a subset is a pass-1 matter, and --quick units all stay here");
    static_assert(HITS == 0 || !(BIG || QUICK), "the hit list is complete after pass 1 and has no --quick form");
    static_assert(!MIND || !(BIG || HITS == 2), "the redo passes repeat units pass 1 counted: they must not count them again");
    constexpr bool LIST = BIG || HITS == 2 || SUB;         // the work is a list of units
    __shared__ uint64_t s_qmin[(K2_QCAP + 1) * 64];       // slot n_pend is written unconditionally, so one spare
    __shared__ uint32_t s_qlen[(K2_QCAP + 1) * 64];
    __shared__ uint32_t s_qpos[QUICK ? (K2_QCAP + 1) * 64 : 1];      // QUICK: k-mers of the unit before the run's first one
    __shared__ uint32_t s_qamb[HITS ? (K2_QCAP + 1) * 64 : 1];       // HITS: K2Q_* word of the entry
    __shared__ uint32_t s_htax[BIG || QUICK || HITS == 2 ? 1 : K2_HCAP * 64], s_hcnt[BIG || QUICK || HITS == 2 ? 1 : K2_HCAP * 64];
    const uint32_t lane = threadIdx.x;
    const uint64_t lmask = PROT ? (a.l < 16 ? ((1ULL << (4 * a.l)) - 1) : ~0ULL) : (a.l < 32 ? ((1ULL << (2 * a.l)) - 1) : ~0ULL);
    const int32_t wlim = a.k - a.l + 1;
    const uint64_t n_work = LIST ? a.n_list : a.n_units;
    unsigned long long probes_thr = 0, kmers_thr = 0; uint32_t class_thr = 0;
    std::conditional_t<MIND, K2MdState, K2NoMd> M{};       // (an empty object in the other instances)
    [[maybe_unused]] const uint64_t tx_beg = PROT ? a.offsets[0] : 0;      // PROT: the batch's first base (the code array starts there)
    for (uint64_t base = (uint64_t)blockIdx.x * 64; base < n_work; base += (uint64_t)gridDim.x * 64) {
        const uint64_t wi = base + lane;
        const bool active = wi < n_work;
        const uint64_t u = active ? (LIST ? (uint64_t)a.unit_list[wi] : wi) : 0;
        K2Hits<BIG ? 1 : 64, BIG ? K2_BIG_CAP : K2_HCAP> H;
        if (BIG) { H.tax = a.big_tax + (active ? wi : 0) * K2_BIG_CAP; H.cnt = a.big_cnt + (active ? wi : 0) * K2_BIG_CAP; }
        else { H.tax = s_htax + lane; H.cnt = s_hcnt + lane; }
        H.n = 0; H.over = false;
        uint32_t total = 0, groups = 0, n_pend = 0, probes_unit = 0;
        bool stopped = false; uint32_t q_call = 0, q_total = 0;      // QUICK: the unit's scan has stopped on q_call
        const int n_mates = a.paired ? 2 : 1, n_frag = PROT ? 6 * n_mates : n_mates;
        std::conditional_t<HITS != 0, K2HitState, K2NoHits> R{};       // (an empty object in the other instances)
        if constexpr (HITS == 1) { R.out = a.hits + u * K2_HIT_INLINE; R.cap = active ? K2_HIT_INLINE : 0; }
        if constexpr (HITS == 2) { if (active) { R.out = a.hits + a.hit_off[u]; R.cap = (uint32_t)(a.hit_off[u + 1] - a.hit_off[u]); } }
        auto drain = [&]() {
            // pass 1: every lane gathers the home group of each pending run, eight 16-B loads in flight; the outcome goes
            // back into the queue slot: the taxon, or (undecided | truncated key | group) for the rare longer chain
            const uint32_t vmask = (1u << a.T.value_bits) - 1;
            const uint64_t n_full = a.T.capacity / 8;
            uint32_t undecided = 0, skipped = 0;         // per-lane bit e: entry e needs the long-chain code / was not looked up
            for (uint32_t e0 = 0; e0 < K2_QCAP; e0 += 4) {
                if (__ballot(e0 < n_pend) == 0) break;
                uint64_t idx[4]; uint32_t comp[4]; bool go[4]; K2Group G[4];
                [[maybe_unused]] uint32_t mdc[4];        // MIND: k2_md_code of the hash, kept beside the taxon in the slot's high half
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    go[q] = e0 + q < n_pend;
                    if constexpr (HITS) go[q] = go[q] && (s_qamb[(e0 + q) * 64 + lane] & K2Q_PROBE);      // a resumed run, a tail: no probe
                    idx[q] = 0; comp[q] = 0;
                    if (go[q]) {
                        const uint64_t hc = k2_fmix64(s_qmin[(e0 + q) * 64 + lane]);
                        if (a.min_hash && hc < a.min_hash) { go[q] = false; skipped |= 1u << (e0 + q); }      // down-sampled database: not looked up
                        else { comp[q] = (uint32_t)(hc >> (32 + a.T.value_bits)); idx[q] = k2_mod(hc, a.T.capacity, a.T.inv_capacity); }
                        if constexpr (MIND) mdc[q] = k2_md_code(hc);
                    }
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const bool whole = go[q] && (idx[q] >> 3) < n_full;
                    G[q] = whole ? k2_load_group(a.T.cells, idx[q] >> 3) : K2Group{make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0)};
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (!go[q]) continue;
                    uint32_t taxon = 0;
                    const bool whole = (idx[q] >> 3) < n_full;
                    const bool done = whole && k2_scan_group(G[q], (uint32_t)idx[q] & 7u, vmask, a.T.value_bits, comp[q], taxon);
                    if (done) {                                               // else the slot keeps the minimizer for pass 2
                        if constexpr (MIND) s_qmin[(e0 + q) * 64 + lane] = (uint64_t)mdc[q] << 32 | taxon;
                        else s_qmin[(e0 + q) * 64 + lane] = taxon;
                    } else undecided |= 1u << (e0 + q);
                }
            }
            // pass 2: one copy of the long-chain code and of the hit-list update
#pragma nounroll
            for (uint32_t e = 0; e < K2_QCAP + (HITS ? 1 : 0); ++e) {      // HITS: a fragment's flush may queue a ninth entry (a tail)
                if (__ballot(e < n_pend) == 0) break;
                if constexpr (HITS) {
                    if (e < n_pend) {
                        const uint32_t qa = s_qamb[e * 64 + lane], len = s_qlen[e * 64 + lane];
                        if (qa & K2Q_PROBE) {               // the entry starts a run: looked up as in the other instances
                            R.run_taxon = 0;                // not looked up: taxon 0
                            if (!((skipped >> e) & 1u)) {
                                ++probes_unit;
                                const uint64_t v = s_qmin[e * 64 + lane];
                                R.run_taxon = (undecided >> e) & 1u ? k2_probe_long(a.T, v, n_full) : (uint32_t)v;
                                if (R.run_taxon) {
                                    ++groups;
                                    if constexpr (MIND) M.hit(a, R.run_taxon, (undecided >> e) & 1u ? k2_md_code(k2_fmix64(v)) : (uint32_t)(v >> 32));
                                    if constexpr (HITS == 1) H.add(R.run_taxon, len);
                                }
                            }
                        } else if (HITS == 1 && R.run_taxon && len) H.add(R.run_taxon, len);      // the rest of a run after ambiguous k-mers
                        // read order: the ambiguous k-mers, the piece's k-mers, the border
                        if (qa & K2Q_AMB) R.emit(SH_K2_HIT_AMBIGUOUS, qa & K2Q_AMB);
                        if (len) R.emit(R.run_taxon, len);
                        if (qa & K2Q_BORDER) R.emit(SH_K2_HIT_BORDER, 0);
                    }
                } else if (e < n_pend && !(QUICK && stopped)) {      // QUICK: no run after the stopping one is looked at
                    const uint64_t v = s_qmin[e * 64 + lane];
                    if (!((skipped >> e) & 1u)) {
                        ++probes_unit;
                        uint32_t taxon = (uint32_t)v;
                        if ((undecided >> e) & 1u) {        // the chain leaves the home group (or starts in the ragged tail group)
                            const uint64_t hc = k2_fmix64(v);
                            const uint32_t comp = (uint32_t)(hc >> (32 + a.T.value_bits));
                            const uint64_t idx = k2_mod(hc, a.T.capacity, a.T.inv_capacity);
                            taxon = (idx >> 3) < n_full ? k2_probe_rest(a.T, idx >> 3, comp) : k2_finish_probe(a.T, idx, a.T.cells[idx], comp);
                        }
                        if (taxon) {
                            ++groups;
                            if constexpr (MIND) M.hit(a, taxon, (undecided >> e) & 1u ? k2_md_code(k2_fmix64(v)) : (uint32_t)(v >> 32));
                            if constexpr (QUICK) {
                                if ((int32_t)groups >= a.min_hit_groups) { stopped = true; q_call = taxon; q_total = s_qpos[e * 64 + lane]; }
                            } else H.add(taxon, s_qlen[e * 64 + lane]);
                        }
                    }
                }
            }
            n_pend = 0;
        };
        // Both fragments run through ONE character loop (one call site of drain): fragment f covers the chunk range
        // [f * n_chunks_max, (f + 1) * n_chunks_max) of the wave, each lane idling past its own read's end.
        uint64_t o_beg[2] = {0, 0}; int32_t len[2] = {0, 0};
        int32_t max_len = 0;
        for (int f = 0; f < n_mates; ++f) {
            const uint64_t rec = a.paired ? 2 * u + (uint64_t)f : u;
            o_beg[f] = active ? a.offsets[rec] : 0;
            len[f] = active ? (int32_t)(a.offsets[rec + 1] - o_beg[f]) : 0;
            const int32_t frag_len = PROT ? (len[f] >= 3 ? len[f] / 3 : 0) : len[f];      // PROT: a mate's longest frame (frame 2)
            max_len = frag_len > max_len ? frag_len : max_len;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { int32_t t = __shfl_xor(max_len, o); max_len = t > max_len ? t : max_len; }
        const int32_t n_chunks = (max_len + 7) / 8;
        K2Scan<W, PROT> S; S.reset();
        uint64_t last_min = ~0ull; uint32_t run = 0, run_pos = 0;
        int32_t my_len = 0, off8 = 0; uint32_t sh = 0;
        [[maybe_unused]] int32_t frag = 0, frag_c0 = 0;      // PROT: the fragment the loop is in and its first chunk
        const uint64_t *wp = nullptr, *qp = nullptr;
        uint64_t w_cur = 0, w_next = 0, q_cur = 0, q_next = 0, qw = 0;
        // ONE loop over the characters of both fragments with ONE call site of drain (the probe code is large): step s is
        // character (s & 7) of chunk (s >> 3); the step after the last one flushes the final run and empties the queues.
        const int32_t n_steps = n_chunks * n_frag * 8;
        uint64_t w = 0;
#pragma nounroll
        for (int32_t s = 0;; ++s) {
            const bool end = s == n_steps;
            const int32_t cc = s >> 3;
            if constexpr (PROT) {
                if ((s & 7) == 0 && !end && cc - frag_c0 == n_chunks) { ++frag; frag_c0 = cc; }      // (wave-uniform) on to the next frame
            }
            const int32_t c = PROT ? cc - frag_c0 : (cc < n_chunks ? cc : cc - n_chunks);
            if ((s & 7) == 0) {
                if (c == 0 || end) {       // (wave-uniform) fragment boundary: flush the last run, restart the scanner
                    s_qmin[n_pend * 64 + lane] = last_min; s_qlen[n_pend * 64 + lane] = run;
                    if constexpr (QUICK) s_qpos[n_pend * 64 + lane] = run_pos;
                    if constexpr (HITS) s_qamb[n_pend * 64 + lane] = R.pamb | R.pflag;
                    n_pend += run != 0 && !(QUICK && stopped);
                    if constexpr (HITS) {
                        // the fragment's trailing ambiguous k-mers and, after mate 1 (even one without k-mers), the border
                        const bool border = a.paired && s == n_chunks * 8;
                        s_qlen[n_pend * 64 + lane] = 0; s_qamb[n_pend * 64 + lane] = R.namb | (border ? K2Q_BORDER : 0u);
                        n_pend += R.namb != 0 || border;
                        R.pamb = 0; R.namb = 0; R.pflag = 0;
                    }
                    S.reset(); last_min = ~0ull; run = 0;
                    if (!end) {
                        uintptr_t pa;
                        [[maybe_unused]] const int f = cc < n_chunks ? 0 : 1;
                        if constexpr (PROT) {
                            // frame fr of mate m: forward frames 0, 1, 2 and then the reverse ones, back to back from
                            // 2 * (the mate's first base - the batch's); no per-fragment array, only selects
                            const bool m = frag >= 6;
                            const int fr = m ? frag - 6 : frag, g = fr >= 3 ? fr - 3 : fr;
                            uint64_t n0, n1, n2;
                            k2_tx_frame_lens((uint64_t)(m ? len[1] : len[0]), n0, n1, n2);
                            my_len = (int32_t)(g == 0 ? n0 : g == 1 ? n1 : n2);
                            const uint64_t at = (fr >= 3 ? n0 + n1 + n2 : 0) + (g >= 1 ? n0 : 0) + (g >= 2 ? n1 : 0);
                            pa = (uintptr_t)(a.bases + 2 * ((m ? o_beg[1] : o_beg[0]) - tx_beg) + at);
                        } else {
                            my_len = len[f];
                            pa = (uintptr_t)(a.bases + o_beg[f]);
                        }
                        wp = (const uint64_t *)(pa & ~(uintptr_t)7); off8 = (int32_t)(pa & 7); sh = (uint32_t)off8 * 8;
                        // only the aligned words that overlap the read are ever loaded
                        w_cur = my_len > 0 ? wp[0] : 0;
                        w_next = my_len + off8 > 8 ? wp[1] : 0;
                        if constexpr (QMASK) {      // the same words of the quality array (same offsets, same address mod 8)
                            qp = (const uint64_t *)((uintptr_t)(a.quals + o_beg[f]) & ~(uintptr_t)7);
                            q_cur = my_len > 0 ? qp[0] : 0;
                            q_next = my_len + off8 > 8 ? qp[1] : 0;
                        }
                    }
                }
                if (!end) {
                    w = sh ? (w_cur >> sh) | (w_next << (64 - sh)) : w_cur;
                    w_cur = w_next;
                    w_next = (c + 2) * 8 < my_len + off8 ? wp[c + 2] : 0;      // two words ahead: the load has a whole chunk to land
                    if constexpr (QMASK) {
                        qw = sh ? (q_cur >> sh) | (q_next << (64 - sh)) : q_cur;
                        q_cur = q_next;
                        q_next = (c + 2) * 8 < my_len + off8 ? qp[c + 2] : 0;
                    }
                }
            }
            if (__ballot(n_pend >= (end ? 1u : (uint32_t)K2_QCAP - 1)) != 0) drain();       // wave-uniform: every lane is here
            if constexpr (QUICK) {
                // (wave-uniform) every lane has stopped, or has read the last character of its last fragment: straight on to
                // the final flush and drain
                const bool last_frag = cc >= (n_frag - 1) * n_chunks;
                if ((s & 7) == 0 && !end && __ballot(!(stopped || !active || (last_frag && c * 8 >= my_len))) == 0) { s = n_steps - 1; continue; }
            }
            if (end) break;
            const int32_t i = c * 8 + (s & 7);
            uint64_t m;
            uint32_t code = PROT ? (uint32_t)w & 0xffu : sh_nt4((uint32_t)w & 0xffu);
            if constexpr (QMASK) { code = k2_masked((uint32_t)qw & 0xffu, a.min_qual) ? 4u : code; qw >>= 8; }
            int ev = S.step_w(code, i + 1, a.k, a.l, lmask, a.spaced, a.toggle, m, wlim);
            w >>= 8;
            ev = i < my_len ? ev : 0;
            total += ev != 0;
            const bool fresh = ev == 2 && m != last_min;
            s_qmin[n_pend * 64 + lane] = last_min; s_qlen[n_pend * 64 + lane] = run;      // kept only if the run just ended
            if constexpr (QUICK) s_qpos[n_pend * 64 + lane] = run_pos;
            if constexpr (HITS) {
                // a new minimizer, or the same one back after ambiguous k-mers, closes the open piece
                const bool cut = ev == 2 && (fresh || R.namb != 0);
                s_qamb[n_pend * 64 + lane] = R.pamb | R.pflag;
                n_pend += cut && run != 0;
                R.pflag = fresh ? K2Q_PROBE : (cut ? 0u : R.pflag);
                R.pamb = cut ? R.namb : R.pamb;
                R.namb = cut ? 0u : R.namb + (ev == 1);
                run = cut ? 1u : run + (ev == 2);
            } else {
                n_pend += fresh && run != 0 && !(QUICK && stopped);
                run = fresh ? 1u : run + (ev == 2);
            }
            last_min = fresh ? m : last_min;
            if constexpr (QUICK) run_pos = fresh ? total - 1 : run_pos;
        }
        if (QUICK && stopped) total = q_total;      // kraken2 --quick: the k-mers before the stopping one
        if constexpr (HITS) {
            if (R.code != K2_HIT_NONE) R.put(R.code, R.cnt);
            if (HITS == 1 && active) {
                a.n_hits[u] = R.n;
                if (R.n > K2_HIT_INLINE) {
                    const uint32_t oi = (uint32_t)atomicAdd(&a.ctr[K2C_HOVER], 1ull);
                    a.hit_over[oi] = (uint32_t)u;
                }
            }
        }
        if (HITS != 2 && active) {       // HITS 2 redoes units whose results the first pass wrote
            kmers_thr += total;
            if (BIG || !H.over) probes_thr += probes_unit;       // a unit redone by the overflow pass is counted there
            if (!BIG && H.over) {
                const uint32_t oi = (uint32_t)atomicAdd(&a.ctr[K2C_OVER], 1ull);
                a.over_list[oi] = (uint32_t)u;
            } else {
                uint32_t call;
                if constexpr (QUICK) call = stopped ? q_call : 0u;       // no stop: unclassified, whatever ResolveTree would say
                else {
                    if constexpr (PROT) call = k2_resolve(H, a.parent, total + (a.paired ? K2_TX_S_PAIR : K2_TX_S_READ), a.confidence);
                    else call = k2_resolve(H, a.parent, total, a.confidence);
                    if (call && groups < (uint32_t)a.min_hit_groups) call = 0;
                }
                sh_k2_result r{call ? a.ext[call] : 0u, call, total, groups};
                a.out[u] = r;
                class_thr += call != 0;
            }
        }
    }
    if constexpr (MIND) M.flush(a.md_cnt);
    // statistics: one atomic per wave and counter, 64-way sharded
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        probes_thr += (unsigned long long)__shfl_xor((long long)probes_thr, o);
        kmers_thr += (unsigned long long)__shfl_xor((long long)kmers_thr, o);
        class_thr += (uint32_t)__shfl_xor((int)class_thr, o);
    }
    if (lane == 0) {
        const uint32_t sh = blockIdx.x & 63;
        if (probes_thr) atomicAdd(&a.ctr[K2C_PROBES + sh], probes_thr);
        if (kmers_thr && !BIG) atomicAdd(&a.ctr[K2C_KMERS + sh], kmers_thr);
        if (class_thr) atomicAdd(&a.ctr[K2C_CLASSIFIED + sh], (unsigned long long)class_thr);
    }
}

// bases the QMASK instances mask, over the whole batch [offsets[0], offsets[n_records]): counted apart from the scan, which
// with --quick leaves a read early
__global__ void k_k2_count_masked(const uint8_t *quals, const uint64_t *offsets, uint64_t n_records, int32_t min_qual, unsigned long long *ctr)
{
    const uint64_t beg = offsets[0], end = offsets[n_records];
    unsigned long long n = 0;
    for (uint64_t i = beg + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < end; i += (uint64_t)gridDim.x * blockDim.x) n += k2_masked(quals[i], min_qual);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += (unsigned long long)__shfl_xor((long long)n, o);
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(&ctr[K2C_MASKED + (blockIdx.x & 63)], n);
}

// ---- the wave route: one wave classifies one unit (DESIGN.md §7 "Long reads") -------------------------------------------
// A fragment's k-mers are cut into tiles of 64 segments of `seg` k-mers, one segment per lane.  A lane restarts the scanner
// k - 1 bases before its first k-mer (the state at a k-mer depends on that k-mer's bases only) and sees the events the
// sequential scan sees; a run is probed where it starts in the lane, and the first run of a lane becomes a hit group, a
// counted probe and a minimizer-data lookup only once the wave has seen that the last valid minimizer before the segment
// (lanes back, or in the tile before) differs.  K-mer counts go to one taxon table per wave in LDS (open addressing, LDS
// atomics); once it holds K2_WT_CAP taxa new ones go to the block's table in HBM, and a unit that spilled resolves from
// that table after the LDS entries have joined it.  ResolveTree runs across the lanes (the scores in parallel, the tie rule
// an LCA fold over the lanes, each level of the confidence climb one wave sum).  HITS: the tile's per-k-mer codes go to LDS
// and the wave run-length encodes them 64 at a time; form 1 counts the entries and writes the first K2_HIT_INLINE in place,
// form 2 writes the listed units' whole lists at hit_off, as the lane kernel's forms do.
#define K2_WAVE_SEG 63u                     // k-mers per lane and tile at most; odd, so the lanes' code stores hit 64 banks
#define K2_WAVE_TILE (64u * K2_WAVE_SEG)    // k-mers per tile (exported: sh_k2_wave_tile)
#define K2_WAVE_WORDS ((K2_WAVE_TILE + 80u) / 8u)      // the tile's bases: its k-mers + k - 1 <= 45 more + 7 of misalignment, in 8-byte words
#define K2_WT_SLOTS 512u                    // the LDS taxon table
#define K2_WT_CAP 384u                      // ... takes new taxa up to here (64 lanes may pass it together: 448 < 512)
#define K2_WS_SLOTS (2u * K2_BIG_CAP)       // the HBM table of a block; it takes new taxa up to K2_BIG_CAP, the BIG pass's limit
// ctr words of the wave kernels
#define K2C_WTICKET 2
#define K2C_WHOVER 3
#define K2C_WOVER 4
#define K2C_WTICKET2 5
static_assert((K2_WAVE_TILE + 80u) % 8u == 0 && (K2_WT_SLOTS & (K2_WT_SLOTS - 1)) == 0 && K2_WS_SLOTS == 8192u, "wave route sizes");

struct K2Wave {
    uint32_t *spill_tax, *spill_cnt;        // K2_WS_SLOTS each per block, zero between units
    uint32_t *hit_over;                     // HITS 1: the wave route's units with more than K2_HIT_INLINE entries
};

// one probe from the hash to the taxon (the lane kernel splits this over its two drain passes)
__device__ static inline uint32_t k2_probe(const K2Table &T, uint64_t hc)
{
    const uint32_t vmask = (1u << T.value_bits) - 1, comp = (uint32_t)(hc >> (32 + T.value_bits));
    const uint64_t idx = k2_mod(hc, T.capacity, T.inv_capacity), n_full = T.capacity / 8;
    if ((idx >> 3) >= n_full) return k2_finish_probe(T, idx, T.cells[idx], comp);
    uint32_t taxon;
    if (k2_scan_group(k2_load_group(T.cells, idx >> 3), (uint32_t)idx & 7u, vmask, T.value_bits, comp, taxon)) return taxon;
    return k2_probe_rest(T, idx >> 3, comp);
}

// the spill table is touched by atomics and agent-scope loads and stores only: nothing of it may sit in the CU's L1
__device__ static inline uint32_t k2_ld(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ static inline void k2_st(uint32_t *p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

struct K2WaveTable {
    uint32_t *tax, *cnt, *n;                // LDS: the table, n[0] taxa in it, n[1] taxa in the spill table
    uint32_t *stax, *scnt;
    __device__ inline void add_spill(uint32_t t, uint32_t c)
    {
        uint32_t h = (t * 0x9E3779B1u) >> 19;
        for (uint32_t step = 0; step < K2_WS_SLOTS; ++step, h = (h + 1) & (K2_WS_SLOTS - 1)) {
            uint32_t cur = k2_ld(&stax[h]);
            if (cur == 0) {
                if (__hip_atomic_load(&n[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) >= K2_BIG_CAP) return;      // the BIG pass's silent limit
                cur = atomicCAS(&stax[h], 0u, t);
                if (cur == 0) { atomicAdd(&n[1], 1u); cur = t; }
            }
            if (cur == t) { atomicAdd(&scnt[h], c); return; }
        }
    }
    __device__ inline void add(uint32_t t, uint32_t c)
    {
        uint32_t h = (t * 0x9E3779B1u) >> 23;
        for (uint32_t step = 0; step < K2_WT_SLOTS; ++step, h = (h + 1) & (K2_WT_SLOTS - 1)) {
            uint32_t cur = __hip_atomic_load(&tax[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (cur == 0) {
                if (__hip_atomic_load(&n[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) >= K2_WT_CAP) break;
                cur = atomicCAS(&tax[h], 0u, t);
                if (cur == 0) { atomicAdd(&n[0], 1u); cur = t; }
            }
            if (cur == t) { atomicAdd(&cnt[h], c); return; }
        }
        add_spill(t, c);       // (a taxon may then sit in both tables: the LDS entries join the spill table before it is read)
    }
};
struct K2LdsEntries {
    const uint32_t *t, *c;
    __device__ inline uint32_t tax(uint32_t i) const { return t[i]; }
    __device__ inline uint32_t cnt(uint32_t i) const { return c[i]; }
};
struct K2SpillEntries {
    const uint32_t *t, *c;
    __device__ inline uint32_t tax(uint32_t i) const { return k2_ld(t + i); }
    __device__ inline uint32_t cnt(uint32_t i) const { return k2_ld(c + i); }
};

// k2_resolve over n dense entries, by the whole wave (every lane returns the call).  Order-free: a score is a sum over the
// entries, the tie rule leaves the LCA of exactly the taxa with the maximal score, each level of the climb is a sum.
template <class E>
__device__ static inline uint32_t k2_resolve_wave(const E &H, uint32_t n, const uint32_t *__restrict__ parent, uint32_t total_kmers, double confidence, uint32_t lane)
{
    const uint32_t required = (uint32_t)ceil(confidence * (double)total_kmers);
    uint32_t best_s = 0, best_t = 0;
    for (uint32_t i0 = 0; i0 < n; i0 += 64) {
        const uint32_t ti = i0 + lane < n ? H.tax(i0 + lane) : 0u;
        uint32_t score = 0;
        for (uint32_t j0 = 0; j0 < n; j0 += 64) {
            const uint32_t tj = j0 + lane < n ? H.tax(j0 + lane) : 0u, cj = j0 + lane < n ? H.cnt(j0 + lane) : 0u;
            const uint32_t m = n - j0 < 64u ? n - j0 : 64u;
            for (uint32_t jj = 0; jj < m; ++jj) {
                const uint32_t t = (uint32_t)wave_bcast((int32_t)tj, (int)jj), c = (uint32_t)wave_bcast((int32_t)cj, (int)jj);
                if (k2_is_ancestor(parent, t, ti)) score += c;
            }
        }
        if (ti) {
            if (score > best_s) { best_s = score; best_t = ti; }
            else if (score == best_s) best_t = k2_lca(parent, best_t, ti);
        }
    }
    const uint32_t top = wave_all_max_u32(best_s);
    uint32_t max_taxon = best_s == top ? best_t : 0u;       // 0 is the fold's identity
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) max_taxon = k2_lca(parent, max_taxon, (uint32_t)__shfl_xor((int)max_taxon, o));
    uint32_t s = 0;
    for (uint32_t i = lane; i < n; i += 64) if (H.tax(i) == max_taxon) s = H.cnt(i);
    uint32_t max_score = (uint32_t)wave_all_add((int32_t)s);
    while (max_taxon && max_score < required) {
        s = 0;
        for (uint32_t i = lane; i < n; i += 64) if (k2_is_ancestor(parent, max_taxon, H.tax(i))) s += H.cnt(i);
        max_score = (uint32_t)wave_all_add((int32_t)s);
        if (max_score >= required) return max_taxon;
        max_taxon = parent[max_taxon];
    }
    return max_taxon;
}

template <int W, bool QMASK, int HITS = 0, bool MIND = false>
__global__ __launch_bounds__(64) void k_k2_classify_wave(K2ArgsOf<QMASK, HITS, MIND> a, K2Wave wv)
{
    static_assert(!MIND || HITS != 2, "the redo pass repeats units pass 1 counted");
    constexpr bool COUNT = HITS != 2;                      // HITS 2 only writes the lists
    __shared__ uint64_t s_bases[K2_WAVE_WORDS];
    __shared__ uint64_t s_quals[QMASK ? K2_WAVE_WORDS : 1];
    __shared__ uint32_t s_code[HITS ? K2_WAVE_TILE : 1];
    __shared__ uint32_t s_ttax[COUNT ? K2_WT_SLOTS : 1], s_tcnt[COUNT ? K2_WT_SLOTS : 1];
    __shared__ uint32_t s_n[2];
    const uint32_t lane = threadIdx.x;
    const unsigned long long lt = (1ull << lane) - 1;      // the lanes below this one
    const uint64_t lmask = a.l < 32 ? ((1ULL << (2 * a.l)) - 1) : ~0ULL;
    const int32_t wlim = a.k - a.l + 1;
    K2WaveTable H{s_ttax, s_tcnt, s_n, wv.spill_tax + (uint64_t)blockIdx.x * K2_WS_SLOTS, wv.spill_cnt + (uint64_t)blockIdx.x * K2_WS_SLOTS};
    unsigned long long probes_thr = 0, kmers_thr = 0; uint32_t class_thr = 0, over_thr = 0;
    std::conditional_t<MIND, K2MdState, K2NoMd> M{};
    for (;;) {
        uint32_t ticket = 0;
        if (lane == 0) ticket = (uint32_t)atomicAdd(&a.ctr[HITS == 2 ? K2C_WTICKET2 : K2C_WTICKET], 1ull);
        ticket = (uint32_t)__builtin_amdgcn_readfirstlane((int)ticket);
        if (ticket >= a.n_list) break;
        const uint64_t u = a.unit_list[ticket];
        __syncthreads();                                   // the unit before is done with the table
        if constexpr (COUNT) {
            for (uint32_t i = lane; i < K2_WT_SLOTS; i += 64) { s_ttax[i] = 0; s_tcnt[i] = 0; }
            if (lane < 2) s_n[lane] = 0;
        }
        uint32_t total = 0, groups = 0;
        // HITS: the list's state, the same on every lane: the open entry, the entries closed so far, where they go
        uint32_t r_code = K2_HIT_NONE, r_cnt = 0, r_n = 0, r_cap = 0, last_code = K2_HIT_NONE;
        uint2 *r_out = nullptr;
        if constexpr (HITS == 1) { r_out = a.hits + u * K2_HIT_INLINE; r_cap = K2_HIT_INLINE; }
        if constexpr (HITS == 2) { r_out = a.hits + a.hit_off[u]; r_cap = (uint32_t)(a.hit_off[u + 1] - a.hit_off[u]); }
        auto put = [&](uint32_t at, uint32_t c, uint32_t k) { if (at < r_cap) r_out[at] = make_uint2(c, k); };
        const int n_frag = a.paired ? 2 : 1;
        for (int f = 0; f < n_frag; ++f) {
            const uint64_t rec = a.paired ? 2 * u + (uint64_t)f : u;
            const uint64_t o_beg = a.offsets[rec];
            const int32_t len = (int32_t)(a.offsets[rec + 1] - o_beg);
            const uint32_t nk = len >= a.k ? (uint32_t)(len - a.k + 1) : 0u;
            uint32_t seg = ((nk + 63u) / 64u) | 1u;
            seg = seg < K2_WAVE_SEG ? seg : K2_WAVE_SEG;
            bool carry_valid = false; uint64_t carry_min = 0;      // the last valid minimizer of the tiles before (none at a fragment's start)
            for (uint32_t t0 = 0; t0 < nk; t0 += 64u * seg) {
                const uint32_t tile_nk = nk - t0 < 64u * seg ? nk - t0 : 64u * seg;
                // the tile's bases, k-mers t0 .. t0 + tile_nk - 1 = bases t0 .. t0 + tile_nk + k - 2, as the aligned words that hold them
                const uintptr_t pa = (uintptr_t)(a.bases + o_beg + t0);
                const uint32_t d = (uint32_t)(pa & 7), n_words = (d + tile_nk + (uint32_t)a.k - 1u + 7u) / 8u;
                __syncthreads();                           // the tile before has been read
                for (uint32_t w = lane; w < n_words; w += 64) s_bases[w] = ((const uint64_t *)(pa & ~(uintptr_t)7))[w];
                if constexpr (QMASK) {                     // same offsets, same address mod 8
                    const uintptr_t qa = (uintptr_t)(a.quals + o_beg + t0) & ~(uintptr_t)7;
                    for (uint32_t w = lane; w < n_words; w += 64) s_quals[w] = ((const uint64_t *)qa)[w];
                }
                __syncthreads();
                const uint8_t *sb = (const uint8_t *)s_bases + d;
                [[maybe_unused]] const uint8_t *sq = (const uint8_t *)s_quals + d;
                const uint32_t a0 = lane * seg, b0 = a0 + seg < tile_nk ? a0 + seg : tile_nk;      // this lane's k-mers [a0, b0) of the tile
                const bool mine = a0 < tile_nk;
                const uint32_t n_steps = seg + (uint32_t)a.k - 1u;
                K2Scan<W> S; S.reset();
                bool have = false, f_skip = false; uint64_t cur_min = 0, f_min = 0; uint32_t cur_tax = 0, f_tax = 0;
                uint32_t acc_tax = 0, acc_cnt = 0;         // k-mers of the taxon being counted, not yet in the table
#pragma nounroll
                for (uint32_t s = 0; s < n_steps; ++s) {
                    const uint32_t i = a0 + s;             // base of the tile
                    const bool in = mine && i < b0 + (uint32_t)a.k - 1u;
                    uint32_t code = in ? sh_nt4(sb[i]) : 4u;
                    if constexpr (QMASK) code = in && k2_masked(sq[i], a.min_qual) ? 4u : code;
                    uint64_t m;
                    int ev = S.step_w(code, (int32_t)(t0 + i + 1u), a.k, a.l, lmask, a.spaced, a.toggle, m, wlim);
                    ev = in && s >= (uint32_t)a.k - 1u ? ev : 0;      // the warm-up reports nothing
                    total += ev != 0;
                    uint32_t kc = SH_K2_HIT_AMBIGUOUS;
                    if (ev == 2) {
                        if (!have || m != cur_min) {       // a run starts here (the lane's first one: perhaps only continues)
                            const uint64_t hc = k2_fmix64(m);
                            const bool skip = a.min_hash && hc < a.min_hash;      // down-sampled database: not looked up
                            const uint32_t tx = skip ? 0u : k2_probe(a.T, hc);
                            if (!have) { f_min = m; f_tax = tx; f_skip = skip; }
                            else if (COUNT && !skip) {
                                ++probes_thr;
                                if (tx) { ++groups; if constexpr (MIND) M.hit(a, tx, k2_md_code(hc)); }
                            }
                            have = true; cur_min = m; cur_tax = tx;
                        }
                        kc = cur_tax;
                        if (COUNT && cur_tax) {
                            if (cur_tax != acc_tax) { if (acc_cnt) H.add(acc_tax, acc_cnt); acc_tax = cur_tax; acc_cnt = 0; }
                            ++acc_cnt;
                        }
                    }
                    if constexpr (HITS != 0) { if (ev) s_code[i - ((uint32_t)a.k - 1u)] = kc; }
                }
                if (COUNT && acc_cnt) H.add(acc_tax, acc_cnt);
                // whose first run is a run's head: the last lane before this one with a valid k-mer, else the carry
                const unsigned long long vm = __ballot(have);
                const int pl = (vm & lt) ? 63 - __clzll((long long)(vm & lt)) : 0;
                const uint64_t p_min = (uint64_t)__shfl((unsigned long long)cur_min, pl);
                const bool pred = (vm & lt) ? true : carry_valid;
                const uint64_t pm = (vm & lt) ? p_min : carry_min;
                if (COUNT && have && !(pred && pm == f_min) && !f_skip) {
                    ++probes_thr;
                    if (f_tax) { ++groups; if constexpr (MIND) M.hit(a, f_tax, k2_md_code(k2_fmix64(f_min))); }
                }
                if (vm) { carry_min = (uint64_t)__shfl((unsigned long long)cur_min, 63 - __clzll((long long)vm)); carry_valid = true; }
                if constexpr (HITS != 0) {
                    __syncthreads();                       // the codes are in LDS
                    for (uint32_t c0 = 0; c0 < tile_nk; c0 += 64) {
                        const uint32_t nv = tile_nk - c0 < 64u ? tile_nk - c0 : 64u;
                        const uint32_t code = lane < nv ? s_code[c0 + lane] : 0u;
                        uint32_t prev = (uint32_t)__shfl_up((int)code, 1);
                        prev = lane == 0 ? last_code : prev;
                        const bool head = lane < nv && code != prev;      // (a border is never a k-mer's code)
                        const unsigned long long hm = __ballot(head);
                        if (!hm) r_cnt += nv;
                        else {
                            const uint32_t fl = (uint32_t)__ffsll((unsigned long long)hm) - 1u;
                            if (r_code != K2_HIT_NONE) { if (lane == 0) put(r_n, r_code, r_cnt + fl); ++r_n; }
                            const unsigned long long rest = lane < 63 ? hm >> (lane + 1) : 0ull;
                            if (head && rest) put(r_n + (uint32_t)__popcll(hm & lt), code, (uint32_t)__ffsll(rest));
                            r_n += (uint32_t)__popcll(hm) - 1u;
                            const int hl = 63 - __clzll((long long)hm);
                            r_code = (uint32_t)__shfl((int)code, hl); r_cnt = nv - (uint32_t)hl;
                        }
                        last_code = (uint32_t)__shfl((int)code, (int)nv - 1);
                    }
                }
            }
            if constexpr (HITS != 0) {
                if (a.paired && f == 0) {                  // the mate border: closes the open entry, never merges
                    if (r_code != K2_HIT_NONE) { if (lane == 0) put(r_n, r_code, r_cnt); ++r_n; }
                    r_code = SH_K2_HIT_BORDER; r_cnt = 0; last_code = SH_K2_HIT_BORDER;
                }
            }
        }
        if constexpr (HITS != 0) {
            if (r_code != K2_HIT_NONE) { if (lane == 0) put(r_n, r_code, r_cnt); ++r_n; }
            if (HITS == 1 && lane == 0) {
                a.n_hits[u] = r_n;
                if (r_n > K2_HIT_INLINE) wv.hit_over[(uint32_t)atomicAdd(&a.ctr[K2C_WHOVER], 1ull)] = (uint32_t)u;
            }
        }
        if constexpr (COUNT) {
            total = (uint32_t)wave_all_add((int32_t)total);
            groups = (uint32_t)wave_all_add((int32_t)groups);
            __syncthreads();                               // every lane's counts are in the tables
            uint32_t call, n = 0;
            const bool spilled = s_n[1] != 0;
            if (!spilled) {                                // the table's entries to its front (a slot moves to a lower or the same index)
                for (uint32_t c0 = 0; c0 < K2_WT_SLOTS; c0 += 64) {
                    const uint32_t t = s_ttax[c0 + lane], c = s_tcnt[c0 + lane];
                    const unsigned long long tm = __ballot(t != 0);
                    if (t) { const uint32_t at = n + (uint32_t)__popcll(tm & lt); s_ttax[at] = t; s_tcnt[at] = c; }
                    n += (uint32_t)__popcll(tm);
                }
                __syncthreads();
                call = k2_resolve_wave(K2LdsEntries{s_ttax, s_tcnt}, n, a.parent, total, a.confidence, lane);
            } else {
                for (uint32_t i = lane; i < K2_WT_SLOTS; i += 64) if (s_ttax[i]) H.add_spill(s_ttax[i], s_tcnt[i]);
                __threadfence(); __syncthreads();
                for (uint32_t c0 = 0; c0 < K2_WS_SLOTS; c0 += 64) {
                    const uint32_t t = k2_ld(&H.stax[c0 + lane]), c = k2_ld(&H.scnt[c0 + lane]);
                    const unsigned long long tm = __ballot(t != 0);
                    if (t) { const uint32_t at = n + (uint32_t)__popcll(tm & lt); k2_st(&H.stax[at], t); k2_st(&H.scnt[at], c); }
                    n += (uint32_t)__popcll(tm);
                }
                __threadfence(); __syncthreads();
                call = k2_resolve_wave(K2SpillEntries{H.stax, H.scnt}, n, a.parent, total, a.confidence, lane);
                for (uint32_t i = lane; i < K2_WS_SLOTS; i += 64) { k2_st(&H.stax[i], 0u); k2_st(&H.scnt[i], 0u); }
                __threadfence();
            }
            if (call && groups < (uint32_t)a.min_hit_groups) call = 0;
            if (lane == 0) {
                sh_k2_result r{call ? a.ext[call] : 0u, call, total, groups};
                a.out[u] = r;
                kmers_thr += total; class_thr += call != 0; over_thr += n > K2_HCAP;      // n_overflow keeps its meaning
            }
        }
    }
    if constexpr (MIND) M.flush(a.md_cnt);
    if constexpr (COUNT) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) probes_thr += (unsigned long long)__shfl_xor((long long)probes_thr, o);
        if (lane == 0) {
            const uint32_t sh = blockIdx.x & 63;
            if (probes_thr) atomicAdd(&a.ctr[K2C_PROBES + sh], probes_thr);
            if (kmers_thr) atomicAdd(&a.ctr[K2C_KMERS + sh], kmers_thr);
            if (class_thr) atomicAdd(&a.ctr[K2C_CLASSIFIED + sh], (unsigned long long)class_thr);
            if (over_thr) atomicAdd(&a.ctr[K2C_WOVER], (unsigned long long)over_thr);
        }
    }
}

// ---- table construction ----------------------------------------------------------------------------------------------
struct K2Build { uint32_t *cells; uint64_t capacity; int32_t value_bits; const uint32_t *parent; unsigned long long *ctr; };

__device__ static inline void k2_insert(const K2Build &B, uint64_t key, uint32_t value)
{
    const uint64_t hc = k2_fmix64(key);
    const uint32_t compacted = (uint32_t)(hc >> (32 + B.value_bits));
    const uint32_t vmask = (1u << B.value_bits) - 1;
    uint64_t idx = hc % B.capacity;
    const uint64_t first = idx;
    for (;;) {
        uint32_t c = B.cells[idx];
        if (!(c & vmask)) {
            const uint32_t prev = atomicCAS(&B.cells[idx], c, compacted << B.value_bits | value);
            if (prev == c) { atomicAdd(&B.ctr[0], 1ull); return; }
            c = prev;                       // somebody else claimed the cell: look at what is there now
        }
        if ((c >> B.value_bits) == compacted) {
            for (;;) {                      // same (truncated) key: keep the LCA of the two taxa
                const uint32_t nv = k2_lca(B.parent, c & vmask, value);
                if (nv == (c & vmask)) return;
                const uint32_t prev = atomicCAS(&B.cells[idx], c, compacted << B.value_bits | nv);
                if (prev == c) return;
                c = prev;
            }
        }
        idx = idx + 1 == B.capacity ? 0 : idx + 1;
        if (idx == first) { atomicAdd(&B.ctr[1], 1ull); return; }
    }
}

__global__ void k_k2_insert(K2Build B, const uint64_t *keys, const uint32_t *taxa, uint64_t n)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) k2_insert(B, keys[i], taxa[i]);
}

__global__ void k_k2_insert_random(K2Build B, uint64_t seed, uint64_t n, uint32_t lo, uint32_t hi)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t h = k2_fmix64(seed + 0x9E3779B97F4A7C15ULL * (i + 1));
        const uint64_t key = k2_fmix64(h ^ 0xD6E8FEB86659FD93ULL) & ((1ULL << 62) - 1);
        k2_insert(B, key, lo + (uint32_t)(h % (uint64_t)(hi - lo + 1)));
    }
}

#define K2_SEG 1024u
// one thread per K2_SEG-base segment of a long sequence: every minimizer whose k-mer ends inside the segment
template <int W>
__global__ void k_k2_insert_seq(K2Build B, const uint8_t *bases, uint64_t n, uint32_t taxon, int32_t k, int32_t l, uint64_t spaced,
                                uint64_t toggle, uint64_t min_hash, unsigned long long *n_runs)
{
    const uint64_t lmask = l < 32 ? ((1ULL << (2 * l)) - 1) : ~0ULL;
    const uint64_t n_seg = (n + K2_SEG - 1) / K2_SEG;
    unsigned long long runs = 0;
    for (uint64_t sg = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; sg < n_seg; sg += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t s0 = sg * K2_SEG, s1 = s0 + K2_SEG < n ? s0 + K2_SEG : n;
        const uint64_t from = s0 >= (uint64_t)(k - 1) ? s0 - (uint64_t)(k - 1) : 0;      // the first k-mer ending in the segment starts here
        K2Scan<W> S; S.reset();
        uint64_t last = ~0ull;
        for (uint64_t i = from; i < s1; ++i) {
            uint64_t m;
            // `pos` only gates "a full k-mer has been read": count from the warm-up start, never below the true position
            const uint64_t consumed = i - from + 1;
            const int ev = S.step(sh_nt4(bases[i]), (int32_t)(consumed > (uint64_t)k ? (uint64_t)k : consumed), k, l, lmask, spaced, toggle, m);
            if (ev != 2 || i < s0) continue;
            if (m == last) continue;
            last = m;
            if (min_hash && k2_fmix64(m) < min_hash) continue;
            k2_insert(B, m, taxon);
            ++runs;
        }
    }
    if (runs) atomicAdd(n_runs, runs);
}

// ---- library build: a batch of records per launch (DESIGN.md §7 "Database build") ---------------------------------------
// Work item = (record, segment of `seg` bases).  seg_off is the exclusive prefix sum of the records' segment counts, so a lane
// finds its record by binary search and 10^5 short records fill the machine like one chromosome does.  A segment reads its own
// record only: the k - 1 warm-up bases before it (none at the record's start), then its bases; minimizers are reported from the
// first k-mer that ENDS inside the segment, as k_k2_insert_seq does.  The bases come in aligned 8-byte words (two in flight, as in
// k_k2_classify) instead of one byte load per base.  The character loop has one trip count per wave, so `emit` is called by
// all 64 lanes together and may use wave operations.
#define K2_LIB_SEG 1024u      // measured choice: DESIGN.md §7
struct K2LibArgs {
    const uint8_t *bases; const uint64_t *offsets; const uint32_t *taxa;     // taxa == nullptr: every record counts (estimator)
    uint64_t n_records; uint64_t *seg_off;                                   // n_records + 1
    uint32_t n_nodes;                                                        // a taxon at or above it is skipped like taxon 0
    uint32_t seg; int32_t k, l; uint64_t spaced, toggle, min_hash;
};

__global__ void k_k2_lib_segcount(K2LibArgs a)
{
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r <= a.n_records; r += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t n = 0;
        if (r < a.n_records && (!a.taxa || (a.taxa[r] && a.taxa[r] < a.n_nodes))) {
            const uint64_t len = a.offsets[r + 1] - a.offsets[r];
            n = len >= (uint64_t)a.k ? (len + a.seg - 1) / a.seg : 0;
        }
        a.seg_off[r] = n;
    }
}

// AA: a protein library, a.bases holding scanner codes (k_k2_aa_encode), scanned by the amino-acid form of K2Scan
template <int W, bool AA, typename Emit>
__device__ static inline void k2_lib_scan(const K2LibArgs &a, Emit emit)
{
    const uint32_t lane = threadIdx.x;
    const uint64_t lmask = AA ? (a.l < 16 ? ((1ULL << (4 * a.l)) - 1) : ~0ULL) : (a.l < 32 ? ((1ULL << (2 * a.l)) - 1) : ~0ULL);
    const int32_t wlim = a.k - a.l + 1;
    const uint64_t n_items = a.seg_off[a.n_records];
    for (uint64_t base = (uint64_t)blockIdx.x * 64; base < n_items; base += (uint64_t)gridDim.x * 64) {
        const uint64_t item = base + lane;
        const bool active = item < n_items;
        uint32_t taxon = 0; int32_t n = 0, lead = 0;
        const uint8_t *p = a.bases;
        if (active) {
            uint64_t lo = 0, hi = a.n_records;       // the last record r with seg_off[r] <= item (records without segments are passed over)
            while (hi - lo > 1) { const uint64_t mid = (lo + hi) >> 1; if (a.seg_off[mid] <= item) lo = mid; else hi = mid; }
            const uint64_t r0 = a.offsets[lo], len = a.offsets[lo + 1] - r0;
            const uint64_t s0 = (item - a.seg_off[lo]) * a.seg, s1 = s0 + a.seg < len ? s0 + a.seg : len;
            const uint64_t from = s0 >= (uint64_t)(a.k - 1) ? s0 - (uint64_t)(a.k - 1) : 0;
            p = a.bases + r0 + from; n = (int32_t)(s1 - from); lead = (int32_t)(s0 - from);
            taxon = a.taxa ? a.taxa[lo] : 1u;
        }
        int32_t n_max = n;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { const int32_t t = __shfl_xor(n_max, o); n_max = t > n_max ? t : n_max; }
        const uint64_t *wp = (const uint64_t *)((uintptr_t)p & ~(uintptr_t)7);
        const int32_t off8 = (int32_t)((uintptr_t)p & 7); const uint32_t sh = (uint32_t)off8 * 8;
        // only the aligned words that overlap the segment are ever loaded
        uint64_t w_cur = n > 0 ? wp[0] : 0, w_next = n + off8 > 8 ? wp[1] : 0;
        K2Scan<W, AA> S; S.reset();
        uint64_t last = ~0ull;
        const int32_t n_chunks = (n_max + 7) / 8;
#pragma nounroll
        for (int32_t c = 0; c < n_chunks; ++c) {
            uint64_t w = sh ? (w_cur >> sh) | (w_next << (64 - sh)) : w_cur;
            w_cur = w_next;
            w_next = (c + 2) * 8 < n + off8 ? wp[c + 2] : 0;
#pragma unroll
            for (int32_t j = 0; j < 8; ++j) {
                const int32_t i = c * 8 + j;
                uint64_t m;
                // `pos` only gates "a full k-mer has been read": counted from the warm-up start, never above k
                const int ev = S.step_w(AA ? (uint32_t)w & 0xffu : sh_nt4((uint32_t)w & 0xffu), i + 1 < a.k ? i + 1 : a.k, a.k, a.l, lmask, a.spaced, a.toggle, m, wlim);
                w >>= 8;
                const bool fresh = ev == 2 && i < n && i >= lead && m != last;
                last = fresh ? m : last;
                emit(fresh && !(a.min_hash && k2_fmix64(m) < a.min_hash), m, taxon);
            }
        }
    }
}

template <int W, bool AA = false>
__global__ __launch_bounds__(64) void k_k2_insert_lib(K2Build B, K2LibArgs a, unsigned long long *n_runs)
{
    unsigned long long runs = 0;
    k2_lib_scan<W, AA>(a, [&](bool go, uint64_t m, uint32_t taxon) {
        if (go) { k2_insert(B, m, taxon); ++runs; }
    });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) runs += (unsigned long long)__shfl_xor((long long)runs, o);
    if (threadIdx.x == 0 && runs) atomicAdd(n_runs, runs);
}

// estimate_capacity.cc as recalled: minimizers whose hash falls in 4 of 1024 residues are collected; the distinct ones are
// counted on the host side of the call (sort + unique).  One atomic per wave and step that samples anything; ctr[0] counts
// every sampled run, also those that no longer fit `cap` (the caller grows the buffer and repeats the batch).
template <int W, bool AA = false>
__global__ __launch_bounds__(64) void k_k2_estimate_lib(K2LibArgs a, uint64_t *buf, uint64_t cap, unsigned long long *ctr)
{
    const uint32_t lane = threadIdx.x;
    k2_lib_scan<W, AA>(a, [&](bool go, uint64_t m, uint32_t) {
        const bool take = go && (k2_fmix64(m) & 1023u) < 4u;
        const unsigned long long mask = __ballot(take);
        if (!mask) return;
        unsigned long long at = 0;
        const int leader = __ffsll((long long)mask) - 1;
        if ((int)lane == leader) at = atomicAdd(ctr, (unsigned long long)__popcll(mask));
        at = (unsigned long long)__shfl((long long)at, leader);
        at += (unsigned long long)__popcll(mask & ((1ull << lane) - 1));
        if (take && at < cap) buf[at] = m;
    });
}

// the window k - l + 1 as a compile-time constant, handed to a generic lambda: 1, 5 (k = 35, l = 31) and, for every other
// (k, l), 16 with the live part given at run time (K2Scan)
template <class F>
static void k2_with_window(int32_t k, int32_t l, F &&f)
{
    switch (k - l + 1) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 5: f(std::integral_constant<int, 5>{}); break;
    default: f(std::integral_constant<int, 16>{}); break;
    }
}
// ... of the amino-acid scanner: 4 (k = 15, l = 12) and the generic 16
template <class F>
static void k2_with_window_aa(int32_t k, int32_t l, F &&f)
{
    if (k - l + 1 == 4) f(std::integral_constant<int, 4>{}); else f(std::integral_constant<int, 16>{});
}
template <class F>
static void k2_with_flag(bool b, F &&f)
{
    if (b) f(std::true_type{}); else f(std::false_type{});
}

// ---- host side -------------------------------------------------------------------------------------------------------
extern "C" sh_status sh_k2_default_opts(sh_k2_opts *o)
{
    SH_CHECK(o, SH_ERR_BAD_ARG, "sh_k2_default_opts: null argument");
    memset(o, 0, sizeof(*o));
    o->k = 35; o->l = 31;
    o->spaced_seed_mask = (0x3ffffffffULL << 28) | 0x3333333ULL;      // --minimizer-spaces 7
    o->toggle_mask = 0xe37e28c4271b5a2dULL;
    o->value_bits = 17;
    o->min_hit_groups = 2;
    o->confidence = 0.0;
    o->min_base_quality = 0; o->quick = 0;
    o->long_unit_bases = 0;
    return SH_OK;
}

// kraken2-build --protein as recalled (PARITY UNPINNED): k = 15 and l = 12 amino acids, no spaced seed
extern "C" sh_status sh_k2_default_protein_opts(sh_k2_opts *o)
{
    sh_status st = sh_k2_default_opts(o);
    if (st != SH_OK) return st;
    o->k = 15; o->l = 12; o->spaced_seed_mask = 0; o->protein = 1;
    return SH_OK;
}

// (k, l) a scanner exists for: the l-mer fits 64 bits (2 bits a base, 4 bits an amino acid), the window 16 candidates
static bool k2_kl_ok(const sh_k2_opts &o)
{
    return o.l >= 1 && o.l <= (o.protein ? 15 : 31) && o.k >= o.l && o.k - o.l + 1 <= 16;
}
static const char *k2_kind(int32_t protein) { return protein ? "protein" : "nucleotide"; }
// the check every call with options of its own makes: they are for the kind of database they are used on
#define K2_CHECK_KIND(db, o, who) \
    SH_CHECK(((o).protein != 0) == ((db)->opts.protein != 0), SH_ERR_BAD_ARG, "%s: %s options on a %s database", who, k2_kind((o).protein), k2_kind((db)->opts.protein))

static sh_status k2_upload_taxonomy(sh_k2_db *db)
{
    const size_t n = db->nodes.size();
    std::vector<uint32_t> parent(n), ext(n);
    for (size_t i = 0; i < n; ++i) {
        SH_CHECK(db->nodes[i].parent < (i ? i : 1) || i <= 1, SH_ERR_BAD_ARG, "taxonomy: node %zu has parent %llu (ids must be breadth-first)", i,
                 (unsigned long long)db->nodes[i].parent);
        parent[i] = (uint32_t)db->nodes[i].parent; ext[i] = (uint32_t)db->nodes[i].external_id;
    }
    SH_HIP(hipMalloc(&db->d_parent, std::max<size_t>(n, 1) * 4));
    SH_HIP(hipMalloc(&db->d_ext, std::max<size_t>(n, 1) * 4));
    SH_HIP(hipMemcpy(db->d_parent, parent.data(), n * 4, hipMemcpyHostToDevice));
    SH_HIP(hipMemcpy(db->d_ext, ext.data(), n * 4, hipMemcpyHostToDevice));
    SH_HIP(hipMalloc(&db->d_ctr, K2C_WORDS * 8));
    SH_HIP(hipMemset(db->d_ctr, 0, K2C_WORDS * 8));
    return SH_OK;
}

extern "C" sh_status sh_k2_free(sh_k2_db *db)
{
    if (!db) return SH_OK;
    hipFree(db->d_cells); hipFree(db->d_parent); hipFree(db->d_ext); hipFree(db->d_ctr);
    delete db;
    return SH_OK;
}

extern "C" sh_status sh_k2_create(const sh_k2_opts *opts, uint64_t capacity, const sh_k2_taxnode *nodes, uint64_t n_nodes,
                                  const char *names, uint64_t names_len, const char *ranks, uint64_t ranks_len, int device, sh_k2_db **out)
{
    SH_CHECK(opts && nodes && out && capacity > 0 && n_nodes >= 2, SH_ERR_BAD_ARG, "sh_k2_create: bad argument");
    SH_CHECK(k2_kl_ok(*opts), SH_ERR_BAD_ARG, "sh_k2_create: unsupported k=%d l=%d for a %s database", opts->k, opts->l, k2_kind(opts->protein));
    SH_CHECK(opts->value_bits >= 1 && opts->value_bits <= 31 && n_nodes <= (1ull << opts->value_bits), SH_ERR_BAD_ARG,
             "sh_k2_create: %llu taxonomy nodes do not fit %d value bits", (unsigned long long)n_nodes, opts->value_bits);
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= device) { sh_set_error("no HIP device %d", device); return SH_ERR_NO_DEVICE; }
    SH_HIP(hipSetDevice(device));
    sh_k2_db *db = new sh_k2_db;
    db->device = device; db->opts = *opts; db->capacity = capacity; db->value_bits = opts->value_bits; db->key_bits = 32 - opts->value_bits;
    db->opts.protein = opts->protein != 0; db->dna_db = !db->opts.protein;
    db->nodes.assign(nodes, nodes + n_nodes);
    if (names) db->names.assign(names, names + names_len);
    if (ranks) db->ranks.assign(ranks, ranks + ranks_len);
    hipError_t e = hipMalloc(&db->d_cells, capacity * 4);
    if (e != hipSuccess) { sh_set_error("sh_k2_create: %llu cells: %s", (unsigned long long)capacity, hipGetErrorString(e)); sh_k2_free(db); return SH_ERR_OOM; }
    e = hipMemset(db->d_cells, 0, capacity * 4);
    if (e != hipSuccess) { sh_set_error("memset: %s", hipGetErrorString(e)); sh_k2_free(db); return SH_ERR_HIP; }
    sh_status st = k2_upload_taxonomy(db);
    if (st != SH_OK) { sh_k2_free(db); return st; }
    *out = db;
    return SH_OK;
}

static sh_status k2_sync_counts(sh_k2_db *db, hipStream_t s)
{
    unsigned long long c[2];
    SH_HIP(hipMemcpyAsync(c, db->d_ctr, 16, hipMemcpyDeviceToHost, s));
    SH_HIP(hipStreamSynchronize(s));
    SH_HIP(hipGetLastError());
    SH_CHECK(c[1] == 0, SH_ERR_OOM, "k2 table of %llu cells is full: build with a larger --capacity", (unsigned long long)db->capacity);
    db->size = c[0];
    return SH_OK;
}

static K2Build k2_build_args(sh_k2_db *db) { return K2Build{db->d_cells, db->capacity, db->value_bits, db->d_parent, db->d_ctr}; }

extern "C" sh_status sh_k2_insert_device(sh_k2_db *db, const uint64_t *d_keys, const uint32_t *d_taxa, uint64_t n, void *stream)
{
    SH_CHECK(db && (n == 0 || (d_keys && d_taxa)), SH_ERR_BAD_ARG, "sh_k2_insert_device: null argument");
    SH_HIP(hipSetDevice(db->device));
    hipStream_t s = (hipStream_t)stream;
    if (n) hipLaunchKernelGGL(k_k2_insert, dim3((uint32_t)std::min<uint64_t>((n + 255) / 256, 65536)), dim3(256), 0, s, k2_build_args(db), d_keys, d_taxa, n);
    return k2_sync_counts(db, s);
}

extern "C" sh_status sh_k2_insert_random(sh_k2_db *db, uint64_t seed, uint64_t n, uint32_t lo, uint32_t hi, void *stream)
{
    SH_CHECK(db && lo >= 1 && hi >= lo && hi < db->nodes.size(), SH_ERR_BAD_ARG, "sh_k2_insert_random: taxon range [%u, %u] outside the taxonomy", lo, hi);
    SH_HIP(hipSetDevice(db->device));
    hipStream_t s = (hipStream_t)stream;
    if (n) hipLaunchKernelGGL(k_k2_insert_random, dim3((uint32_t)std::min<uint64_t>((n + 255) / 256, 65536)), dim3(256), 0, s, k2_build_args(db), seed, n, lo, hi);
    return k2_sync_counts(db, s);
}

extern "C" sh_status sh_k2_insert_sequence_device(sh_k2_db *db, const uint8_t *d_bases, uint64_t n, uint32_t taxon, void *stream, uint64_t *n_inserted)
{
    SH_CHECK(db && d_bases && taxon >= 1 && taxon < db->nodes.size(), SH_ERR_BAD_ARG, "sh_k2_insert_sequence_device: bad argument");
    SH_CHECK(!db->opts.protein, SH_ERR_BAD_ARG, "sh_k2_insert_sequence_device: a protein database is filled by sh_k2_insert_library_device");
    SH_HIP(hipSetDevice(db->device));
    hipStream_t s = (hipStream_t)stream;
    unsigned long long *d_runs = db->d_ctr + 2;
    SH_HIP(hipMemsetAsync(d_runs, 0, 8, s));
    if (n >= (uint64_t)db->opts.k) {
        const uint64_t n_seg = (n + K2_SEG - 1) / K2_SEG;
        k2_with_window(db->opts.k, db->opts.l, [&](auto w) {
            hipLaunchKernelGGL(k_k2_insert_seq<decltype(w)::value>, dim3((uint32_t)std::min<uint64_t>((n_seg + 63) / 64, 1 << 20)), dim3(64), 0, s, k2_build_args(db),
                               d_bases, n, taxon, db->opts.k, db->opts.l, db->opts.spaced_seed_mask, db->opts.toggle_mask, db->opts.min_acceptable_hash, d_runs);
        });
    }
    unsigned long long r = 0;
    SH_HIP(hipMemcpyAsync(&r, d_runs, 8, hipMemcpyDeviceToHost, s));
    sh_status st = k2_sync_counts(db, s);
    if (n_inserted) *n_inserted = r;
    return st;
}

// ---- library build: host side of the two kernels above -------------------------------------------------------------------
static uint32_t k2_lib_seg()
{   // the segment length is a measured choice (scripts/k2_build_speed.py sweeps it through this switch)
    const char *e = getenv("SCRUBBY_HIP_K2_SEG");
    const long v = e && *e ? atol(e) : 0;
    return v >= 64 && v <= (1 << 20) ? (uint32_t)v : K2_LIB_SEG;
}

// segment counts and their prefix sum in d_seg (n_records + 1 words, caller-owned, as is the scan's scratch, which must outlive
// the stream's work); everything on stream s, no synchronisation
static sh_status k2_lib_prepare(K2LibArgs &a, const sh_k2_opts &o, const uint8_t *d_bases, const uint64_t *d_offsets, const uint32_t *d_taxa, uint64_t n_records,
                                uint64_t *d_seg, DevBuf &tmp, hipStream_t s)
{
    a.bases = d_bases; a.offsets = d_offsets; a.taxa = d_taxa; a.n_records = n_records; a.seg_off = d_seg;
    a.seg = k2_lib_seg(); a.k = o.k; a.l = o.l; a.spaced = o.spaced_seed_mask; a.toggle = o.toggle_mask; a.min_hash = o.min_acceptable_hash;
    hipLaunchKernelGGL(k_k2_lib_segcount, dim3((uint32_t)std::min<uint64_t>((n_records + 256) / 256, 4096)), dim3(256), 0, s, a);
    size_t tmp_bytes = 0;
    SH_HIP(rocprim::exclusive_scan(nullptr, tmp_bytes, d_seg, d_seg, (uint64_t)0, n_records + 1, rocprim::plus<uint64_t>(), s));
    SH_HIP(tmp.alloc(std::max<size_t>(tmp_bytes, 1)));
    SH_HIP(rocprim::exclusive_scan(tmp.p, tmp_bytes, d_seg, d_seg, (uint64_t)0, n_records + 1, rocprim::plus<uint64_t>(), s));
    return SH_OK;
}
#define K2_LIB_GRID (256 * 32)      // one-wave blocks, grid-stride over the work items (their number stays on the device)

// A protein library batch (amino-acid FASTA residues, either case): its scanner codes in call-scoped scratch, one streaming pass
// (k_k2_aa_encode).  *d_codes is the array to scan in place of d_bases (indexed by the same offsets, same address modulo 8).
// One synchronisation: the batch's extent is read back.
static sh_status k2_lib_encode(const uint8_t *d_bases, const uint64_t *d_offsets, uint64_t n_records, DevBuf &scratch, const uint8_t **d_codes, hipStream_t s)
{
    uint64_t ends[2];
    SH_HIP(hipMemcpyAsync(&ends[0], d_offsets, 8, hipMemcpyDeviceToHost, s));
    SH_HIP(hipMemcpyAsync(&ends[1], d_offsets + n_records, 8, hipMemcpyDeviceToHost, s));
    SH_HIP(hipStreamSynchronize(s));
    SH_CHECK(ends[1] >= ends[0], SH_ERR_BAD_ARG, "protein library: offsets decrease");
    const uint64_t n = ends[1] - ends[0];
    const uintptr_t mis = (uintptr_t)(d_bases + ends[0]) & 7;
    SH_HIP(scratch.alloc(n + 24));
    SH_HIP(hipMemsetAsync(scratch.p, (int)K2_AA_AMBIG, n + 24, s));          // the bytes around the batch: ambiguous, as 'N' is around a nucleotide batch
    uint8_t *codes = scratch.as<uint8_t>() + mis;
    sh_status st = shi_k2_aa_encode_device(d_bases + ends[0], codes, n, s);
    if (st != SH_OK) return st;
    *d_codes = (const uint8_t *)((uintptr_t)codes - (uintptr_t)ends[0]);
    return SH_OK;
}

extern "C" sh_status sh_k2_set_min_acceptable_hash(sh_k2_db *db, uint64_t min_acceptable_hash)
{
    SH_CHECK(db, SH_ERR_BAD_ARG, "sh_k2_set_min_acceptable_hash: null argument");
    db->opts.min_acceptable_hash = min_acceptable_hash;
    return SH_OK;
}

extern "C" sh_status sh_k2_insert_library_device(sh_k2_db *db, const uint8_t *d_bases, const uint64_t *d_offsets, const uint32_t *d_taxa, uint64_t n_records,
                                                 void *stream, sh_k2_build_stats *stats)
{
    SH_CHECK(db && d_offsets && d_taxa && (d_bases || n_records == 0), SH_ERR_BAD_ARG, "sh_k2_insert_library_device: null argument");
    if (stats) memset(stats, 0, sizeof(*stats));
    SH_HIP(hipSetDevice(db->device));
    hipStream_t s = (hipStream_t)stream;
    if (n_records == 0) return k2_sync_counts(db, s);
    DevBuf b_seg, b_tmp;
    DevEvent e0, e1;
    SH_HIP(b_seg.alloc((n_records + 1) * 8));
    SH_HIP(e0.create()); SH_HIP(e1.create());
    uint64_t *d_seg = b_seg.as<uint64_t>();
    unsigned long long *d_runs = db->d_ctr + 2;
    SH_HIP(hipMemsetAsync(d_runs, 0, 8, s));
    SH_HIP(hipEventRecord(e0.e, s));
    K2LibArgs a{};
    a.n_nodes = (uint32_t)db->nodes.size();
    DevBuf b_codes;
    sh_status st = SH_OK;
    if (db->opts.protein) { st = k2_lib_encode(d_bases, d_offsets, n_records, b_codes, &d_bases, s); if (st != SH_OK) return st; }
    st = k2_lib_prepare(a, db->opts, d_bases, d_offsets, d_taxa, n_records, d_seg, b_tmp, s);
    if (st != SH_OK) return st;
    if (db->opts.protein) k2_with_window_aa(db->opts.k, db->opts.l, [&](auto w) {
        hipLaunchKernelGGL((k_k2_insert_lib<decltype(w)::value, true>), dim3(K2_LIB_GRID), dim3(64), 0, s, k2_build_args(db), a, d_runs);
    });
    else k2_with_window(db->opts.k, db->opts.l, [&](auto w) {
        hipLaunchKernelGGL(k_k2_insert_lib<decltype(w)::value>, dim3(K2_LIB_GRID), dim3(64), 0, s, k2_build_args(db), a, d_runs);
    });
    hipEventRecord(e1.e, s);
    unsigned long long r = 0, n_seg = 0;
    hipMemcpyAsync(&r, d_runs, 8, hipMemcpyDeviceToHost, s);
    hipMemcpyAsync(&n_seg, d_seg + n_records, 8, hipMemcpyDeviceToHost, s);
    st = k2_sync_counts(db, s);        // the one synchronisation of the batch
    if (stats) {
        stats->n_records = n_records; stats->n_segments = n_seg; stats->n_runs = r; stats->size = db->size;
        hipEventElapsedTime(&stats->ms, e0.e, e1.e);
    }
    return st;
}

struct sh_k2_estimator {
    int device = 0;
    sh_k2_opts opts{};
    uint64_t *d_buf = nullptr, *d_alt = nullptr;      // [0, n_have) distinct and sorted; a batch appends behind them
    uint64_t cap = 0, n_have = 0;
    unsigned long long *d_ctr = nullptr;              // [0] appended entries (n_have included), [1] distinct after the batch
};

extern "C" sh_status sh_k2_estimator_free(sh_k2_estimator *e)
{
    if (!e) return SH_OK;
    hipSetDevice(e->device);
    hipFree(e->d_buf); hipFree(e->d_alt); hipFree(e->d_ctr);
    delete e;
    return SH_OK;
}

extern "C" sh_status sh_k2_estimator_create(const sh_k2_opts *opts, int device, sh_k2_estimator **out)
{
    SH_CHECK(opts && out, SH_ERR_BAD_ARG, "sh_k2_estimator_create: null argument");
    SH_CHECK(k2_kl_ok(*opts), SH_ERR_BAD_ARG, "sh_k2_estimator_create: unsupported k=%d l=%d for a %s database", opts->k, opts->l, k2_kind(opts->protein));
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= device) { sh_set_error("no HIP device %d", device); return SH_ERR_NO_DEVICE; }
    SH_HIP(hipSetDevice(device));
    sh_k2_estimator *e = new sh_k2_estimator;
    e->device = device; e->opts = *opts;
    e->opts.min_acceptable_hash = 0;       // the estimate is of the whole library; --max-db-size is applied to it afterwards
    if (hipMalloc(&e->d_ctr, 16) != hipSuccess) { delete e; sh_set_error("sh_k2_estimator_create: out of device memory"); return SH_ERR_OOM; }
    *out = e;
    return SH_OK;
}

static sh_status k2_estimator_grow(sh_k2_estimator *e, uint64_t cap, hipStream_t s)
{
    DevBuf nb, na;
    SH_HIP(nb.alloc(cap * 8));
    SH_HIP(na.alloc(cap * 8));
    if (e->n_have) SH_HIP(hipMemcpyAsync(nb.p, e->d_buf, e->n_have * 8, hipMemcpyDeviceToDevice, s));
    SH_HIP(hipStreamSynchronize(s));
    void *old_buf = e->d_buf, *old_alt = e->d_alt;
    e->d_buf = nb.as<uint64_t>(); e->d_alt = na.as<uint64_t>(); e->cap = cap;
    nb.p = old_buf; na.p = old_alt;      // the handle owns the new pair; the old one is freed on the way out
    return SH_OK;
}

extern "C" sh_status sh_k2_estimate_capacity_device(sh_k2_estimator *e, const uint8_t *d_bases, const uint64_t *d_offsets, uint64_t n_records, void *stream,
                                                    uint64_t *n_sampled)
{
    SH_CHECK(e && d_offsets && (d_bases || n_records == 0), SH_ERR_BAD_ARG, "sh_k2_estimate_capacity_device: null argument");
    SH_HIP(hipSetDevice(e->device));
    hipStream_t s = (hipStream_t)stream;
    if (n_sampled) *n_sampled = e->n_have;
    if (n_records == 0) return SH_OK;
    DevBuf b_seg, b_tmp, b_tmp2, b_codes;
    SH_HIP(b_seg.alloc((n_records + 1) * 8));
    K2LibArgs a{};
    sh_status st = SH_OK;
    if (e->opts.protein) { st = k2_lib_encode(d_bases, d_offsets, n_records, b_codes, &d_bases, s); if (st != SH_OK) return st; }
    st = k2_lib_prepare(a, e->opts, d_bases, d_offsets, nullptr, n_records, b_seg.as<uint64_t>(), b_tmp, s);
    if (st != SH_OK) return st;
    if (e->cap < e->n_have + (1u << 16)) { st = k2_estimator_grow(e, e->n_have * 2 + (1u << 20), s); if (st != SH_OK) return st; }
    for (int attempt = 0;; ++attempt) {
        unsigned long long c0 = e->n_have, total = 0;
        SH_CHECK(hipMemcpyAsync(e->d_ctr, &c0, 8, hipMemcpyHostToDevice, s) == hipSuccess, SH_ERR_HIP, "estimator: copy failed");
        if (e->opts.protein) k2_with_window_aa(e->opts.k, e->opts.l, [&](auto w) {
            hipLaunchKernelGGL((k_k2_estimate_lib<decltype(w)::value, true>), dim3(K2_LIB_GRID), dim3(64), 0, s, a, e->d_buf, e->cap, e->d_ctr);
        });
        else k2_with_window(e->opts.k, e->opts.l, [&](auto w) {
            hipLaunchKernelGGL(k_k2_estimate_lib<decltype(w)::value>, dim3(K2_LIB_GRID), dim3(64), 0, s, a, e->d_buf, e->cap, e->d_ctr);
        });
        SH_CHECK(hipMemcpyAsync(&total, e->d_ctr, 8, hipMemcpyDeviceToHost, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess && hipGetLastError() == hipSuccess,
                 SH_ERR_HIP, "estimator: the scan failed");
        if (total > e->cap) {           // more sampled runs than the buffer holds: a larger one, and the batch again
            SH_CHECK(!attempt, SH_ERR_HIP, "estimator: sample buffer overflow");
            st = k2_estimator_grow(e, total + (1u << 16), s);
            if (st != SH_OK) return st;
            continue;
        }
        if (total > e->n_have) {        // sort everything, keep the distinct keys
            size_t b1 = 0, b2 = 0;
            SH_CHECK(rocprim::radix_sort_keys(nullptr, b1, e->d_buf, e->d_alt, total, 0, 64, s) == hipSuccess &&
                     rocprim::unique(nullptr, b2, e->d_alt, e->d_buf, e->d_ctr + 1, total, rocprim::equal_to<uint64_t>(), s) == hipSuccess &&
                     b_tmp2.alloc(std::max<size_t>(std::max(b1, b2), 1)) == hipSuccess, SH_ERR_OOM, "estimator: scratch allocation failed");
            unsigned long long uniq = 0;
            SH_CHECK(rocprim::radix_sort_keys(b_tmp2.p, b1, e->d_buf, e->d_alt, total, 0, 64, s) == hipSuccess &&
                     rocprim::unique(b_tmp2.p, b2, e->d_alt, e->d_buf, e->d_ctr + 1, total, rocprim::equal_to<uint64_t>(), s) == hipSuccess &&
                     hipMemcpyAsync(&uniq, e->d_ctr + 1, 8, hipMemcpyDeviceToHost, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess,
                     SH_ERR_HIP, "estimator: sort failed");
            e->n_have = uniq;
        }
        break;
    }
    if (n_sampled) *n_sampled = e->n_have;
    return SH_OK;
}

// ---- per-k-mer codes of a library batch (DESIGN.md §7 "Abundance re-estimation"; the windows over them: sh_k2_distrib.hip) ----
// The work items and the character loop of k2_lib_scan, in a copy of its own: this caller needs every k-mer, not only the first
// of a run, and the ambiguous ones too, and the two build kernels keep the code they had.  Consecutive k-mers with one minimizer
// share one probe; a segment's first valid k-mer probes whatever the segment before it ended with (the code is a function of the
// minimizer alone, so the repeated probe changes no answer: it costs one lookup per 1024 bases).
template <int W>
__global__ __launch_bounds__(64) void k_k2_codes_lib(K2LibArgs a, K2Table T, uint32_t *codes, uint64_t cap, unsigned long long *need)
{
    const uint32_t lane = threadIdx.x;
    const uint64_t n_bases = a.offsets[a.n_records];
    if (n_bases > cap) {        // the scratch is too small for this batch: say how much it takes, write nothing
        if (blockIdx.x == 0 && lane == 0) *need = n_bases;
        return;
    }
    const uint64_t lmask = a.l < 32 ? ((1ULL << (2 * a.l)) - 1) : ~0ULL;
    const int32_t wlim = a.k - a.l + 1;
    const uint64_t n_items = a.seg_off[a.n_records];
    for (uint64_t base = (uint64_t)blockIdx.x * 64; base < n_items; base += (uint64_t)gridDim.x * 64) {
        const uint64_t item = base + lane;
        int32_t n = 0, lead = 0;
        const uint8_t *p = a.bases;
        uint64_t d0 = 0;                 // the k-mer that ends at the segment's character i (i >= k - 1) has its code at codes[d0 + i - (k - 1)]
        if (item < n_items) {
            uint64_t lo = 0, hi = a.n_records;
            while (hi - lo > 1) { const uint64_t mid = (lo + hi) >> 1; if (a.seg_off[mid] <= item) lo = mid; else hi = mid; }
            const uint64_t r0 = a.offsets[lo], len = a.offsets[lo + 1] - r0;
            const uint64_t s0 = (item - a.seg_off[lo]) * a.seg, s1 = s0 + a.seg < len ? s0 + a.seg : len;
            const uint64_t from = s0 >= (uint64_t)(a.k - 1) ? s0 - (uint64_t)(a.k - 1) : 0;
            p = a.bases + r0 + from; n = (int32_t)(s1 - from); lead = (int32_t)(s0 - from);
            d0 = r0 + from;
        }
        int32_t n_max = n;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { const int32_t t = __shfl_xor(n_max, o); n_max = t > n_max ? t : n_max; }
        const uint64_t *wp = (const uint64_t *)((uintptr_t)p & ~(uintptr_t)7);
        const int32_t off8 = (int32_t)((uintptr_t)p & 7); const uint32_t sh = (uint32_t)off8 * 8;
        uint64_t w_cur = n > 0 ? wp[0] : 0, w_next = n + off8 > 8 ? wp[1] : 0;
        K2Scan<W> S; S.reset();
        uint64_t last = 0; bool have = false; uint32_t taxon = 0;
        const int32_t n_chunks = (n_max + 7) / 8;
#pragma nounroll
        for (int32_t c = 0; c < n_chunks; ++c) {
            uint64_t w = sh ? (w_cur >> sh) | (w_next << (64 - sh)) : w_cur;
            w_cur = w_next;
            w_next = (c + 2) * 8 < n + off8 ? wp[c + 2] : 0;
#pragma nounroll
            for (int32_t j = 0; j < 8; ++j) {
                const int32_t i = c * 8 + j;
                uint64_t m;
                const int ev = S.step_w(sh_nt4((uint32_t)w & 0xffu), i + 1 < a.k ? i + 1 : a.k, a.k, a.l, lmask, a.spaced, a.toggle, m, wlim);
                w >>= 8;
                if (ev == 0 || i >= n || i < lead) continue;
                if (ev == 2 && !(have && m == last)) {
                    const uint64_t hc = k2_fmix64(m);
                    taxon = a.min_hash && hc < a.min_hash ? 0u : k2_probe(T, hc);
                    taxon = taxon < a.n_nodes ? taxon : 0u;       // a cell value outside the taxonomy counts for nobody
                    last = m; have = true;
                }
                codes[d0 + (uint64_t)(i - (a.k - 1))] = ev == 2 ? taxon : SH_K2_HIT_AMBIGUOUS;
            }
        }
    }
}

sh_status shi_k2_codes_device(const sh_k2_db *db, const uint8_t *d_bases, const uint64_t *d_offsets, const uint32_t *d_taxa, uint64_t n_records,
                              uint64_t *d_seg, DevBuf &tmp, uint32_t *d_codes, uint64_t codes_cap, unsigned long long *d_need, hipStream_t s)
{
    K2LibArgs a{};
    a.n_nodes = (uint32_t)db->nodes.size();
    sh_status st = k2_lib_prepare(a, db->opts, d_bases, d_offsets, d_taxa, n_records, d_seg, tmp, s);
    if (st != SH_OK) return st;
    const K2Table T{db->d_cells, db->capacity, db->value_bits, 1.0 / (double)db->capacity};
    k2_with_window(db->opts.k, db->opts.l, [&](auto w) {
        hipLaunchKernelGGL(k_k2_codes_lib<decltype(w)::value>, dim3(K2_LIB_GRID), dim3(64), 0, s, a, T, d_codes, codes_cap, d_need);
    });
    return SH_OK;
}

extern "C" sh_status sh_k2_info_get(const sh_k2_db *db, sh_k2_info *o)
{
    SH_CHECK(db && o, SH_ERR_BAD_ARG, "sh_k2_info_get: null argument");
    o->capacity = db->capacity; o->size = db->size; o->n_nodes = db->nodes.size();
    o->hbm_bytes = db->capacity * 4 + db->nodes.size() * 8;
    o->k = db->opts.k; o->l = db->opts.l; o->value_bits = db->value_bits; o->key_bits = db->key_bits;
    return SH_OK;
}

extern "C" sh_status sh_k2_db_opts(const sh_k2_db *db, sh_k2_opts *o)
{
    SH_CHECK(db && o, SH_ERR_BAD_ARG, "sh_k2_db_opts: null argument");
    *o = db->opts;
    o->long_unit_bases = 0;
    return SH_OK;
}

extern "C" sh_status sh_k2_export(const sh_k2_db *db, uint32_t *cells, uint32_t *parent, uint32_t *external)
{
    SH_CHECK(db, SH_ERR_BAD_ARG, "sh_k2_export: null argument");
    SH_HIP(hipSetDevice(db->device));
    if (cells) SH_HIP(hipMemcpy(cells, db->d_cells, db->capacity * 4, hipMemcpyDeviceToHost));
    if (parent) SH_HIP(hipMemcpy(parent, db->d_parent, db->nodes.size() * 4, hipMemcpyDeviceToHost));
    if (external) SH_HIP(hipMemcpy(external, db->d_ext, db->nodes.size() * 4, hipMemcpyDeviceToHost));
    return SH_OK;
}

// ---- database files (SURVEY.md App. B "DB files") --------------------------------------------------------------------
struct K2OptsFile {         // opts.k2d: the index options struct as written by the builder (64 B with padding)
    uint64_t k, l, spaced_seed_mask, toggle_mask;
    uint8_t dna_db; uint8_t pad0[7];
    uint64_t minimum_acceptable_hash_value;
    int32_t revcom_version, db_version, db_type, pad1;
};
static_assert(sizeof(K2OptsFile) == 64, "opts.k2d layout");

extern "C" sh_status sh_k2_save(const sh_k2_db *db, const char *dir)
{
    SH_CHECK(db && dir, SH_ERR_BAD_ARG, "sh_k2_save: null argument");
    SH_HIP(hipSetDevice(db->device));
    const std::string d = dir;
    {
        K2OptsFile of{};
        of.k = (uint64_t)db->opts.k; of.l = (uint64_t)db->opts.l; of.spaced_seed_mask = db->opts.spaced_seed_mask; of.toggle_mask = db->opts.toggle_mask;
        of.dna_db = (uint8_t)db->dna_db; of.minimum_acceptable_hash_value = db->opts.min_acceptable_hash;
        of.revcom_version = db->revcom_version; of.db_version = db->db_version; of.db_type = db->db_type;
        FILE *f = fopen((d + "/opts.k2d").c_str(), "wb");
        SH_CHECK(f, SH_ERR_IO, "cannot write %s/opts.k2d", dir);
        bool ok = fwrite(&of, sizeof(of), 1, f) == 1;
        ok = fclose(f) == 0 && ok;
        SH_CHECK(ok, SH_ERR_IO, "short write to %s/opts.k2d", dir);
    }
    {
        FILE *f = fopen((d + "/taxo.k2d").c_str(), "wb");
        SH_CHECK(f, SH_ERR_IO, "cannot write %s/taxo.k2d", dir);
        const uint64_t hdr[3] = {db->nodes.size(), db->names.size(), db->ranks.size()};
        bool ok = fwrite("K2TAXDAT", 8, 1, f) == 1 && fwrite(hdr, 8, 3, f) == 3;
        ok = ok && fwrite(db->nodes.data(), sizeof(sh_k2_taxnode), db->nodes.size(), f) == db->nodes.size();
        ok = ok && (db->names.empty() || fwrite(db->names.data(), 1, db->names.size(), f) == db->names.size());
        ok = ok && (db->ranks.empty() || fwrite(db->ranks.data(), 1, db->ranks.size(), f) == db->ranks.size());
        ok = fclose(f) == 0 && ok;
        SH_CHECK(ok, SH_ERR_IO, "short write to %s/taxo.k2d", dir);
    }
    {
        FILE *f = fopen((d + "/hash.k2d").c_str(), "wb");
        SH_CHECK(f, SH_ERR_IO, "cannot write %s/hash.k2d", dir);
        const uint64_t hdr[4] = {db->capacity, db->size, (uint64_t)db->key_bits, (uint64_t)db->value_bits};
        bool ok = fwrite(hdr, 8, 4, f) == 4;
        const uint64_t CH = 64ull << 20;            // cells per copy
        std::vector<uint32_t> buf(std::min(CH, db->capacity));
        for (uint64_t o = 0; ok && o < db->capacity; o += CH) {
            const uint64_t m = std::min(CH, db->capacity - o);
            if (hipMemcpy(buf.data(), db->d_cells + o, m * 4, hipMemcpyDeviceToHost) != hipSuccess) { fclose(f); sh_set_error("copy of the table failed"); return SH_ERR_HIP; }
            ok = fwrite(buf.data(), 4, m, f) == m;
        }
        ok = fclose(f) == 0 && ok;
        SH_CHECK(ok, SH_ERR_IO, "short write to %s/hash.k2d", dir);
    }
    return SH_OK;
}

extern "C" sh_status sh_k2_open(const char *dir, int device, sh_k2_db **out)
{
    SH_CHECK(dir && out, SH_ERR_BAD_ARG, "sh_k2_open: null argument");
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= device) { sh_set_error("no HIP device %d", device); return SH_ERR_NO_DEVICE; }
    SH_HIP(hipSetDevice(device));
    const std::string d = dir;
    sh_k2_db *db = new sh_k2_db;
    db->device = device;
    auto fail = [&](sh_status st) { sh_k2_free(db); return st; };
    {
        FILE *f = fopen((d + "/opts.k2d").c_str(), "rb");
        if (!f) { sh_set_error("cannot open %s/opts.k2d", dir); return fail(SH_ERR_IO); }
        K2OptsFile of{};
        const size_t got = fread(&of, 1, sizeof(of), f);        // older databases wrote a shorter struct: the rest stays zero
        fclose(f);
        if (got < 32) { sh_set_error("%s/opts.k2d is truncated", dir); return fail(SH_ERR_IO); }
        sh_k2_default_opts(&db->opts);
        db->opts.k = (int32_t)of.k; db->opts.l = (int32_t)of.l; db->opts.spaced_seed_mask = of.spaced_seed_mask; db->opts.toggle_mask = of.toggle_mask;
        db->opts.min_acceptable_hash = got >= 48 ? of.minimum_acceptable_hash_value : 0;
        db->dna_db = got >= 33 ? of.dna_db : 1; db->revcom_version = got >= 52 ? of.revcom_version : 0;
        db->db_version = got >= 56 ? of.db_version : 0; db->db_type = got >= 60 ? of.db_type : 0;
        db->opts.protein = !db->dna_db;
        if (!k2_kl_ok(db->opts)) {
            sh_set_error("%s: unsupported k=%d l=%d for a %s database", dir, db->opts.k, db->opts.l, k2_kind(db->opts.protein)); return fail(SH_ERR_BAD_ARG);
        }
    }
    {
        FILE *f = fopen((d + "/taxo.k2d").c_str(), "rb");
        if (!f) { sh_set_error("cannot open %s/taxo.k2d", dir); return fail(SH_ERR_IO); }
        char magic[8]; uint64_t hdr[3];
        bool ok = fread(magic, 8, 1, f) == 1 && memcmp(magic, "K2TAXDAT", 8) == 0 && fread(hdr, 8, 3, f) == 3;
        if (ok) {
            db->nodes.resize(hdr[0]); db->names.resize(hdr[1]); db->ranks.resize(hdr[2]);
            ok = fread(db->nodes.data(), sizeof(sh_k2_taxnode), hdr[0], f) == hdr[0];
            ok = ok && (hdr[1] == 0 || fread(&db->names[0], 1, hdr[1], f) == hdr[1]);
            ok = ok && (hdr[2] == 0 || fread(&db->ranks[0], 1, hdr[2], f) == hdr[2]);
        }
        fclose(f);
        if (!ok || db->nodes.size() < 2) { sh_set_error("%s/taxo.k2d is not a Kraken 2 taxonomy", dir); return fail(SH_ERR_IO); }
    }
    {
        FILE *f = fopen((d + "/hash.k2d").c_str(), "rb");
        if (!f) { sh_set_error("cannot open %s/hash.k2d", dir); return fail(SH_ERR_IO); }
        uint64_t hdr[4];
        if (fread(hdr, 8, 4, f) != 4 || hdr[0] == 0 || hdr[2] + hdr[3] != 32 || hdr[3] < 1 || hdr[3] > 31) { fclose(f); sh_set_error("%s/hash.k2d: bad header", dir); return fail(SH_ERR_IO); }
        db->capacity = hdr[0]; db->size = hdr[1]; db->key_bits = (int32_t)hdr[2]; db->value_bits = (int32_t)hdr[3]; db->opts.value_bits = db->value_bits;
        hipError_t e = hipMalloc(&db->d_cells, db->capacity * 4);
        if (e != hipSuccess) { fclose(f); sh_set_error("table of %llu cells: %s", (unsigned long long)db->capacity, hipGetErrorString(e)); return fail(SH_ERR_OOM); }
        const uint64_t CH = 64ull << 20;
        std::vector<uint32_t> buf(std::min(CH, db->capacity));
        for (uint64_t o = 0; o < db->capacity; o += CH) {
            const uint64_t m = std::min(CH, db->capacity - o);
            if (fread(buf.data(), 4, m, f) != m) { fclose(f); sh_set_error("%s/hash.k2d is truncated", dir); return fail(SH_ERR_IO); }
            if (hipMemcpy(db->d_cells + o, buf.data(), m * 4, hipMemcpyHostToDevice) != hipSuccess) { fclose(f); sh_set_error("copy to HBM failed"); return fail(SH_ERR_HIP); }
        }
        fclose(f);
    }
    if (db->nodes.size() > (1ull << db->value_bits)) { sh_set_error("%s: taxonomy larger than the table's value range", dir); return fail(SH_ERR_BAD_ARG); }
    sh_status st = k2_upload_taxonomy(db);
    if (st != SH_OK) return fail(st);
    *out = db;
    return SH_OK;
}

// ---- classification ---------------------------------------------------------------------------------------------------
// one form of the kernel; the window, QMASK and (for a pass-1 form) MIND become compile-time constants here
template <bool BIG, bool QUICK, int HITS>
static void launch_classify(const K2MArgs &a, uint64_t n_work, hipStream_t s, bool qmask, bool mind, bool sub)
{
    const uint32_t grid = (uint32_t)std::min<uint64_t>(std::max<uint64_t>((n_work + 63) / 64, 1), 256 * 32);
    k2_with_window(a.k, a.l, [&](auto w) {
        k2_with_flag(qmask, [&](auto q) {
            k2_with_flag(mind, [&](auto m) {
                k2_with_flag(sub, [&](auto sb) {
                    constexpr bool QMASK = decltype(q)::value, MIND = decltype(m)::value && !(BIG || HITS == 2);
                    constexpr bool SUB = decltype(sb)::value && !(BIG || QUICK || HITS == 2);
                    const K2ArgsOf<QMASK, HITS, MIND> &ka = a;
                    hipLaunchKernelGGL((k_k2_classify<decltype(w)::value, BIG, QMASK, QUICK, HITS, MIND, SUB>), dim3(grid), dim3(64), 0, s, ka);
                });
            });
        });
    });
}
// only the instances that are needed: a QUICK unit keeps no hit list, so it never overflows into the BIG pass; the BIG pass
// needs no HITS instance (pass 1 already emitted the whole list of a unit with many taxa); MIND goes with the three pass-1
// forms only (the two redo passes are never asked for it: their units were counted by pass 1)
enum K2Form { K2F_PLAIN, K2F_QUICK, K2F_HITS1, K2F_HITS2, K2F_BIG };
// sub: a pass-1 form over a.unit_list (the units the wave route left)
static void dispatch_classify(K2Form form, const K2MArgs &a, uint64_t n_work, hipStream_t s, bool qmask, bool mind = false, bool sub = false)
{
    switch (form) {
    case K2F_PLAIN: launch_classify<false, false, 0>(a, n_work, s, qmask, mind, sub); break;
    case K2F_QUICK: launch_classify<false, true, 0>(a, n_work, s, qmask, mind, false); break;
    case K2F_HITS1: launch_classify<false, false, 1>(a, n_work, s, qmask, mind, sub); break;
    case K2F_HITS2: launch_classify<false, false, 2>(a, n_work, s, qmask, false, false); break;
    case K2F_BIG: launch_classify<true, false, 0>(a, n_work, s, qmask, false, false); break;
    }
}

// translated search: the two forms a protein database has (pass 1 over every unit, BIG over a.unit_list)
template <bool BIG>
static void launch_classify_prot(const K2MArgs &a, uint64_t n_work, hipStream_t s)
{
    const uint32_t grid = (uint32_t)std::min<uint64_t>(std::max<uint64_t>((n_work + 63) / 64, 1), 256 * 32);
    k2_with_window_aa(a.k, a.l, [&](auto w) {
        const K2Args &ka = a;
        hipLaunchKernelGGL((k_k2_classify<decltype(w)::value, BIG, false, false, 0, false, false, true>), dim3(grid), dim3(64), 0, s, ka);
    });
}

// the wave route's forms (PLAIN, HITS1, HITS2) over a.unit_list: one block of 64 threads per unit in flight, units drawn by ticket
#define K2_WAVE_GRID 2048u      // 8 waves per CU; each block owns a 64-KiB spill table
template <int HITS>
static void launch_classify_wave(const K2MArgs &a, const K2Wave &wv, hipStream_t s, bool qmask, bool mind)
{
    const uint32_t grid = std::min<uint32_t>(std::max<uint32_t>(a.n_list, 1), K2_WAVE_GRID);
    k2_with_window(a.k, a.l, [&](auto w) {
        k2_with_flag(qmask, [&](auto q) {
            k2_with_flag(mind, [&](auto m) {
                constexpr bool QMASK = decltype(q)::value, MIND = decltype(m)::value && HITS != 2;
                const K2ArgsOf<QMASK, HITS, MIND> &ka = a;
                hipLaunchKernelGGL((k_k2_classify_wave<decltype(w)::value, QMASK, HITS, MIND>), dim3(grid), dim3(64), 0, s, ka, wv);
            });
        });
    });
}
static void dispatch_classify_wave(K2Form form, const K2MArgs &a, const K2Wave &wv, hipStream_t s, bool qmask, bool mind = false)
{
    switch (form) {
    case K2F_HITS1: launch_classify_wave<1>(a, wv, s, qmask, mind); break;
    case K2F_HITS2: launch_classify_wave<2>(a, wv, s, qmask, false); break;
    default: launch_classify_wave<0>(a, wv, s, qmask, mind); break;
    }
}

extern "C" uint32_t sh_k2_wave_tile(void) { return K2_WAVE_TILE; }

// opts.long_unit_bases resolved: the wave route's threshold in bases, 0 = no unit takes it
#define K2_LONG_DEFAULT 8192      // measured choice: DESIGN.md §7 "Long reads"
static uint64_t k2_long_threshold(const sh_k2_opts &o)
{
    if (o.quick || o.long_unit_bases < 0 || (o.long_unit_bases == 0 && K2_LONG_DEFAULT < 0)) return 0;
    return o.long_unit_bases ? (uint64_t)o.long_unit_bases : (uint64_t)K2_LONG_DEFAULT;
}
// the units of a batch that take the wave route
struct K2IsLong {
    const uint64_t *off; int32_t paired; uint64_t thr;
    __host__ __device__ bool operator()(uint32_t u) const
    {
        if (!paired) return off[u + 1] - off[u] >= thr;
        const uint64_t l0 = off[2 * (uint64_t)u + 1] - off[2 * (uint64_t)u], l1 = off[2 * (uint64_t)u + 2] - off[2 * (uint64_t)u + 1];
        return (l0 > l1 ? l0 : l1) >= thr;
    }
};
// how many there are: the cheap question first, so that a batch without one pays for no list
#define K2C_NLONG 7
__global__ void k_k2_count_long(K2IsLong is_long, uint64_t n_units, unsigned long long *out)
{
    unsigned long long n = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_units; i += (uint64_t)gridDim.x * blockDim.x) n += is_long((uint32_t)i);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += (unsigned long long)__shfl_xor((long long)n, o);
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(out, n);
}

// the hit lists of one call (sh_k2_classify_ex_* with hits): per-unit offsets and the entries, compacted, in HBM
struct sh_k2_hits {
    int device = 0;
    uint64_t n_units = 0, n_entries = 0, n_redone = 0;
    uint64_t *d_off = nullptr;           // n_units + 1
    sh_k2_hit *d_ent = nullptr;          // n_entries
};

// units whose list fits inline: their entries to the final offsets (the others were written there by the HITS 2 pass)
__global__ void k_k2_hits_compact(const uint2 *inl, const uint32_t *n_hits, const uint64_t *off, uint64_t n_units, uint2 *out)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_units * K2_HIT_INLINE; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t u = i / K2_HIT_INLINE; const uint32_t j = (uint32_t)(i % K2_HIT_INLINE);
        const uint32_t n = n_hits[u];
        if (n <= K2_HIT_INLINE && j < n) out[off[u] + j] = inl[i];
    }
}

// ---- minimizer data: the accumulator of one database and its three small kernels --------------------------------------
struct sh_k2_mindata {
    int device = 0;
    uint64_t n_nodes = 0;
    uint32_t *d_parent = nullptr;                // a copy: the accumulator may outlive the database handle
    uint32_t *d_regs = nullptr;                  // n_nodes * K2_MD_WORDS
    unsigned long long *d_cnt = nullptr;         // n_nodes
    // the clade values, made by the first read-out after a classify call or a reset
    uint32_t *d_clade_regs = nullptr; unsigned long long *d_clade_cnt = nullptr;
    uint32_t *d_hist = nullptr;                  // 2 * n_nodes * K2_MD_BINS: own, then clade
    bool clade_valid = false;
};

__global__ void k_k2_md_clear(uint4 *p, uint64_t n16)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (uint64_t)gridDim.x * blockDim.x) p[i] = make_uint4(0, 0, 0, 0);
}

// Clade values: block t carries taxon t's own registers and count to itself and every ancestor (internal ids are breadth-first,
// so the walk over parent[] only descends in id and ends at the root, id 1).  Only a taxon with data pushes anything.  The
// clade buffers start cleared; a word is read first and CASed only where a byte grows, as in the classifier.
__global__ __launch_bounds__(256) void k_k2_md_clade(const uint32_t *__restrict__ parent, uint32_t n_nodes, const uint32_t *__restrict__ regs,
                                                     const unsigned long long *__restrict__ cnt, uint32_t *clade_regs, unsigned long long *clade_cnt)
{
    for (uint32_t t = blockIdx.x + 1; t < n_nodes; t += gridDim.x) {
        const unsigned long long c = cnt[t];
        if (!c) continue;
        uint32_t mine[K2_MD_WORDS / 256];
#pragma unroll
        for (uint32_t j = 0; j < K2_MD_WORDS / 256; ++j) mine[j] = regs[(uint64_t)t * K2_MD_WORDS + j * 256 + threadIdx.x];
        uint32_t x = t;
        for (uint32_t depth = 0; depth < n_nodes; ++depth) {      // (the bound only guards against a parent array with a cycle)
            if (threadIdx.x == 0) atomicAdd(&clade_cnt[x], c);
#pragma unroll
            for (uint32_t j = 0; j < K2_MD_WORDS / 256; ++j) {
                uint32_t *w = clade_regs + (uint64_t)x * K2_MD_WORDS + j * 256 + threadIdx.x;
                uint32_t cur = __atomic_load_n(w, __ATOMIC_RELAXED);
                for (;;) {
                    const uint32_t nw = k2_md_max4(cur, mine[j]);
                    if (nw == cur) break;
                    const uint32_t prev = atomicCAS(w, cur, nw);
                    if (prev == cur) break;
                    cur = prev;
                }
            }
            const uint32_t up = parent[x];
            if (x <= 1 || up == 0 || up >= x) break;
            x = up;
        }
    }
}

// Register histogram (the estimator's input): one block per taxon with data, K2_MD_BINS bins
__global__ __launch_bounds__(256) void k_k2_md_hist(uint32_t n_nodes, const uint32_t *__restrict__ regs, const unsigned long long *__restrict__ cnt, uint32_t *hist)
{
    __shared__ uint32_t s_h[K2_MD_BINS];
    for (uint32_t t = blockIdx.x + 1; t < n_nodes; t += gridDim.x) {
        if (!cnt[t]) continue;                    // (block-uniform)
        if (threadIdx.x < K2_MD_BINS) s_h[threadIdx.x] = 0;
        __syncthreads();
        for (uint32_t j = threadIdx.x; j < K2_MD_WORDS; j += 256) {
            const uint32_t w = regs[(uint64_t)t * K2_MD_WORDS + j];
#pragma unroll
            for (int b = 0; b < 32; b += 8) { const uint32_t r = (w >> b) & 0xffu; atomicAdd(&s_h[r < K2_MD_BINS ? r : K2_MD_BINS - 1], 1u); }
        }
        __syncthreads();
        if (threadIdx.x < K2_MD_BINS) hist[(uint64_t)t * K2_MD_BINS + threadIdx.x] = s_h[threadIdx.x];
        __syncthreads();
    }
}

extern "C" sh_status sh_k2_hits_count(const sh_k2_hits *h, uint64_t *n_units, uint64_t *n_entries, uint64_t *n_redone)
{
    SH_CHECK(h, SH_ERR_BAD_ARG, "sh_k2_hits_count: null argument");
    if (n_units) *n_units = h->n_units;
    if (n_entries) *n_entries = h->n_entries;
    if (n_redone) *n_redone = h->n_redone;
    return SH_OK;
}

extern "C" sh_status sh_k2_hits_device(const sh_k2_hits *h, const uint64_t **d_offsets, const sh_k2_hit **d_entries)
{
    SH_CHECK(h, SH_ERR_BAD_ARG, "sh_k2_hits_device: null argument");
    if (d_offsets) *d_offsets = h->d_off;
    if (d_entries) *d_entries = h->d_ent;
    return SH_OK;
}

extern "C" sh_status sh_k2_hits_copy(const sh_k2_hits *h, uint64_t *offsets, sh_k2_hit *entries)
{
    SH_CHECK(h, SH_ERR_BAD_ARG, "sh_k2_hits_copy: null argument");
    SH_HIP(hipSetDevice(h->device));
    if (offsets && h->d_off) SH_HIP(hipMemcpy(offsets, h->d_off, (h->n_units + 1) * 8, hipMemcpyDeviceToHost));
    else if (offsets) offsets[0] = 0;
    if (entries && h->n_entries) SH_HIP(hipMemcpy(entries, h->d_ent, h->n_entries * sizeof(sh_k2_hit), hipMemcpyDeviceToHost));
    return SH_OK;
}

extern "C" sh_status sh_k2_hits_free(sh_k2_hits *h)
{
    if (!h) return SH_OK;
    hipSetDevice(h->device);
    hipFree(h->d_off); hipFree(h->d_ent);
    delete h;
    return SH_OK;
}

// the handle a classify call is filling: the caller gets it only from a call that succeeds
struct K2HitsOwner {
    sh_k2_hits *h = nullptr;
    ~K2HitsOwner() { sh_k2_hits_free(h); }
    sh_k2_hits *release() { sh_k2_hits *r = h; h = nullptr; return r; }
};

// what both entries reach: the checks they share, the passes, the copy of the results to host_out (nullable: the host entry's),
// and *hits_out (nullable), which is NULL after any failure
static sh_status k2_classify(const sh_k2_db *db, const sh_k2_opts *opts, const uint8_t *d_bases, const uint8_t *d_quals, const uint64_t *d_offsets,
                             uint64_t n_records, int32_t paired, sh_k2_result *d_out, sh_k2_result *host_out, void *stream, sh_k2_stats *stats,
                             sh_k2_hits **hits_out, sh_k2_mindata *md, bool may_be_long = true)
{
    if (hits_out) *hits_out = nullptr;
    SH_CHECK(db && d_offsets && d_out && (d_bases || n_records == 0), SH_ERR_BAD_ARG, "sh_k2_classify_ex: null argument");
    SH_CHECK(!md || (md->device == db->device && md->n_nodes == db->nodes.size()), SH_ERR_BAD_ARG, "the minimizer data belongs to another database");
    SH_CHECK(!paired || (n_records & 1) == 0, SH_ERR_BAD_ARG, "paired input needs an even number of records (got %llu)", (unsigned long long)n_records);
    const sh_k2_opts &o = opts ? *opts : db->opts;
    K2_CHECK_KIND(db, o, "sh_k2_classify_ex");
    const bool prot = db->opts.protein != 0;
    // what translated search leaves out (DESIGN.md §7 "Translated search")
    SH_CHECK(!prot || !o.quick, SH_ERR_BAD_ARG, "--quick is not supported on a protein database");
    SH_CHECK(!prot || !hits_out, SH_ERR_BAD_ARG, "hit lists are not supported on a protein database: call with hits = NULL");
    SH_CHECK(!prot || !md, SH_ERR_BAD_ARG, "minimizer data is not supported on a protein database: call with md = NULL");
    SH_CHECK(!hits_out || !o.quick, SH_ERR_BAD_ARG, "--quick writes no hit list: call with hits = NULL");
    SH_HIP(hipSetDevice(db->device));
    hipStream_t s = (hipStream_t)stream;
    SH_CHECK(o.k == db->opts.k && o.l == db->opts.l, SH_ERR_BAD_ARG, "options disagree with the database (k, l)");
    // a protein database: the qualities mask at translation, the classify kernel sees codes only
    const bool qmask_any = d_quals && o.min_base_quality > 0, qmask = qmask_any && !prot, quick = o.quick != 0;
    SH_CHECK(!qmask || ((uintptr_t)d_quals & 7) == ((uintptr_t)d_bases & 7), SH_ERR_BAD_ARG,
             "sh_k2_classify_ex_device: qualities and bases must lie at the same address modulo 8");
    const uint64_t n_units = paired ? n_records / 2 : n_records;
    if (stats) memset(stats, 0, sizeof(*stats));
    K2HitsOwner hl;
    if (hits_out) { hl.h = new sh_k2_hits; hl.h->device = db->device; }
    if (n_units == 0) { if (hits_out) *hits_out = hl.release(); return SH_OK; }
    SH_CHECK(n_units <= 0xffffffffull, SH_ERR_BAD_ARG, "at most 2^32 - 1 units per call");
    DevEvent e0, e1;
    SH_HIP(e0.create()); SH_HIP(e1.create());
    DevBuf b_ctr, b_over, b_hit_inl, b_n_hits, b_hit_over, b_big_tax, b_big_cnt, b_split, b_n_long, b_spill, b_whit_over, b_codes;
    DevEvent e2, e3, et0, et1;
    SH_HIP(b_ctr.alloc(K2C_WORDS * 8));
    SH_HIP(b_over.alloc(n_units * 4));
    unsigned long long *ctr = b_ctr.as<unsigned long long>();
    SH_HIP(hipMemsetAsync(ctr, 0, K2C_WORDS * 8, s));
    K2MArgs a{};
    if (md) { a.md_regs = md->d_regs; a.md_cnt = md->d_cnt; md->clade_valid = false; }
    if (hits_out) {       // pass 1: K2_HIT_INLINE entries per unit in place, every unit's count (one spare: the scan's total)
        SH_HIP(b_hit_inl.alloc(n_units * K2_HIT_INLINE * sizeof(uint2)));
        SH_HIP(b_n_hits.alloc((n_units + 1) * 4));
        SH_HIP(b_hit_over.alloc(n_units * 4));
        a.hits = b_hit_inl.as<uint2>(); a.n_hits = b_n_hits.as<uint32_t>(); a.hit_over = b_hit_over.as<uint32_t>();
        SH_HIP(hipMemsetAsync(a.n_hits + n_units, 0, 4, s));
    }
    a.bases = d_bases; a.offsets = d_offsets; a.n_units = n_units; a.paired = paired;
    a.T = K2Table{db->d_cells, db->capacity, db->value_bits, 1.0 / (double)db->capacity}; a.parent = db->d_parent; a.ext = db->d_ext; a.n_nodes = (uint32_t)db->nodes.size();
    a.k = o.k; a.l = o.l; a.spaced = o.spaced_seed_mask; a.toggle = o.toggle_mask; a.min_hash = o.min_acceptable_hash;
    a.min_hit_groups = o.min_hit_groups; a.confidence = o.confidence;
    a.out = d_out; a.over_list = b_over.as<uint32_t>(); a.ctr = ctr;
    a.quals = qmask ? d_quals : nullptr; a.min_qual = qmask ? o.min_base_quality : 0;
    // the split: are there long units at all (one pass over the offsets, an 8-byte read-back); if so, the long units first in b_split
    // (by unit), the others behind them (last unit first: rocprim::partition's layout).  Nothing of it when no unit can be long
    const uint64_t long_thr = may_be_long && !prot ? k2_long_threshold(o) : 0;      // a protein database: every unit takes the lane route
    uint64_t n_long = 0;
    K2Wave wv{};
    if (long_thr) {
        const K2IsLong is_long{d_offsets, paired, long_thr};
        unsigned long long n_counted = 0;
        hipLaunchKernelGGL(k_k2_count_long, dim3((uint32_t)std::min<uint64_t>((n_units + 255) / 256, 1024)), dim3(256), 0, s, is_long, n_units, ctr + K2C_NLONG);
        SH_HIP(hipMemcpyAsync(&n_counted, ctr + K2C_NLONG, 8, hipMemcpyDeviceToHost, s));
        SH_HIP(hipStreamSynchronize(s));
        n_long = n_counted;
    }
    if (n_long) {
        SH_HIP(b_split.alloc(n_units * 4));
        SH_HIP(b_n_long.alloc(8));
        size_t tmp_bytes = 0; DevBuf tmp;      // (the partition's own count lands in b_n_long: the same number)
        const K2IsLong is_long{d_offsets, paired, long_thr};
        SH_HIP(rocprim::partition(nullptr, tmp_bytes, rocprim::counting_iterator<uint32_t>(0), b_split.as<uint32_t>(), b_n_long.as<size_t>(), (size_t)n_units, is_long, s));
        SH_HIP(tmp.alloc(std::max<size_t>(tmp_bytes, 1)));
        SH_HIP(rocprim::partition(tmp.p, tmp_bytes, rocprim::counting_iterator<uint32_t>(0), b_split.as<uint32_t>(), b_n_long.as<size_t>(), (size_t)n_units, is_long, s));
    }
    if (n_long) {
        const uint64_t grid = std::min<uint64_t>(n_long, K2_WAVE_GRID);
        SH_HIP(b_spill.alloc(grid * K2_WS_SLOTS * 8));
        SH_HIP(hipMemsetAsync(b_spill.p, 0, grid * K2_WS_SLOTS * 8, s));
        wv.spill_tax = b_spill.as<uint32_t>(); wv.spill_cnt = wv.spill_tax + grid * K2_WS_SLOTS;
        if (hits_out) { SH_HIP(b_whit_over.alloc(n_long * 4)); wv.hit_over = b_whit_over.as<uint32_t>(); }
        SH_HIP(e2.create()); SH_HIP(e3.create());
    }
    if (prot) {       // the batch's six frames as scanner codes in call-scoped scratch (k_k2_translate); the kernels below read them
        uint64_t ends[2];
        SH_HIP(hipMemcpyAsync(&ends[0], d_offsets, 8, hipMemcpyDeviceToHost, s));
        SH_HIP(hipMemcpyAsync(&ends[1], d_offsets + n_records, 8, hipMemcpyDeviceToHost, s));
        SH_HIP(hipStreamSynchronize(s));
        SH_CHECK(ends[1] >= ends[0], SH_ERR_BAD_ARG, "sh_k2_classify_ex: offsets decrease");
        SH_HIP(b_codes.alloc(2 * (ends[1] - ends[0]) + 8));
        SH_HIP(et0.create()); SH_HIP(et1.create());
        SH_HIP(hipEventRecord(et0.e, s));
        sh_status st = shi_k2_translate_device(d_bases, d_quals, d_offsets, n_records, ends[0], ends[1] - ends[0], qmask_any ? o.min_base_quality : 0, 0, b_codes.as<uint8_t>(), s);
        if (st != SH_OK) return st;
        SH_HIP(hipEventRecord(et1.e, s));
        a.bases = b_codes.as<uint8_t>();
    }
    const K2Form form1 = quick ? K2F_QUICK : hits_out ? K2F_HITS1 : K2F_PLAIN;
    SH_HIP(hipEventRecord(e0.e, s));
    if (qmask_any) hipLaunchKernelGGL(k_k2_count_masked, dim3(1024), dim3(256), 0, s, d_quals, d_offsets, n_records, o.min_base_quality, ctr);
    if (prot) launch_classify_prot<false>(a, n_units, s);
    else if (!n_long) dispatch_classify(form1, a, n_units, s, qmask, md != nullptr);      // the only pass that counts minimizers
    else {       // the long units one wave each, then the others one lane each
        K2MArgs al = a;
        al.unit_list = b_split.as<uint32_t>(); al.n_list = (uint32_t)n_long;
        SH_HIP(hipEventRecord(e2.e, s));
        dispatch_classify_wave(form1, al, wv, s, qmask, md != nullptr);
        SH_HIP(hipEventRecord(e3.e, s));
        if (n_long < n_units) {
            al.unit_list += n_long; al.n_list = (uint32_t)(n_units - n_long);
            dispatch_classify(form1, al, n_units - n_long, s, qmask, md != nullptr, true);
        }
    }
    SH_HIP(hipEventRecord(e1.e, s));
    std::vector<unsigned long long> h(K2C_WORDS);
    SH_HIP(hipMemcpyAsync(h.data(), ctr, K2C_WORDS * 8, hipMemcpyDeviceToHost, s));
    SH_HIP(hipStreamSynchronize(s));
    SH_HIP(hipGetLastError());
    const uint64_t n_over = h[K2C_OVER];
    if (n_over) {       // units with more than K2_HCAP distinct taxa: hit lists in HBM
        SH_HIP(b_big_tax.alloc(n_over * K2_BIG_CAP * 4));
        SH_HIP(b_big_cnt.alloc(n_over * K2_BIG_CAP * 4));
        a.unit_list = a.over_list; a.n_list = (uint32_t)n_over; a.big_tax = b_big_tax.as<uint32_t>(); a.big_cnt = b_big_cnt.as<uint32_t>();
        if (prot) launch_classify_prot<true>(a, n_over, s);
        else dispatch_classify(K2F_BIG, a, n_over, s, qmask);
        SH_HIP(hipMemcpyAsync(h.data(), ctr, K2C_WORDS * 8, hipMemcpyDeviceToHost, s));
        SH_HIP(hipStreamSynchronize(s));
        SH_HIP(hipGetLastError());
    }
    if (hits_out) {
        // exact offsets from the counts, the units with longer lists redone straight into place, the rest compacted
        hl.h->n_units = n_units;
        SH_HIP(hipMalloc(&hl.h->d_off, (n_units + 1) * 8));
        {
            size_t tmp_bytes = 0; DevBuf tmp;
            SH_HIP(rocprim::exclusive_scan(nullptr, tmp_bytes, a.n_hits, hl.h->d_off, (uint64_t)0, n_units + 1, rocprim::plus<uint64_t>(), s));
            SH_HIP(tmp.alloc(std::max<size_t>(tmp_bytes, 1)));
            SH_HIP(rocprim::exclusive_scan(tmp.p, tmp_bytes, a.n_hits, hl.h->d_off, (uint64_t)0, n_units + 1, rocprim::plus<uint64_t>(), s));
            SH_HIP(hipMemcpyAsync(&hl.h->n_entries, hl.h->d_off + n_units, 8, hipMemcpyDeviceToHost, s));
            SH_HIP(hipStreamSynchronize(s));
        }
        SH_HIP(hipMalloc(&hl.h->d_ent, std::max<uint64_t>(hl.h->n_entries, 1) * sizeof(sh_k2_hit)));
        const uint64_t n_hover = h[K2C_HOVER], n_whover = h[K2C_WHOVER];
        if (n_hover) {
            a.unit_list = a.hit_over; a.n_list = (uint32_t)n_hover; a.hits = (uint2 *)hl.h->d_ent; a.hit_off = hl.h->d_off;
            dispatch_classify(K2F_HITS2, a, n_hover, s, qmask);
        }
        if (n_whover) {       // the wave route's long lists
            K2MArgs al = a;
            al.unit_list = wv.hit_over; al.n_list = (uint32_t)n_whover; al.hits = (uint2 *)hl.h->d_ent; al.hit_off = hl.h->d_off;
            dispatch_classify_wave(K2F_HITS2, al, wv, s, qmask);
        }
        const uint64_t n_cp = n_units * K2_HIT_INLINE;
        hipLaunchKernelGGL(k_k2_hits_compact, dim3((uint32_t)std::min<uint64_t>((n_cp + 255) / 256, 65536)), dim3(256), 0, s, b_hit_inl.as<uint2>(), a.n_hits, hl.h->d_off, n_units,
                           (uint2 *)hl.h->d_ent);
        SH_HIP(hipStreamSynchronize(s));
        SH_HIP(hipGetLastError());
        hl.h->n_redone = n_hover + n_whover;
    }
    if (host_out) SH_HIP(hipMemcpy(host_out, d_out, n_units * sizeof(sh_k2_result), hipMemcpyDeviceToHost));
    float ms = 0, ms_long = 0, ms_tx = 0;
    hipEventElapsedTime(&ms, e0.e, e1.e);
    if (n_long) hipEventElapsedTime(&ms_long, e2.e, e3.e);
    if (prot) hipEventElapsedTime(&ms_tx, et0.e, et1.e);
    if (stats) {
        stats->n_units = n_units; stats->n_overflow = n_over + h[K2C_WOVER]; stats->ms_classify = ms; stats->ms_total = ms + ms_tx;
        stats->n_long_units = n_long; stats->ms_long = ms_long; stats->ms_translate = ms_tx;
        for (int i = 0; i < 64; ++i) {
            stats->n_probes += h[K2C_PROBES + i]; stats->n_kmers += h[K2C_KMERS + i]; stats->n_classified += h[K2C_CLASSIFIED + i];
            stats->n_masked_bases += h[K2C_MASKED + i];
        }
    }
    if (hits_out) *hits_out = hl.release();
    return SH_OK;
}

extern "C" sh_status sh_k2_classify_ex_device(const sh_k2_db *db, const sh_k2_opts *opts, const sh_k2_batch *b, sh_k2_result *d_out, void *stream,
                                              sh_k2_stats *stats, sh_k2_hits **hits, sh_k2_mindata *md)
{
    if (hits) *hits = nullptr;
    SH_CHECK(b, SH_ERR_BAD_ARG, "sh_k2_classify_ex_device: null argument");
    return k2_classify(db, opts, b->bases, b->quals, b->offsets, b->n_records, b->paired, d_out, nullptr, stream, stats, hits, md);
}

// the same from host memory: the batch is staged in HBM and the results copied back
extern "C" sh_status sh_k2_classify_ex_batch(const sh_k2_db *db, const sh_k2_opts *opts, const sh_k2_batch *b, sh_k2_result *out, sh_k2_stats *stats,
                                             sh_k2_hits **hits, sh_k2_mindata *md)
{
    if (hits) *hits = nullptr;
    SH_CHECK(db && b && b->offsets && out, SH_ERR_BAD_ARG, "sh_k2_classify_ex_batch: null argument");
    const uint8_t *bases = b->bases, *quals = b->quals; const uint64_t *offsets = b->offsets, n_records = b->n_records;
    // an empty batch stages nothing: k2_classify touches none of its pointers, but makes its checks and the empty hit list
    if (n_records == 0) return k2_classify(db, opts, nullptr, nullptr, offsets, 0, b->paired, out, nullptr, nullptr, stats, hits, md);
    SH_HIP(hipSetDevice(db->device));
    const uint64_t o0 = offsets[0], n_bases = offsets[n_records] - o0;
    const uint64_t n_units = b->paired ? n_records / 2 : n_records;
    // qualities are staged only when they can mask something; both arrays come from hipMalloc, so they share the address mod 8
    const bool want_q = quals && (opts ? *opts : db->opts).min_base_quality > 0;
    DevBuf d_bases, d_quals, d_off, d_out;
    if (want_q) {
        SH_HIP(d_quals.alloc(n_bases + 64));
        SH_HIP(hipMemcpy(d_quals.p, quals + o0, n_bases, hipMemcpyHostToDevice));
        SH_HIP(hipMemset(d_quals.as<uint8_t>() + n_bases, 0xff, 64));
    }
    SH_HIP(d_bases.alloc(n_bases + 64));
    SH_HIP(d_off.alloc((n_records + 1) * 8));
    SH_HIP(d_out.alloc(std::max<uint64_t>(n_units, 1) * sizeof(sh_k2_result)));
    std::vector<uint64_t> rel(n_records + 1);
    for (uint64_t i = 0; i <= n_records; ++i) rel[i] = offsets[i] - o0;
    SH_HIP(hipMemcpy(d_bases.p, bases + o0, n_bases, hipMemcpyHostToDevice));
    SH_HIP(hipMemset(d_bases.as<uint8_t>() + n_bases, 'N', 64));
    SH_HIP(hipMemcpy(d_off.p, rel.data(), (n_records + 1) * 8, hipMemcpyHostToDevice));
    // the host offsets tell whether any unit can take the wave route
    bool any_long = false;
    if (const uint64_t thr = k2_long_threshold(opts ? *opts : db->opts)) {
        const K2IsLong is_long{rel.data(), b->paired, thr};
        for (uint64_t u = 0; u < n_units && !any_long; ++u) any_long = is_long((uint32_t)u);
    }
    return k2_classify(db, opts, d_bases.as<uint8_t>(), d_quals.as<uint8_t>(), d_off.as<uint64_t>(), n_records, b->paired, d_out.as<sh_k2_result>(), out, nullptr,
                       stats, hits, md, any_long);
}

// ---- Kraken-style report (SURVEY.md App. B "Outputs consumed by Scrubby"; parsed by classifier.rs:449-466) -------------
extern "C" sh_status sh_k2_write_report(const sh_k2_db *db, const sh_k2_result *res, uint64_t n_units, const char *path)
{
    SH_CHECK(db && path && (res || n_units == 0), SH_ERR_BAD_ARG, "sh_k2_write_report: null argument");
    const size_t n = db->nodes.size();
    std::vector<uint64_t> direct(n, 0), clade(n, 0);
    uint64_t unclassified = 0;
    for (uint64_t i = 0; i < n_units; ++i) { if (res[i].call && res[i].call < n) ++direct[res[i].call]; else ++unclassified; }
    clade = direct;
    for (size_t i = n - 1; i >= 2; --i) clade[db->nodes[i].parent] += clade[i];      // parents have smaller ids
    FILE *f = fopen(path, "w");
    SH_CHECK(f, SH_ERR_IO, "cannot write %s", path);
    const double total = n_units ? (double)n_units : 1.0;
    if (unclassified) fprintf(f, "%6.2f\t%llu\t%llu\tU\t0\tunclassified\n", 100.0 * (double)unclassified / total, (unsigned long long)unclassified, (unsigned long long)unclassified);
    // the rows are those of a database inspection (sh_k2_inspect.hip): one tree walk for both reports
    shi_k2_report_rows(f, db->nodes.data(), n, db->names, db->ranks, clade.data(), direct.data(), total, 0);
    const bool ok = fclose(f) == 0;
    SH_CHECK(ok, SH_ERR_IO, "short write to %s", path);
    return SH_OK;
}

// ---- minimizer data: host side ------------------------------------------------------------------------------------------
extern "C" sh_status sh_k2_mindata_free(sh_k2_mindata *md)
{
    if (!md) return SH_OK;
    hipSetDevice(md->device);
    hipFree(md->d_parent); hipFree(md->d_regs); hipFree(md->d_cnt); hipFree(md->d_clade_regs); hipFree(md->d_clade_cnt); hipFree(md->d_hist);
    delete md;
    return SH_OK;
}

static void k2_md_clear(void *p, uint64_t bytes, hipStream_t s)      // bytes: a multiple of 16 (hipMalloc aligns to more)
{
    const uint64_t n16 = bytes / 16;
    if (n16) hipLaunchKernelGGL(k_k2_md_clear, dim3((uint32_t)std::min<uint64_t>((n16 + 255) / 256, 4096)), dim3(256), 0, s, (uint4 *)p, n16);
}
// counters are 8 bytes each: round the node count up to an even one
static uint64_t k2_md_cnt_bytes(uint64_t n_nodes) { return (n_nodes + 1) / 2 * 16; }

extern "C" sh_status sh_k2_mindata_reset(sh_k2_mindata *md)
{
    SH_CHECK(md, SH_ERR_BAD_ARG, "sh_k2_mindata_reset: null argument");
    SH_HIP(hipSetDevice(md->device));
    k2_md_clear(md->d_regs, md->n_nodes * K2_MD_M, nullptr);
    k2_md_clear(md->d_cnt, k2_md_cnt_bytes(md->n_nodes), nullptr);
    md->clade_valid = false;
    SH_HIP(hipDeviceSynchronize());
    SH_HIP(hipGetLastError());
    return SH_OK;
}

extern "C" sh_status sh_k2_mindata_create(const sh_k2_db *db, sh_k2_mindata **out)
{
    SH_CHECK(db && out, SH_ERR_BAD_ARG, "sh_k2_mindata_create: null argument");
    *out = nullptr;
    SH_HIP(hipSetDevice(db->device));
    sh_k2_mindata *md = new sh_k2_mindata;
    md->device = db->device; md->n_nodes = db->nodes.size();
    const uint64_t reg_bytes = md->n_nodes * K2_MD_M, cnt_bytes = k2_md_cnt_bytes(md->n_nodes);
    if (hipMalloc(&md->d_regs, reg_bytes) != hipSuccess || hipMalloc(&md->d_cnt, cnt_bytes) != hipSuccess || hipMalloc(&md->d_parent, md->n_nodes * 4) != hipSuccess) {
        (void)hipGetLastError();
        sh_k2_mindata_free(md);
        sh_set_error("sh_k2_mindata_create: %llu bytes of registers and counters for %llu taxa do not fit the device", (unsigned long long)(reg_bytes + cnt_bytes),
                     (unsigned long long)db->nodes.size());
        return SH_ERR_OOM;
    }
    if (hipMemcpy(md->d_parent, db->d_parent, md->n_nodes * 4, hipMemcpyDeviceToDevice) != hipSuccess) { sh_k2_mindata_free(md); sh_set_error("copy of the taxonomy failed"); return SH_ERR_HIP; }
    sh_status st = sh_k2_mindata_reset(md);
    if (st != SH_OK) { sh_k2_mindata_free(md); return st; }
    *out = md;
    return SH_OK;
}

// clade registers, clade counts and both histograms, once per state of the accumulator
static sh_status k2_md_finish(sh_k2_mindata *md)
{
    SH_HIP(hipSetDevice(md->device));
    if (md->clade_valid) return SH_OK;
    const uint64_t reg_bytes = md->n_nodes * K2_MD_M, cnt_bytes = k2_md_cnt_bytes(md->n_nodes), hist_bytes = (2 * md->n_nodes * K2_MD_BINS * 4 + 15) / 16 * 16;
    if (!md->d_clade_regs) {
        if (hipMalloc(&md->d_clade_regs, reg_bytes) != hipSuccess || hipMalloc(&md->d_clade_cnt, cnt_bytes) != hipSuccess || hipMalloc(&md->d_hist, hist_bytes) != hipSuccess) {
            (void)hipGetLastError();
            hipFree(md->d_clade_regs); hipFree(md->d_clade_cnt); hipFree(md->d_hist);
            md->d_clade_regs = nullptr; md->d_clade_cnt = nullptr; md->d_hist = nullptr;
            sh_set_error("minimizer data: %llu bytes of clade registers for %llu taxa do not fit the device", (unsigned long long)(reg_bytes + cnt_bytes + hist_bytes),
                         (unsigned long long)md->n_nodes);
            return SH_ERR_OOM;
        }
    }
    k2_md_clear(md->d_clade_regs, reg_bytes, nullptr);
    k2_md_clear(md->d_clade_cnt, cnt_bytes, nullptr);
    k2_md_clear(md->d_hist, hist_bytes, nullptr);
    const uint32_t n = (uint32_t)md->n_nodes, grid = std::min<uint32_t>(std::max<uint32_t>(n, 1), 65536);
    hipLaunchKernelGGL(k_k2_md_clade, dim3(grid), dim3(256), 0, nullptr, md->d_parent, n, md->d_regs, md->d_cnt, md->d_clade_regs, md->d_clade_cnt);
    hipLaunchKernelGGL(k_k2_md_hist, dim3(grid), dim3(256), 0, nullptr, n, md->d_regs, md->d_cnt, md->d_hist);
    hipLaunchKernelGGL(k_k2_md_hist, dim3(grid), dim3(256), 0, nullptr, n, md->d_clade_regs, md->d_clade_cnt, md->d_hist + md->n_nodes * K2_MD_BINS);
    SH_HIP(hipDeviceSynchronize());
    SH_HIP(hipGetLastError());
    md->clade_valid = true;
    return SH_OK;
}

// Ertl's improved raw estimator (kraken2's default, hyperloglogplus.cc as recalled: PARITY UNPINNED) over the register
// histogram C[0 .. q + 1], q = 64 - p, in doubles
static double k2_hll_sigma(double x)
{
    if (x == 1.0) return INFINITY;
    double y = 1.0, z = x, zp;
    do { x *= x; zp = z; z += x * y; y += y; } while (zp != z);
    return z;
}
static double k2_hll_tau(double x)
{
    if (x == 0.0 || x == 1.0) return 0.0;
    double y = 1.0, z = 1.0 - x, zp;
    do { x = sqrt(x); zp = z; y *= 0.5; z -= (1.0 - x) * (1.0 - x) * y; } while (zp != z);
    return z / 3.0;
}
static double k2_hll_from_hist(const uint32_t *C)
{
    const double m = (double)K2_MD_M;
    const int q = 64 - K2_MD_P;
    double z = m * k2_hll_tau(1.0 - (double)C[q + 1] / m);
    for (int k = q; k >= 1; --k) z = 0.5 * (z + (double)C[k]);
    z += m * k2_hll_sigma((double)C[0] / m);
    return m * m / (2.0 * log(2.0) * z);       // (all registers empty: z = inf, the estimate 0)
}

extern "C" sh_status sh_k2_hll_estimate(const uint8_t *regs, double *out)
{
    SH_CHECK(regs && out, SH_ERR_BAD_ARG, "sh_k2_hll_estimate: null argument");
    uint32_t C[K2_MD_BINS] = {0};
    for (uint32_t i = 0; i < K2_MD_M; ++i) {
        SH_CHECK(regs[i] < K2_MD_BINS, SH_ERR_BAD_ARG, "sh_k2_hll_estimate: register %u holds %u (at most %d)", i, (unsigned)regs[i], K2_MD_BINS - 1);
        ++C[regs[i]];
    }
    *out = k2_hll_from_hist(C);
    return SH_OK;
}

extern "C" sh_status sh_k2_mindata_merge_host(uint8_t *dst_regs, const uint8_t *src_regs, uint64_t n)
{
    SH_CHECK((dst_regs && src_regs) || n == 0, SH_ERR_BAD_ARG, "sh_k2_mindata_merge_host: null argument");
    for (uint64_t i = 0; i < n; ++i) dst_regs[i] = std::max(dst_regs[i], src_regs[i]);
    return SH_OK;
}

extern "C" sh_status sh_k2_mindata_counts(sh_k2_mindata *md, uint64_t *n_minimizers, uint64_t *clade_minimizers, double *distinct, double *clade_distinct)
{
    SH_CHECK(md, SH_ERR_BAD_ARG, "sh_k2_mindata_counts: null argument");
    sh_status st = k2_md_finish(md);
    if (st != SH_OK) return st;
    const uint64_t n = md->n_nodes;
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "counter width");
    std::vector<uint64_t> own(n), clade(n);
    SH_HIP(hipMemcpy(own.data(), md->d_cnt, n * 8, hipMemcpyDeviceToHost));
    SH_HIP(hipMemcpy(clade.data(), md->d_clade_cnt, n * 8, hipMemcpyDeviceToHost));
    if (n_minimizers) memcpy(n_minimizers, own.data(), n * 8);
    if (clade_minimizers) memcpy(clade_minimizers, clade.data(), n * 8);
    if (distinct || clade_distinct) {
        std::vector<uint32_t> hist(2 * n * K2_MD_BINS);
        SH_HIP(hipMemcpy(hist.data(), md->d_hist, hist.size() * 4, hipMemcpyDeviceToHost));
        for (uint64_t t = 0; t < n; ++t) {       // a taxon without data has no histogram: nothing was seen
            if (distinct) distinct[t] = own[t] ? k2_hll_from_hist(hist.data() + t * K2_MD_BINS) : 0.0;
            if (clade_distinct) clade_distinct[t] = clade[t] ? k2_hll_from_hist(hist.data() + (n + t) * K2_MD_BINS) : 0.0;
        }
    }
    return SH_OK;
}

extern "C" sh_status sh_k2_mindata_registers(sh_k2_mindata *md, uint32_t taxon, uint8_t *out, int32_t clade)
{
    SH_CHECK(md && out, SH_ERR_BAD_ARG, "sh_k2_mindata_registers: null argument");
    SH_CHECK(taxon < md->n_nodes, SH_ERR_BAD_ARG, "sh_k2_mindata_registers: taxon %u outside the taxonomy of %llu nodes", taxon, (unsigned long long)md->n_nodes);
    SH_HIP(hipSetDevice(md->device));
    if (clade) { sh_status st = k2_md_finish(md); if (st != SH_OK) return st; }
    else SH_HIP(hipDeviceSynchronize());
    // register i is byte i & 3 of word i >> 2: on a little-endian host the words are the byte array
    SH_HIP(hipMemcpy(out, (clade ? md->d_clade_regs : md->d_regs) + (uint64_t)taxon * K2_MD_WORDS, K2_MD_M, hipMemcpyDeviceToHost));
    return SH_OK;
}

// the estimate as the report prints it
static uint64_t k2_hll_round(double e) { return !(e < 1.8e19) ? ~0ull : (uint64_t)floor(e + 0.5); }

// kraken2 --report-minimizer-data (reports.cc as recalled: PARITY UNPINNED): the rows of sh_k2_write_report with the clade's
// minimizer count and distinct-minimizer estimate after "direct reads"; the unclassified row carries 0 for both
extern "C" sh_status sh_k2_write_minimizer_report(const sh_k2_taxnode *nodes, uint64_t n_nodes, const char *names, uint64_t names_len, const char *ranks,
                                                  uint64_t ranks_len, const uint64_t *clade_reads, const uint64_t *direct_reads, const uint64_t *clade_minimizers,
                                                  const uint64_t *clade_distinct, uint64_t total_units, const char *path)
{
    SH_CHECK(nodes && clade_reads && direct_reads && clade_minimizers && clade_distinct && path && (names || names_len == 0) && (ranks || ranks_len == 0), SH_ERR_BAD_ARG,
             "sh_k2_write_minimizer_report: null argument");
    SH_CHECK(n_nodes >= 2, SH_ERR_BAD_ARG, "sh_k2_write_minimizer_report: a taxonomy has at least the empty node and the root");
    for (uint64_t i = 2; i < n_nodes; ++i)
        SH_CHECK(nodes[i].parent >= 1 && nodes[i].parent < i, SH_ERR_BAD_ARG, "sh_k2_write_minimizer_report: node %llu: ids must be breadth-first", (unsigned long long)i);
    SH_CHECK(clade_reads[1] <= total_units, SH_ERR_BAD_ARG, "sh_k2_write_minimizer_report: %llu classified units of %llu", (unsigned long long)clade_reads[1],
             (unsigned long long)total_units);
    const std::string name_pool(names ? names : "", names_len), rank_pool(ranks ? ranks : "", ranks_len);
    FILE *f = fopen(path, "w");
    SH_CHECK(f, SH_ERR_IO, "cannot write %s", path);
    const double total = total_units ? (double)total_units : 1.0;
    const uint64_t unclassified = total_units - clade_reads[1];
    if (unclassified) fprintf(f, "%6.2f\t%llu\t%llu\t0\t0\tU\t0\tunclassified\n", 100.0 * (double)unclassified / total, (unsigned long long)unclassified, (unsigned long long)unclassified);
    shi_k2_report_rows(f, nodes, n_nodes, name_pool, rank_pool, clade_reads, direct_reads, total, 0, clade_minimizers, clade_distinct);
    const bool ok = fclose(f) == 0;
    SH_CHECK(ok, SH_ERR_IO, "short write to %s", path);
    return SH_OK;
}

extern "C" sh_status sh_k2_mindata_write_report(const sh_k2_db *db, const sh_k2_result *res, uint64_t n_units, sh_k2_mindata *md, const char *path)
{
    SH_CHECK(db && md && path && (res || n_units == 0), SH_ERR_BAD_ARG, "sh_k2_mindata_write_report: null argument");
    const size_t n = db->nodes.size();
    SH_CHECK(md->n_nodes == n, SH_ERR_BAD_ARG, "the minimizer data belongs to another database");
    std::vector<uint64_t> direct(n, 0), clade, cm(n), cd(n);
    std::vector<double> est(n);
    for (uint64_t i = 0; i < n_units; ++i) if (res[i].call && res[i].call < n) ++direct[res[i].call];
    clade = direct;
    for (size_t i = n - 1; i >= 2; --i) clade[db->nodes[i].parent] += clade[i];      // parents have smaller ids
    sh_status st = sh_k2_mindata_counts(md, nullptr, cm.data(), nullptr, est.data());
    if (st != SH_OK) return st;
    for (size_t i = 0; i < n; ++i) cd[i] = k2_hll_round(est[i]);
    return sh_k2_write_minimizer_report(db->nodes.data(), n, db->names.data(), db->names.size(), db->ranks.data(), db->ranks.size(), clade.data(), direct.data(),
                                        cm.data(), cd.data(), n_units, path);
}
