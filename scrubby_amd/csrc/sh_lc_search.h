// The list search of k_local_cluster (sh_classify.hip), free of HIP so that a host compiler can include it
// (tests/lc_search_host.cpp).  One lane holds one seed of the read; the seed's occurrences are an ascending list of 64-bit words
// (contig << 32 | position << 1 | strand).  The kernel asks which of them lie in the window [wlo, whi] of one contig, and asks again for a
// wider window up to three times: the window only ever grows, so the list is searched ONCE (lc_open) and the answer is then extended at
// its two ends (lc_grow), never searched again from the list's head.
//   lc_open     the 8-ary lower bound of the window's lower key (seven independent loads a step, then eight entries), then the entries
//               from there eight at a time until one lies past the window
//   lc_grow     the wider window: downward from `first`, upward from `stop`, eight entries a step.  The positions of the two entries just
//               outside the old window were seen by the loads that stopped there and are kept (`below`, `above`): where they show that
//               the added stretch holds nothing on a side - the usual case, and every case in a read's last, confirming round - that
//               side costs no load at all
//   lc_collect  the in-window entries of the right strand relation, in list order, loaded eight at a time
// Keys are compared on all 64 bits when they are loaded (a neighbour on another contig is no neighbour: LC_NONE), so that `below` and
// `above` are one register each.  L is anything with operator[](uint32_t) -> uint64_t: a pointer in the kernel, a counting accessor in the
// host test.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define LC_FN __host__ __device__ inline
#else
#define LC_FN inline
#endif

#define LC_CAP 16u                // in-window occurrences of one seed that are taken; more: the read is declined
#define LC_NONE 0xffffffffu       // below / above: no entry on the window's contig there (list start / end, or another contig)
enum { LC_STOP_WHI = 0, LC_STOP_CONTIG, LC_STOP_END, LC_STOP_CAP };      // why the upward scan stopped

// what does not change over the rounds of a read
struct LcQuery {
    uint32_t contig;      // of the window (31 bits)
    uint32_t qbit;        // strand bit of the seed in the read
    uint32_t rel;         // strand relation of K's anchors (0 / 1)
    uint32_t occ;         // length of the list
};

struct LcSearch {
    uint32_t first, stop;      // [first, stop): the list's entries inside the window, either strand
    uint32_t c;                // of them the right strand's, cumulative over open and grow; > LC_CAP: the search gave up there
    uint32_t below, above;     // position of lst[first - 1] / lst[stop] where it is on the window's contig, else LC_NONE
    uint32_t nlo, nhi;         // lowest / highest position the LAST step (open or one grow) counted; 0xffffffff / 0: none
    uint32_t why;              // LC_STOP_*: how the last upward scan ended
};

// the window around the anchors found so far
LC_FN void lc_window(uint32_t lo, uint32_t hi, uint32_t mdx, uint32_t &wlo, uint32_t &whi)
{
    wlo = lo > mdx ? lo - mdx : 0u;
    whi = hi + mdx < hi ? 0xffffffffu : hi + mdx;
}
LC_FN uint64_t lc_key_lo(uint32_t contig, uint32_t wlo) { return (uint64_t)contig << 32 | (uint64_t)wlo << 1; }
LC_FN bool lc_right_strand(uint64_t pw, const LcQuery &Q) { return (((uint32_t)pw & 1u) != Q.qbit) == (Q.rel != 0); }
LC_FN uint32_t lc_neighbour(uint64_t pw, const LcQuery &Q) { return (uint32_t)(pw >> 32) == Q.contig ? (uint32_t)pw >> 1 : LC_NONE; }
LC_FN void lc_count(LcSearch &s, uint64_t pw, const LcQuery &Q)
{
    if (!lc_right_strand(pw, Q)) return;
    const uint32_t xp = (uint32_t)pw >> 1;
    ++s.c;
    s.nlo = xp < s.nlo ? xp : s.nlo; s.nhi = xp > s.nhi ? xp : s.nhi;
}

// from s.stop upward, eight entries a step, until one is past whi, on another contig or past the list's end - or the cap is passed
template <class L>
LC_FN void lc_scan_up(LcSearch &s, L lst, const LcQuery &Q, uint32_t whi)
{
    bool more = true;
    for (uint32_t t0 = s.stop; more && t0 < Q.occ && s.c <= LC_CAP; t0 += 8u) {
        uint64_t pv[8];
#pragma unroll
        for (uint32_t j = 0; j < 8u; ++j) pv[j] = t0 + j < Q.occ ? lst[t0 + j] : ~0ull;
#pragma unroll
        for (uint32_t j = 0; j < 8u; ++j) {
            const uint64_t pw = pv[j];
            if (!more) continue;
            if ((uint32_t)(pw >> 32) != Q.contig) { more = false; s.above = LC_NONE; s.why = t0 + j < Q.occ ? LC_STOP_CONTIG : LC_STOP_END; continue; }
            if (((uint32_t)pw >> 1) > whi) { more = false; s.above = (uint32_t)pw >> 1; s.why = LC_STOP_WHI; continue; }
            ++s.stop;
            lc_count(s, pw, Q);
        }
    }
    if (more) { s.above = LC_NONE; s.why = s.stop < Q.occ ? LC_STOP_CAP : LC_STOP_END; }
}

template <class L>
LC_FN void lc_open(LcSearch &s, L lst, const LcQuery &Q, uint32_t wlo, uint32_t whi)
{
    const uint64_t key_lo = lc_key_lo(Q.contig, wlo);
    uint32_t b = 0, len = Q.occ;
    uint64_t under = ~0ull;      // the last entry seen below key_lo: lst[b - 1] whenever b > 0 (every step's b - 1 is a pivot it loaded)
    while (len > 8u) {
        const uint32_t step = (len + 7u) >> 3;
        uint64_t pv[7];
#pragma unroll
        for (uint32_t j = 0; j < 7u; ++j) { const uint32_t ix = b + (j + 1u) * step - 1u; pv[j] = ix < b + len ? lst[ix] : ~0ull; }
        uint32_t cnt = 0;
#pragma unroll
        for (uint32_t j = 0; j < 7u; ++j) { const bool lt = pv[j] < key_lo; cnt += lt; under = lt ? pv[j] : under; }
        const uint32_t nb = b + cnt * step;
        len = step < b + len - nb ? step : b + len - nb; b = nb;
    }
    {
        uint64_t pv[8];
#pragma unroll
        for (uint32_t j = 0; j < 8u; ++j) pv[j] = j < len ? lst[b + j] : ~0ull;
        uint32_t cnt = 0;
#pragma unroll
        for (uint32_t j = 0; j < 8u; ++j) { const bool lt = pv[j] < key_lo; cnt += lt; under = lt ? pv[j] : under; }
        b += cnt;
    }
    s.first = s.stop = b; s.c = 0;
    s.below = lc_neighbour(under, Q);      // ~0: no entry below (b == 0), contig 0xffffffff is no window's
    s.nlo = 0xffffffffu; s.nhi = 0u;
    lc_scan_up(s, lst, Q, whi);
}

// the window has grown to [wlo, whi] (it contains the one before)
template <class L>
LC_FN void lc_grow(LcSearch &s, L lst, const LcQuery &Q, uint32_t wlo, uint32_t whi)
{
    s.nlo = 0xffffffffu; s.nhi = 0u;
    if (s.below != LC_NONE && s.below >= wlo) {      // lst[first - 1] is inside now
        const uint64_t key_lo = lc_key_lo(Q.contig, wlo);
        bool more = true;
        while (more && s.first > 0u && s.c <= LC_CAP) {
            const uint32_t t1 = s.first;
            uint64_t pv[8];
#pragma unroll
            for (uint32_t j = 0; j < 8u; ++j) pv[j] = j < t1 ? lst[t1 - 1u - j] : 0ull;
#pragma unroll
            for (uint32_t j = 0; j < 8u; ++j) {
                const uint64_t pw = pv[j];
                if (!more) continue;
                if (j >= t1) { more = false; s.below = LC_NONE; continue; }
                if (pw < key_lo) { more = false; s.below = lc_neighbour(pw, Q); continue; }
                --s.first;
                lc_count(s, pw, Q);
            }
        }
        if (more) s.below = LC_NONE;      // the list's head (or the cap: the read is declined)
    }
    if (s.above != LC_NONE && s.above <= whi) lc_scan_up(s, lst, Q, whi);
}

// emit(pw) for every entry of [first, stop) of the right strand relation, in list order
template <class L, class F>
LC_FN void lc_collect(const LcSearch &s, L lst, const LcQuery &Q, F emit)
{
    for (uint32_t t0 = s.first; t0 < s.stop; t0 += 8u) {
        uint64_t pv[8];
#pragma unroll
        for (uint32_t j = 0; j < 8u; ++j) pv[j] = t0 + j < s.stop ? lst[t0 + j] : 0ull;
#pragma unroll
        for (uint32_t j = 0; j < 8u; ++j) if (t0 + j < s.stop && lc_right_strand(pv[j], Q)) emit(pv[j]);
    }
}
