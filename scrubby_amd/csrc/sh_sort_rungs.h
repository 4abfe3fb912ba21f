// The launches of k_sort_top over the LDS sort tables (sh_classify.hip: big_pass), free of HIP so that a host compiler can include it
// (tests/sort_rungs_host.cpp).  A block of k_sort_top holds two ping-pong buffers of (x, q) - 24 B per anchor of its NMAX - plus a fixed part,
// and how many blocks a CU's LDS holds is what decides the residency of the two large tables: so a table may be served by several launches
// ("rungs"), each taking the reads with nmin < n <= nmax of table cls in a block sized to nmax.  The rungs of a table run one after the
// other, smallest first, and tile the table's range without gap or overlap; tables 0-2 are one rung each (what was measured: DESIGN.md 3.3).
#pragma once
#include <stdint.h>

#define SORT_TOP_LDS_PER_ANCHOR 24      // uint64_t s_x[2][NMAX] + uint32_t s_q[2][NMAX]
#define SORT_TOP_LDS_FIXED 2160         // ParFillLds, the backtrack's candidate lists, ticket and reduction words
#define SORT_CU_LDS_BYTES (160 * 1024)  // gfx950
#define SORT_LDS_GRANULE 1280           // ... which hands LDS out in units of 320 dwords

struct SortRung { int cls, nmin, nmax, nthr, blocks; };      // blocks: the residency per CU the rung's LDS is cut for

constexpr SortRung SORT_RUNGS[] = {
    {0, 64, 256, 64, 16},           // tables 0-2: bound by registers or balanced, one launch each (grids as they were: big_pass)
    {1, 256, 512, 128, 8},
    {2, 512, 1024, 256, 6},
    {3, 1024, 1600, 256, 4},        // table 3 (1025 .. 2048): 69 % of its anchors are in the lower rung
    {3, 1600, 2048, 256, 3},
    {4, 2048, 3264, 512, 2},        // table 4 (2049 .. 4096): 85 %
    {4, 3264, 4096, 512, 1},
};
constexpr int SORT_N_RUNGS = (int)(sizeof(SORT_RUNGS) / sizeof(SORT_RUNGS[0]));

constexpr int sort_rung_lds(int nmax) { return SORT_TOP_LDS_PER_ANCHOR * nmax + SORT_TOP_LDS_FIXED; }
// the largest block a CU holds `blocks` of, in whole granules
constexpr int sort_rung_lds_budget(int blocks) { return SORT_CU_LDS_BYTES / SORT_LDS_GRANULE / blocks * SORT_LDS_GRANULE; }
// the index of the launch that takes a read of n anchors, -1: none (n <= 64 is chained inside k_expand, n > 4096 is a giant)
constexpr int sort_rung_of(int n)
{
    for (int i = 0; i < SORT_N_RUNGS; ++i) if (SORT_RUNGS[i].nmin < n && n <= SORT_RUNGS[i].nmax) return i;
    return -1;
}
constexpr bool sort_rung_last_of_table(int i) { return i + 1 == SORT_N_RUNGS || SORT_RUNGS[i + 1].cls != SORT_RUNGS[i].cls; }
// the table's only rung: every read k_expand lists there is its own, the kernel need not look at n
constexpr bool sort_rung_alone(int i) { return (i == 0 || SORT_RUNGS[i - 1].cls != SORT_RUNGS[i].cls) && sort_rung_last_of_table(i); }
