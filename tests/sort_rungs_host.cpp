// Host build of the ladder of k_sort_top launches (scrubby_amd/csrc/sh_sort_rungs.h) for tests/test_sort_rungs_cpu.py: the table as data, and
// the checks on it - every anchor count of the LDS tables belongs to one launch whose block holds it, a rung's LDS fits its residency, the
// rungs of a table tile it.  The table bounds are written out here a second time (k_expand's: 256, 512, 1024, 2048, 4096), not taken from
// the header.  With -DSORT_RUNGS_MAIN the file is a program of its own that runs the checks (the sanitizer build).
#include <cstdint>
#include <cstdio>
#include "../scrubby_amd/csrc/sh_sort_rungs.h"

namespace {

const int TABLE_HI[5] = {256, 512, 1024, 2048, 4096};      // table t lists 65 / TABLE_HI[t - 1] + 1 .. TABLE_HI[t] anchors
int table_lo(int t) { return t == 0 ? 64 : TABLE_HI[t - 1]; }
int table_of(int n) { for (int t = 0; t < 5; ++t) if (n <= TABLE_HI[t]) return t; return -1; }

// what k_sort_top<NMIN, NMAX, CLS, NTHR> does with an item of n anchors in table cls
bool takes(const SortRung &r, int cls, int n) { return r.cls == cls && r.nmin < n && n <= r.nmax; }

}

extern "C" {

int srh_count() { return SORT_N_RUNGS; }
void srh_get(int i, int32_t *out) { const SortRung &r = SORT_RUNGS[i]; out[0] = r.cls; out[1] = r.nmin; out[2] = r.nmax; out[3] = r.nthr; out[4] = r.blocks; }
int srh_lds(int nmax) { return sort_rung_lds(nmax); }
int srh_budget(int blocks) { return sort_rung_lds_budget(blocks); }
int srh_rung_of(int n) { return sort_rung_of(n); }
int srh_last_of_table(int i) { return sort_rung_last_of_table(i) ? 1 : 0; }
int srh_alone(int i) { return sort_rung_alone(i) ? 1 : 0; }

// launches that take a read of n anchors (k_expand lists it in table_of(n))
int srh_launches_for(int n)
{
    int c = 0;
    for (int i = 0; i < SORT_N_RUNGS; ++i) c += takes(SORT_RUNGS[i], table_of(n), n) ? 1 : 0;
    return c;
}

// 0, or 100 * (rung or n) + the code of the property that failed
int srh_check()
{
    for (int n = 65; n <= 4096; ++n) {
        if (srh_launches_for(n) != 1) return 100 * n + 1;                       // exactly one launch
        const int i = sort_rung_of(n);
        if (i < 0 || !takes(SORT_RUNGS[i], table_of(n), n)) return 100 * n + 2; // ... the one sort_rung_of names, in the read's own table
        if (SORT_RUNGS[i].nmax < n) return 100 * n + 3;                         // ... whose block holds the read
    }
    if (sort_rung_of(64) != -1 || sort_rung_of(4097) != -1 || sort_rung_of(0) != -1) return 4;
    for (int i = 0; i < SORT_N_RUNGS; ++i) {
        const SortRung &r = SORT_RUNGS[i];
        if (r.blocks < 1 || r.nthr < 64 || r.nthr > 1024 || r.nthr % 64) return 100 * i + 5;
        if ((long long)sort_rung_lds(r.nmax) * r.blocks > SORT_CU_LDS_BYTES) return 100 * i + 6;      // 24 NMAX + fixed <= 160 KiB / blocks
        if (sort_rung_lds(r.nmax) > sort_rung_lds_budget(r.blocks)) return 100 * i + 7;               // ... also in whole granules
        if (r.blocks * (r.nthr / 64) > 32) return 100 * i + 8;                                        // 8 waves on each of a CU's 4 SIMDs
        if (r.nmax % 64) return 100 * i + 9;
        // tiling: a table's first rung starts at the table's lower bound, each next one where the last ended, the last ends at the upper bound
        const bool first = i == 0 || SORT_RUNGS[i - 1].cls != r.cls;
        if (r.cls < 0 || r.cls > 4 || r.nmin >= r.nmax) return 100 * i + 10;
        if (first ? (r.nmin != table_lo(r.cls) || (i > 0 && SORT_RUNGS[i - 1].cls != r.cls - 1)) : r.nmin != SORT_RUNGS[i - 1].nmax) return 100 * i + 11;
        if (sort_rung_last_of_table(i) && r.nmax != TABLE_HI[r.cls]) return 100 * i + 12;
        if (sort_rung_alone(i) != (first && sort_rung_last_of_table(i))) return 100 * i + 15;
        if (sort_rung_alone(i) && (r.nmin != table_lo(r.cls) || r.nmax != TABLE_HI[r.cls])) return 100 * i + 16;      // a kernel that does not look at n takes the whole table
        if (!first && (r.nthr != SORT_RUNGS[i - 1].nthr || r.blocks >= SORT_RUNGS[i - 1].blocks)) return 100 * i + 13;      // a larger rung holds fewer blocks
    }
    if (SORT_RUNGS[0].cls != 0 || SORT_RUNGS[SORT_N_RUNGS - 1].cls != 4) return 14;
    return 0;
}

}

#ifdef SORT_RUNGS_MAIN
int main()
{
    const int rc = srh_check();
    if (rc) { std::printf("sort rungs: property %d failed at %d\n", rc % 100, rc / 100); return 1; }
    int32_t v[5];
    for (int i = 0; i < srh_count(); ++i) { srh_get(i, v); std::printf("rung %d: table %d, %d < n <= %d, %d threads, %d blocks per CU, %d B of LDS\n", i, v[0], v[1], v[2], v[3], v[4], srh_lds(v[2])); }
    std::printf("%d rungs ok\n", srh_count());
    return 0;
}
#endif
