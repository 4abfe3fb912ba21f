// Index arithmetic of the giant reads' merge passes (sh_classify.hip: k_giant_split / k_giant_merge4), free of HIP so that a host compiler can
// include it (tests/merge4_host.cpp).  A pass with fan-in F (2 or 4) merges groups of up to F consecutive sorted runs of width W into one run of
// F * W as the tree (A + B) + (C + D) of stable two-way merges, the left side winning ties at every node (`<=`): the order is (key, run,
// position in run), element for element what two successive two-way rounds give.  Fan-in 2 is the same code with C and D empty.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define M4_FN __host__ __device__ inline
#else
#define M4_FN inline
#endif

// passes a read of n anchors takes: run widths tile, tile << lf, tile << 2 lf, ... while they are below n (lf = log2 of the fan-in)
M4_FN uint32_t m4_passes(uint32_t n, uint32_t tile, uint32_t lf)
{
    uint32_t r = 0;
    for (uint64_t w = tile; w < n; w <<= lf) ++r;
    return r;
}

// The group of runs that holds output o0 of a read of n anchors: run k is [e[k], e[k+1]) (k < 4), the group's outputs are [e[0], e[4]).
// The last group of a read may have fewer runs and a short last run: the missing ones are empty.
struct M4Group { uint32_t e[5]; };

M4_FN M4Group m4_group(uint32_t o0, uint32_t n, uint32_t width, uint32_t fanin)
{
    M4Group g;
    const uint64_t gb = (uint64_t)o0 / ((uint64_t)fanin * width) * ((uint64_t)fanin * width);
    for (uint32_t k = 0; k <= 4; ++k) {
        const uint64_t b = gb + (uint64_t)(k < fanin ? k : fanin) * width;
        g.e[k] = b < n ? (uint32_t)b : n;
    }
    return g;
}

// Elements the left run L (nl of them) gives to the first k outputs of L + R, the answer known to lie in [lo, hi]
template <class KX>
M4_FN uint32_t m4_corank2(const KX *L, uint32_t nl, const KX *R, uint32_t nr, uint32_t k, uint32_t lo, uint32_t hi)
{
    const uint32_t lo_min = k > nr ? k - nr : 0, hi_max = k < nl ? k : nl;
    lo = lo > lo_min ? lo : lo_min; hi = hi < hi_max ? hi : hi_max;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (L[mid] <= R[k - 1 - mid]) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// Co-rank of the group's output d (0 <= d <= e[4] - e[0]): a + b + c + (d - a - b - c) elements of runs A, B, C, D come before it.
// A nested merge path: the outer search runs over i, the elements (A + B) gives; element k of the virtual A + B is found by the two-run
// co-rank, whose range shrinks with the outer one (the co-rank moves by at most one per element), so that the later probes are short and
// close to each other.  When the outer search ends, the inner co-ranks of both sides are known: no search follows it.
template <class KX>
M4_FN void m4_corank4(const KX *x, const M4Group &g, uint32_t d, uint32_t &a, uint32_t &b, uint32_t &c)
{
    const KX *A = x + g.e[0], *B = x + g.e[1], *C = x + g.e[2], *D = x + g.e[3];
    const uint32_t na = g.e[1] - g.e[0], nb = g.e[2] - g.e[1], nc = g.e[3] - g.e[2], nd = g.e[4] - g.e[3];
    const uint32_t nab = na + nb, ncd = nc + nd;
    uint32_t lo = d > ncd ? d - ncd : 0, hi = d < nab ? d : nab;      // i in [lo, hi]; j = d - i elements of C + D
    // co-ranks of A in A + B at lo and hi, of C in C + D at d - hi and d - lo
    uint32_t a_lo = m4_corank2(A, na, B, nb, lo, 0u, na), a_hi = lo < hi ? m4_corank2(A, na, B, nb, hi, 0u, na) : a_lo;
    uint32_t c_lo = m4_corank2(C, nc, D, nd, d - hi, 0u, nc), c_hi = lo < hi ? m4_corank2(C, nc, D, nd, d - lo, 0u, nc) : c_lo;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1, jm = d - 1 - mid;        // compare (A + B)[mid] with (C + D)[jm]
        uint32_t l = a_hi > hi - mid && a_hi - (hi - mid) > a_lo ? a_hi - (hi - mid) : a_lo;
        uint32_t h = a_lo + (mid - lo) < a_hi ? a_lo + (mid - lo) : a_hi;
        const uint32_t am = m4_corank2(A, na, B, nb, mid, l, h), bm = mid - am;
        const bool from_a = am < na && (bm >= nb || A[am] <= B[bm]);
        const KX vab = from_a ? A[am] : B[bm];
        const uint32_t j_lo = d - hi, j_hi = d - lo;
        l = c_hi > j_hi - jm && c_hi - (j_hi - jm) > c_lo ? c_hi - (j_hi - jm) : c_lo;
        h = c_lo + (jm - j_lo) < c_hi ? c_lo + (jm - j_lo) : c_hi;
        const uint32_t cm = m4_corank2(C, nc, D, nd, jm, l, h), dm = jm - cm;
        const bool from_c = cm < nc && (dm >= nd || C[cm] <= D[dm]);
        const KX vcd = from_c ? C[cm] : D[dm];
        if (vab <= vcd) { lo = mid + 1; a_lo = am + (from_a ? 1u : 0u); c_hi = cm; }      // j_hi becomes jm
        else { hi = mid; a_hi = am; c_lo = cm + (from_c ? 1u : 0u); }                     // j_lo becomes jm + 1
    }
    a = a_lo; b = lo - a_lo; c = c_lo;
}

// One thread's CNT outputs [e0, e0 + CNT) of one merge level over sx / sq (LDS on the device).  The level's input is two pairs of sorted
// ranges side by side, [0, p1) + [p1, p2) and [p2, p3) + [p3, p4); its output is the two merged sequences side by side in the same places,
// [0, p2) and [p2, p4).  Outputs at p4 and beyond do not exist; their ox / oq are left alone.  The thread reads sx / sq only: the caller
// stores the outputs once every thread has read its inputs.
template <uint32_t CNT, class KX, class KQ>
M4_FN void m4_thread_merge(const KX *sx, const KQ *sq, uint32_t p1, uint32_t p2, uint32_t p3, uint32_t p4, uint32_t e0, KX (&ox)[CNT], KQ (&oq)[CNT])
{
    if (e0 >= p4) return;
    const bool second = e0 >= p2;
    const uint32_t l0 = second ? p2 : 0u, l1 = second ? p3 : p1, r1 = second ? p4 : p2, k = e0 - l0;
    const uint32_t split = m4_corank2(sx + l0, l1 - l0, sx + l1, r1 - l1, k, 0u, l1 - l0);
    uint32_t ia = l0 + split, ea = l1, ib = l1 + (k - split), eb = r1;
    KX va = ia < ea ? sx[ia] : (KX)~(KX)0, vb = ib < eb ? sx[ib] : (KX)~(KX)0;
#if defined(__clang__)
#pragma unroll
#endif
    for (uint32_t u = 0; u < CNT; ++u) {
        const uint32_t pos = e0 + u;
        if (pos < p4) {
            if (pos == p2) {      // from the first pair's outputs into the second's
                ia = p2; ea = p3; ib = p3; eb = p4;
                va = ia < ea ? sx[ia] : (KX)~(KX)0; vb = ib < eb ? sx[ib] : (KX)~(KX)0;
            }
            const bool take_l = ia < ea && (ib >= eb || va <= vb);
            if (take_l) { ox[u] = va; oq[u] = sq[ia]; ++ia; va = ia < ea ? sx[ia] : (KX)~(KX)0; }
            else { ox[u] = vb; oq[u] = sq[ib]; ++ib; vb = ib < eb ? sx[ib] : (KX)~(KX)0; }
        }
    }
}
