// Host build of the giant reads' merge passes (scrubby_amd/csrc/sh_merge4.h) for tests/test_merge4_cpu.py: the group bounds, the four-way
// co-rank and the per-thread two-level merge, driven the way k_giant_split / k_giant_merge4 drive them - a block of tile / CNT threads per
// output tile, an array standing in for LDS, every thread reading its inputs before any thread stores - on tiles of 8 anchors.
// With -DMERGE4_MAIN the file is a program of its own that runs every case (the sanitizer build).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <numeric>
#include <vector>
#include "../scrubby_amd/csrc/sh_merge4.h"

namespace {

constexpr uint32_t CNT = 2;      // outputs per emulated thread

struct Buf { std::vector<uint64_t> x; std::vector<uint32_t> q; };

// One pass over a read of n anchors.  Returns 0, or the code of the property that failed.
int pass(const Buf &src, Buf &dst, uint32_t n, uint32_t tile, uint32_t width, uint32_t fanin)
{
    const uint32_t n_tiles = (n + tile - 1) / tile;
    std::vector<uint32_t> split(3 * (size_t)n_tiles);
    for (uint32_t t = 0; t < n_tiles; ++t) {      // k_giant_split
        const M4Group g = m4_group(t * tile, n, width, fanin);
        m4_corank4(src.x.data(), g, t * tile - g.e[0], split[3 * t], split[3 * t + 1], split[3 * t + 2]);
    }
    std::vector<uint64_t> sx(tile); std::vector<uint32_t> sq(tile);
    uint32_t prev[4] = {0, 0, 0, 0};
    for (uint32_t t = 0; t < n_tiles; ++t) {      // k_giant_merge4
        const uint32_t o0 = t * tile, o1 = o0 + tile < n ? o0 + tile : n;
        const M4Group g = m4_group(o0, n, width, fanin);
        if (g.e[0] > o0 || g.e[4] < o1 || g.e[0] % (fanin * width)) return 1;
        if (fanin == 2 && (g.e[3] != g.e[2] || g.e[4] != g.e[2])) return 2;
        uint32_t s0[4], s1[4], len[4];
        s0[0] = split[3 * t]; s0[1] = split[3 * t + 1]; s0[2] = split[3 * t + 2];
        if (s0[0] + s0[1] + s0[2] > o0 - g.e[0]) return 3;                 // the four offsets sum to the tile's output offset (d derived)
        s0[3] = o0 - g.e[0] - s0[0] - s0[1] - s0[2];
        const bool last = o1 == g.e[4];
        if (last) for (int k = 0; k < 4; ++k) s1[k] = g.e[k + 1] - g.e[k];      // the last tile of a group ends at the run ends
        else {
            s1[0] = split[3 * (t + 1)]; s1[1] = split[3 * (t + 1) + 1]; s1[2] = split[3 * (t + 1) + 2];
            if (s1[0] + s1[1] + s1[2] > o1 - g.e[0]) return 3;
            s1[3] = o1 - g.e[0] - s1[0] - s1[1] - s1[2];
        }
        for (int k = 0; k < 4; ++k) {
            if (s0[k] > g.e[k + 1] - g.e[k] || s1[k] > g.e[k + 1] - g.e[k]) return 4;      // inside its run
            if (s1[k] < s0[k]) return 5;                                                    // monotone from tile to tile
            if (o0 != g.e[0] && s0[k] < prev[k]) return 5;
            prev[k] = s1[k]; len[k] = s1[k] - s0[k];
        }
        if (o0 == g.e[0] && (s0[0] | s0[1] | s0[2] | s0[3])) return 6;                      // a group starts at its runs' starts
        const uint32_t m = len[0] + len[1] + len[2] + len[3];
        if (m != o1 - o0) return 7;
        const uint32_t p1 = len[0], p2 = p1 + len[1], p3 = p2 + len[2], p4 = m;
        for (uint32_t i = 0; i < m; ++i) {        // staging: position i of the tile's LDS comes from run k
            const uint32_t k = i < p1 ? 0 : i < p2 ? 1 : i < p3 ? 2 : 3, base = k == 0 ? 0 : k == 1 ? p1 : k == 2 ? p2 : p3;
            const uint32_t s = g.e[k] + s0[k] + (i - base);
            sx[i] = src.x[s]; sq[i] = src.q[s];
        }
        const uint32_t n_thr = tile / CNT;
        std::vector<uint64_t> ox((size_t)n_thr * CNT); std::vector<uint32_t> oq((size_t)n_thr * CNT);
        for (int level = 0; level < 2; ++level) {
            if (level == 1 && (p2 == 0 || p2 == p4)) break;      // one side empty: level 1 gave the output
            for (uint32_t tid = 0; tid < n_thr; ++tid) {
                uint64_t rx[CNT]; uint32_t rq[CNT];
                if (level == 0) m4_thread_merge<CNT>(sx.data(), sq.data(), p1, p2, p3, p4, tid * CNT, rx, rq);
                else m4_thread_merge<CNT>(sx.data(), sq.data(), p2, p4, p4, p4, tid * CNT, rx, rq);
                for (uint32_t u = 0; u < CNT; ++u) if (tid * CNT + u < m) { ox[tid * CNT + u] = rx[u]; oq[tid * CNT + u] = rq[u]; }
            }
            for (uint32_t i = 0; i < m; ++i) { sx[i] = ox[i]; sq[i] = oq[i]; }      // after the barrier
        }
        for (uint32_t i = 0; i < m; ++i) { dst.x[o0 + i] = sx[i]; dst.q[o0 + i] = sq[i]; }
    }
    return 0;
}

// the whole sort, at most max_pass passes; a read changes buffer with every pass it is active in
int sort_read(const uint64_t *x, uint32_t n, uint32_t tile, uint32_t fanin, uint32_t max_pass, Buf &out, uint32_t *n_pass)
{
    const uint32_t lf = fanin == 4 ? 2 : 1;
    Buf a, b;
    a.x.assign(x, x + n); a.q.resize(n); std::iota(a.q.begin(), a.q.end(), 0u);
    b.x.resize(n); b.q.resize(n);
    for (uint32_t c0 = 0; c0 < n; c0 += tile) {      // k_giant_chunksort
        const uint32_t c1 = c0 + tile < n ? c0 + tile : n;
        std::stable_sort(a.q.begin() + c0, a.q.begin() + c1, [&](uint32_t i, uint32_t j) { return x[i] < x[j]; });
        for (uint32_t i = c0; i < c1; ++i) a.x[i] = x[a.q[i]];
    }
    const uint32_t total = m4_passes(n, tile, lf);
    uint32_t p = 0;
    for (; p < total && p < max_pass; ++p) {
        const int rc = pass(p & 1 ? b : a, p & 1 ? a : b, n, tile, tile << (lf * p), fanin);
        if (rc) return 100 * (int)(p + 1) + rc;
    }
    out = p & 1 ? b : a;
    if (n_pass) *n_pass = total;
    return 0;
}

void make_keys(std::vector<uint64_t> &x, uint32_t tile, int mode, uint64_t seed)
{
    uint64_t s = seed * 0x9E3779B97F4A7C15ULL + 1;
    auto rnd = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
    const uint32_t n = (uint32_t)x.size(), n_runs = (n + tile - 1) / tile;
    for (uint32_t i = 0; i < n; ++i) {
        const uint64_t r = rnd();
        switch (mode) {
        case 0: x[i] = 42; break;                                                      // all equal: stability alone decides
        case 1: x[i] = 7 + r % 3; break;                                               // three values
        case 2: x[i] = ((uint64_t)(i / tile) << 32) + r % 1000; break;                  // increasing across runs: every tile draws from one run
        case 3: x[i] = ((uint64_t)(n_runs - i / tile) << 32) + r % 1000; break;         // decreasing across runs
        default: x[i] = r; break;                                                      // random 64-bit
        }
    }
}

}      // namespace

// the sort of one read: out_x / out_q (original index) after at most max_pass passes; *n_pass = the passes the read needs
extern "C" int m4h_sort(const uint64_t *x, uint32_t n, uint32_t tile, uint32_t fanin, uint32_t max_pass, uint64_t *out_x, uint32_t *out_q, uint32_t *n_pass)
{
    Buf out;
    const int rc = sort_read(x, n, tile, fanin, max_pass, out, n_pass);
    if (rc) return rc;
    std::copy(out.x.begin(), out.x.end(), out_x); std::copy(out.q.begin(), out.q.end(), out_q);
    return 0;
}

extern "C" void m4h_keys(uint64_t *x, uint32_t n, uint32_t tile, int mode, uint64_t seed)
{
    std::vector<uint64_t> v(n);
    make_keys(v, tile, mode, seed);
    std::copy(v.begin(), v.end(), x);
}

// every property of one case; 0 or the code of the first that failed
extern "C" int m4h_case(uint32_t n, uint32_t tile, int mode, uint64_t seed)
{
    std::vector<uint64_t> x(n);
    make_keys(x, tile, mode, seed);
    std::vector<uint32_t> ref(n);
    std::iota(ref.begin(), ref.end(), 0u);
    std::stable_sort(ref.begin(), ref.end(), [&](uint32_t i, uint32_t j) { return x[i] < x[j]; });
    uint32_t p4 = 0, p2 = 0;
    Buf o4, o2;
    int rc = sort_read(x.data(), n, tile, 4, ~0u, o4, &p4);
    if (rc) return rc;
    rc = sort_read(x.data(), n, tile, 2, ~0u, o2, &p2);
    if (rc) return 10000 + rc;
    if (p4 != (p2 + 1) / 2) return 20001;
    for (uint32_t i = 0; i < n; ++i) if (o4.q[i] != ref[i] || o4.x[i] != x[ref[i]]) return 20002;      // equals the stable sort
    for (uint32_t i = 0; i < n; ++i) if (o2.q[i] != ref[i] || o2.x[i] != x[ref[i]]) return 20003;
    for (uint32_t p = 1; p <= p4; ++p) {      // pass p of fan-in 4 = rounds 2p and 2p + 1 of fan-in 2, element for element
        rc = sort_read(x.data(), n, tile, 4, p, o4, nullptr);
        if (rc) return 30000 + rc;
        rc = sort_read(x.data(), n, tile, 2, 2 * p, o2, nullptr);
        if (rc) return 40000 + rc;
        if (o4.q != o2.q || o4.x != o2.x) return 50000 + (int)p;
    }
    return 0;
}

#ifdef MERGE4_MAIN
int main()
{
    const uint32_t tile = 8, Ts[] = {1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 20, 64, 65}, rs[] = {0, 1, tile - 1};
    int n_case = 0;
    for (int mode = 0; mode < 5; ++mode)
        for (uint32_t T : Ts)
            for (uint32_t r : rs) {
                const int rc = m4h_case(T * tile + r, tile, mode, 1000u * mode + T);
                if (rc) { std::printf("mode %d n %u: code %d\n", mode, T * tile + r, rc); return 1; }
                ++n_case;
            }
    std::printf("%d cases ok\n", n_case);
    return 0;
}
#endif
