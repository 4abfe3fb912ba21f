// Host build of k_local_cluster's list search (scrubby_amd/csrc/sh_lc_search.h) for tests/test_lc_search_cpu.py: lc_open / lc_grow /
// lc_collect against a brute force over the whole list, for every window of a sequence of nested windows.  The list is read through an
// accessor that counts the loads and refuses an index outside the list.  With -DLC_SEARCH_MAIN the file is a program of its own that runs
// every check (the sanitizer build).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <algorithm>
#include "../scrubby_amd/csrc/sh_lc_search.h"

namespace {

struct Counting {
    const uint64_t *p; uint32_t n; long *loads; int *oob;
    uint64_t operator[](uint32_t i) const { ++*loads; if (i >= n) { *oob = 1; return 0; } return p[i]; }
};

uint64_t word(uint32_t contig, uint32_t pos, uint32_t strand) { return (uint64_t)contig << 32 | (uint64_t)pos << 1 | strand; }

// the whole list, front to back: what the window [wlo, whi] of Q.contig holds
struct Brute { uint32_t first, stop, c, nlo, nhi, below, above, why; std::vector<uint64_t> got; };
Brute brute(const std::vector<uint64_t> &l, const LcQuery &Q, uint32_t wlo, uint32_t whi)
{
    Brute b{0, 0, 0, 0xffffffffu, 0u, LC_NONE, LC_NONE, LC_STOP_END, {}};
    const uint64_t key_lo = (uint64_t)Q.contig << 32 | (uint64_t)wlo << 1;
    while (b.first < l.size() && l[b.first] < key_lo) ++b.first;
    b.stop = b.first;
    while (b.stop < l.size() && (uint32_t)(l[b.stop] >> 32) == Q.contig && ((uint32_t)l[b.stop] >> 1) <= whi) ++b.stop;
    for (uint32_t i = b.first; i < b.stop; ++i)
        if ((((uint32_t)l[i] & 1u) != Q.qbit) == (Q.rel != 0)) { ++b.c; b.nlo = std::min(b.nlo, (uint32_t)l[i] >> 1); b.nhi = std::max(b.nhi, (uint32_t)l[i] >> 1); b.got.push_back(l[i]); }
    if (b.first > 0 && (uint32_t)(l[b.first - 1] >> 32) == Q.contig) b.below = (uint32_t)l[b.first - 1] >> 1;
    if (b.stop < l.size()) {
        const bool same = (uint32_t)(l[b.stop] >> 32) == Q.contig;
        b.why = same ? LC_STOP_WHI : LC_STOP_CONTIG;
        if (same) b.above = (uint32_t)l[b.stop] >> 1;
    }
    return b;
}

struct Step { long loads; uint32_t first, stop, c; };

// open on win[0], grow through win[1 ..]: 0, or 100 * step + the code of what differs from the brute force.  steps: what each step did
int run_sequence(const std::vector<uint64_t> &l, LcQuery Q, const std::vector<std::pair<uint32_t, uint32_t>> &win, std::vector<Step> *steps = nullptr)
{
    long loads = 0; int oob = 0;
    Q.occ = (uint32_t)l.size();
    const Counting lst{l.data(), Q.occ, &loads, &oob};
    LcSearch s{};
    uint32_t nlo = 0xffffffffu, nhi = 0u;
    for (size_t i = 0; i < win.size(); ++i) {
        const long before = loads;
        if (i && (win[i].first > win[i - 1].first || win[i].second < win[i - 1].second)) return 100 * (int)i + 20;      // not nested: the test's own fault
        if (i == 0) lc_open(s, lst, Q, win[i].first, win[i].second); else lc_grow(s, lst, Q, win[i].first, win[i].second);
        const Brute b = brute(l, Q, win[i].first, win[i].second);
        if (steps) steps->push_back(Step{loads - before, s.first, s.stop, s.c});
        if (oob) return 100 * (int)i + 1;
        if (b.c > LC_CAP) { if (s.c <= LC_CAP) return 100 * (int)i + 2; return 0; }      // past the cap the kernel declines the read: nothing else is asked
        if (s.c != b.c) return 100 * (int)i + 3;
        if (s.first != b.first) return 100 * (int)i + 4;
        if (s.stop != b.stop) return 100 * (int)i + 5;
        if (s.why != b.why) return 100 * (int)i + 6;      // (a grow without an upward scan keeps the reason it had: the stop did not move)
        if (s.below != b.below) return 100 * (int)i + 7;
        if (s.above != b.above) return 100 * (int)i + 8;
        nlo = std::min(nlo, s.nlo); nhi = std::max(nhi, s.nhi);
        if (nlo != b.nlo || nhi != b.nhi) return 100 * (int)i + 9;
        std::vector<uint64_t> got;
        const long lb = loads;
        lc_collect(s, lst, Q, [&](uint64_t pw) { got.push_back(pw); });
        if (oob) return 100 * (int)i + 10;
        if (got != b.got) return 100 * (int)i + 11;
        if (loads - lb > (long)((b.stop - b.first + 7u) / 8u * 8u)) return 100 * (int)i + 12;      // batches of eight over [first, stop), nothing else
    }
    return 0;
}

struct Rng {
    uint64_t s;
    uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
    uint32_t below(uint32_t n) { return n ? next() % n : 0u; }
};

// n entries over the contigs 3, 4, 5, mixed strands, distinct words, ascending; positions below `span` so that windows of a few hundred hold several
std::vector<uint64_t> make_list(Rng &r, uint32_t n, uint32_t span)
{
    std::vector<uint64_t> l;
    while (l.size() < n) {
        const uint64_t w = word(3 + r.below(3), r.below(span), r.below(2));
        if (std::find(l.begin(), l.end(), w) == l.end()) l.push_back(w);
    }
    std::sort(l.begin(), l.end());
    return l;
}

}

extern "C" {

// `count` seeded sequences of one to four nested windows over a list of n entries: 0, or 10000 * sequence + run_sequence's code
int lsh_random(uint32_t n, uint32_t seed, int count)
{
    Rng r{0x9E3779B97F4A7C15ull ^ ((uint64_t)seed << 20) ^ n};
    for (int it = 0; it < count; ++it) {
        const uint32_t span = it % 3 == 0 ? 40u + 2u * n : (it % 3 == 1 ? 400u + 10u * n : 3000u);
        const std::vector<uint64_t> l = make_list(r, n, span);
        LcQuery Q{2 + r.below(5), r.below(2), r.below(2), 0};      // contigs 2 and 6 are not in the list
        std::vector<std::pair<uint32_t, uint32_t>> win;
        const uint32_t mid = r.below(span + 20), grow[6] = {0, 0, 1, 1 + r.below(8), 1 + r.below(span / 4 + 1), span};
        uint32_t lo = mid > r.below(span / 8 + 2) ? mid - r.below(span / 8 + 2) : 0u, hi = mid + r.below(span / 8 + 2);
        if (it % 11 == 0) { const uint64_t at = l[r.below(n)]; lo = hi = (uint32_t)at >> 1; Q.contig = (uint32_t)(at >> 32); }      // a window of one position that is taken
        const int n_win = 1 + (int)r.below(4);
        for (int i = 0; i < n_win; ++i) {
            if (i) { const uint32_t d = grow[r.below(6)]; lo = lo > d ? lo - d : 0u; hi += grow[r.below(6)]; }
            win.push_back({lo, hi});
        }
        const int rc = run_sequence(l, Q, win);
        if (rc) return 10000 * (it + 1) + rc;
    }
    return 0;
}

// one sequence from the caller: words[n] ascending, win[2 * n_win]; out[8 * n_win]: first, stop, c, below, above, nlo, nhi (of the step), loads;
// got / n_got: what lc_collect gives after the LAST step.  Returns run_sequence's code.
int lsh_steps(const uint64_t *words, uint32_t n, uint32_t contig, uint32_t qbit, uint32_t rel, const uint32_t *win, int n_win, uint32_t *out, uint64_t *got, uint32_t *n_got)
{
    const std::vector<uint64_t> l(words, words + n);
    LcQuery Q{contig, qbit, rel, n};
    long loads = 0; int oob = 0;
    const Counting lst{l.data(), n, &loads, &oob};
    LcSearch s{};
    for (int i = 0; i < n_win; ++i) {
        const long before = loads;
        if (i == 0) lc_open(s, lst, Q, win[0], win[1]); else lc_grow(s, lst, Q, win[2 * i], win[2 * i + 1]);
        const uint32_t v[8] = {s.first, s.stop, s.c, s.below, s.above, s.nlo, s.nhi, (uint32_t)(loads - before)};
        std::copy(v, v + 8, out + 8 * i);
    }
    *n_got = 0;
    if (s.c <= LC_CAP) lc_collect(s, lst, Q, [&](uint64_t pw) { got[(*n_got)++] = pw; });
    std::vector<std::pair<uint32_t, uint32_t>> w;
    for (int i = 0; i < n_win; ++i) w.push_back({win[2 * i], win[2 * i + 1]});
    return oob ? 1 : run_sequence(l, Q, w);
}

// The edges, each a list built for it and walked through run_sequence; beyond the brute force each asks that the edge itself occurred.
// 0, or 1000 * edge + what failed (run_sequence's code, or 900 + the edge's own property)
int lsh_edges()
{
    const LcQuery Q{4, 0, 0, 0};      // rel 0: the right strand is the seed's own (strand bit 0)
    auto fail = [](int edge, int rc) { return 1000 * edge + rc; };
    std::vector<Step> st;
    int rc;
    {   // 1: growth that reaches index 0 and the list's end, on one contig
        std::vector<uint64_t> l;
        for (uint32_t i = 0; i < 21; ++i) l.push_back(word(4, 1000 + 100 * i, i & 1));
        st.clear();
        if ((rc = run_sequence(l, Q, {{1950, 2050}, {1000, 3000}, {900, 3100}}, &st))) return fail(1, rc);
        if (st[1].first != 0 || st[1].stop != 21 || st[2].loads != 0) return fail(1, 901);
        st.clear();      // ... the head reached exactly at the end of a group of eight, the end one entry past a group
        if ((rc = run_sequence(l, Q, {{1800, 1850}, {1000, 2700}}, &st))) return fail(1, rc);
        if (st[0].first != 8 || st[1].first != 0 || st[1].stop != 18) return fail(1, 902);
    }
    for (uint32_t n : {7u, 8u, 9u, 16u, 17u}) {   // 2: a downward growth that admits exactly n entries; those of the other strand do not count towards the cap
        std::vector<uint64_t> l;
        l.push_back(word(4, 10, 0));
        for (uint32_t i = 0; i < n; ++i) l.push_back(word(4, 1000 + 10 * i, i % 3 == 1));      // a third of them on the other strand
        for (uint32_t i = 0; i < 5; ++i) l.push_back(word(4, 2000 + 10 * i, 0));
        st.clear();
        if ((rc = run_sequence(l, Q, {{2000, 2100}, {1000, 2100}}, &st))) return fail(2, rc);
        const uint32_t right = n - n / 3 - (n % 3 == 2);
        if (st[0].first != n + 1 || st[1].first != 1 || st[1].c != 5 + right || st[1].c > LC_CAP) return fail(2, 900 + (int)n);
    }
    {   // 3: an entry exactly on the new lower key, and one less
        const std::vector<uint64_t> on{word(4, 499, 1), word(4, 500, 0), word(4, 900, 0)}, under{word(4, 499, 0), word(4, 499, 1), word(4, 900, 0)};
        st.clear();
        if ((rc = run_sequence(on, Q, {{800, 1000}, {500, 1000}}, &st))) return fail(3, rc);
        if (st[1].first != 1 || st[1].c != 2) return fail(3, 901);
        st.clear();
        if ((rc = run_sequence(under, Q, {{800, 1000}, {500, 1000}}, &st))) return fail(3, rc);
        if (st[1].first != 2 || st[1].c != 1 || st[1].loads != 0) return fail(3, 902);
    }
    {   // 4: an entry at whi, and at whi + 1
        const std::vector<uint64_t> l{word(4, 900, 0), word(4, 1500, 0), word(4, 1500, 1), word(4, 1501, 0)};
        st.clear();
        if ((rc = run_sequence(l, Q, {{800, 1000}, {800, 1500}, {800, 1501}}, &st))) return fail(4, rc);
        if (st[0].stop != 1 || st[1].stop != 3 || st[1].c != 2 || st[2].stop != 4 || st[2].c != 3) return fail(4, 901);
    }
    {   // 5: the entry just below `first` on the previous contig, its position inside the window; the mirror image above
        const std::vector<uint64_t> l{word(3, 700, 0), word(3, 950, 0), word(4, 900, 0), word(5, 850, 0), word(5, 1100, 0)};
        st.clear();
        if ((rc = run_sequence(l, Q, {{880, 920}, {600, 1200}, {0, 5000}}, &st))) return fail(5, rc);
        if (st[0].first != 2 || st[2].first != 2 || st[2].stop != 3 || st[2].c != 1 || st[1].loads != 0 || st[2].loads != 0) return fail(5, 901);
    }
    for (uint32_t extra : {6u, 7u}) {   // 6: 16 in-window entries reached only cumulatively (10 + 6) are taken, 17 (10 + 7) are not; no step adds more than 16
        std::vector<uint64_t> l;
        for (uint32_t i = 0; i < 4; ++i) l.push_back(word(4, 100 + i, 0));
        for (uint32_t i = 0; i < 10; ++i) l.push_back(word(4, 1000 + 10 * i, 0));
        for (uint32_t i = 0; i < extra - 4; ++i) l.push_back(word(4, 2000 + i, 0));
        l.push_back(word(4, 9000, 0));
        st.clear();
        if ((rc = run_sequence(l, Q, {{1000, 1100}, {100, 2100}}, &st))) return fail(6, rc);
        if (st[0].c != 10 || (extra == 6 ? st[1].c != 16 : st[1].c <= LC_CAP)) return fail(6, 900 + (int)extra);
    }
    {   // 7: a grow whose remembered neighbours make both sides free of loads - in a long list too
        std::vector<uint64_t> l;
        for (uint32_t i = 0; i < 300; ++i) l.push_back(word(4, 100000 + 5000 * i, i & 1));
        st.clear();
        if ((rc = run_sequence(l, Q, {{849000, 851000}, {846000, 854000}, {845001, 854999}}, &st))) return fail(7, rc);
        if (st[0].c != 1 || st[0].loads == 0 || st[1].loads != 0 || st[2].loads != 0 || st[2].c != 1) return fail(7, 901);
        st.clear();      // ... and one side only: the other pays one group of eight
        if ((rc = run_sequence(l, Q, {{849000, 851000}, {845000, 854999}}, &st))) return fail(7, rc);
        if (st[1].loads != 8 || st[1].c != 1 || st[1].first != st[0].first - 1) return fail(7, 902);
    }
    return 0;
}

}

#ifdef LC_SEARCH_MAIN
int main()
{
    int rc = lsh_edges();
    if (rc) { std::printf("lc search: edge %d failed with %d\n", rc / 1000, rc % 1000); return 1; }
    for (uint32_t n : {2u, 7u, 8u, 9u, 15u, 16u, 17u, 63u, 64u, 65u, 511u, 512u, 513u})
        if ((rc = lsh_random(n, 1, 150))) { std::printf("lc search: list of %u, sequence %d failed with %d\n", n, rc / 10000, rc % 10000); return 1; }
    std::printf("lc search ok\n");
    return 0;
}
#endif
