// sh_gunzip.h — one feed of a general gzip stream: the part that is neither kernel nor memory.  It cuts the window of
// compressed bytes into chunks, walks the chain of spans (with the rounds of redone chunks), lays the spans out in the output, and
// checks every member's CRC-32 and ISIZE from the pieces.  The stages themselves - find, size, and the decode (markers, windows, resolve)
// - belong to a backend: the kernels of sh_inflate.hip, or the loops of tests/gunzip_host.cpp over the same SHIN_FN code.  So the device
// path and its host mirror share every decision made here, and the CPU tests and the sanitizer see it.
#pragma once
#include "sh_inflate.h"
#include <algorithm>
#include <vector>

namespace shgz {

constexpr uint32_t MAX_ROUNDS = 8;                                    // launches of the size pass per feed; what is still open then goes to zlib
constexpr uint32_t MIN_CHUNK = 1u << 10, MAX_CHUNK = 1u << 20, DEFAULT_CHUNK = 16u << 10;
constexpr uint32_t MAX_PIECES = SHIN_MAX_ENDS + 1;                   // CRC pieces of a span: one per member it touches

struct Job { uint64_t start_bit, stop_bit; uint32_t at_header, pad; };
// a span of the chain: where it decodes, where its bytes go, how much of the window before it is the open member's, and its pieces
// seg[k] .. seg[k + 1]
struct Item { uint64_t start_bit, stop_bit, out_off; uint32_t at_header, produced, valid_in, n_seg; uint32_t seg[MAX_PIECES + 1]; uint32_t pad; };

enum Outcome {
    FEED_OK = 0,
    FEED_ROUNDS = 1,       // MAX_ROUNDS rounds left a chunk open: the caller's fallback; what the chain held before is delivered
    FEED_ENDS = 2,         // more than SHIN_MAX_ENDS members end in one span: likewise
    FEED_DATA = 3,         // Feed::status at file offset Feed::err_off
    FEED_TRUNCATED = 4,    // last, and the stream does not end at a member end
    FEED_NOT_GZIP = 5,
    FEED_OUT_CAP = 6,      // the first span alone holds Feed::need bytes
    FEED_BACKEND = 7       // Feed::backend_rc
};

struct Counts { uint64_t n_chunks, n_skipped, n_redone, n_rounds, n_members, n_marker_symbols, n_window_steps, in_bytes, out_bytes; };

// one gzip file being read; the 32 KiB of output before the resume point are the backend's
struct State {
    uint32_t chunk_bytes = DEFAULT_CHUNK, resume_bit = 0;
    bool at_header = true, ended = false;
    uint32_t win_valid = 0, crc = 0;          // of the open member: bytes of the window that are its own, CRC-32 and length so far
    uint64_t len = 0, file_off = 0, member_off = 0, n_members = 0;      // file_off: of the next feed's first byte; both may be seeded with where the stream begins in its file
};

struct Feed {
    uint64_t consumed = 0, out_len = 0, err_off = 0, need = 0;
    uint32_t status = SHIN_OK;
    int backend_rc = 0;
    Counts c{};
};

// 128 bits of in[0, n) from bit position p on, zeros behind the input
inline uint64_t load64(const uint8_t *in, uint64_t n, uint64_t byte)
{
    uint64_t v = 0;
    for (uint32_t i = 0; i < 8 && byte + i < n; ++i) v |= (uint64_t)in[byte + i] << (8 * i);
    return v;
}

// Backend:
//   int find(uint32_t chunk_bytes, uint32_t n_chunks, uint64_t *found)             found[j], j >= 1: the first candidate in chunk j or SHIN_NO_START
//   int size(const Job *jobs, uint32_t n_jobs, ShinSpan *res)                        the size pass over the jobs
//   int decode(const Item *items, uint32_t m, uint64_t total, ShinSpan *res, uint32_t *bad, uint32_t *crc, uint64_t *n_markers)
//                                                                                    markers, windows, resolve: total bytes out, crc[i * MAX_PIECES + k]
// each returns 0 or what Feed::backend_rc reports.  The input window of n bytes, `last` and the output are the backend's own.
template <class B>
Outcome feed(State &S, B &be, uint64_t n, bool last, uint64_t out_cap, const uint64_t *given_starts, Feed &F)
{
    F = Feed{};
    if (S.ended) { F.consumed = n; return FEED_OK; }
    if (n == 0) {
        if (!last) return FEED_OK;
        if (S.at_header && S.n_members == 0) { S.ended = true; return FEED_OK; }      // an empty file is an empty stream, as for gzread
        F.err_off = S.file_off;
        return FEED_TRUNCATED;
    }
    const uint64_t C = S.chunk_bytes, n_bits = 8 * n;
    const uint32_t n_chunks = (uint32_t)((n + C - 1) / C);
    auto stop_of = [&](uint32_t j) { return std::min<uint64_t>(8 * C * (j + 1), n_bits); };
    std::vector<uint64_t> start(n_chunks, SHIN_NO_START);
    std::vector<uint8_t> done(n_chunks, 0);
    std::vector<ShinSpan> res(n_chunks), got;
    std::vector<Job> jobs;
    std::vector<uint32_t> todo, chain;
    if (given_starts) {
        for (uint32_t j = 1; j < n_chunks; ++j)
            if (given_starts[j] >= 8 * C * j && given_starts[j] < stop_of(j)) start[j] = given_starts[j];
    } else if (n_chunks > 1 && (F.backend_rc = be.find((uint32_t)C, n_chunks, start.data())) != 0) return FEED_BACKEND;
    start[0] = S.at_header ? 0 : S.resume_bit;
    for (uint32_t j = 0; j < n_chunks; ++j) if (start[j] != SHIN_NO_START) todo.push_back(j);

    bool confirmed = false;
    uint32_t terminal = SHIN_OK, term_chunk = 0;
    for (uint32_t round = 0; round < MAX_ROUNDS && !confirmed; ++round) {
        jobs.clear();
        for (uint32_t j : todo) jobs.push_back(Job{start[j], stop_of(j), j == 0 && S.at_header ? 1u : 0u, 0});
        got.resize(jobs.size());
        if ((F.backend_rc = be.size(jobs.data(), (uint32_t)jobs.size(), got.data())) != 0) return FEED_BACKEND;
        for (size_t i = 0; i < todo.size(); ++i) { res[todo[i]] = got[i]; done[todo[i]] = 1; }
        ++F.c.n_rounds;
        if (round) F.c.n_redone += todo.size();
        todo.clear(); chain.clear();
        // From chunk 0 along the end bits.  Up to the first chunk that does not start where its predecessor ended the chain is confirmed;
        // behind it the walk goes on from the next chunk that has a result, so that every such chunk of this round is redone in the next.
        // A tentative span may itself come from a false or stale start: its end bit then replaces the start of the chunk it falls in,
        // a right one possibly, and that chunk costs a second round when the confirmed walk reaches it.  MAX_ROUNDS covers it.
        confirmed = true;
        terminal = SHIN_OK;
        for (uint32_t cur = 0;;) {
            const ShinSpan &r = res[cur];
            if (confirmed && (r.status == SHIN_OK || r.status == SHIN_SPAN_END)) chain.push_back(cur);
            if (r.status != SHIN_OK && confirmed) { terminal = r.status; term_chunk = cur; break; }
            uint32_t nj = cur;      // a tentative span that fails is passed over
            if (r.status == SHIN_OK) {
                const uint64_t e = r.end_bit;
                if (e >= n_bits) break;
                nj = (uint32_t)(e / (8 * C));
                if (done[nj] && start[nj] == e) { cur = nj; continue; }
                start[nj] = e; done[nj] = 0;
                todo.push_back(nj);
                confirmed = false;
            }
            for (++nj; nj < n_chunks && !done[nj]; ++nj) {}
            if (nj == n_chunks) break;
            cur = nj;
        }
    }
    Outcome fallback = FEED_OK;
    if (!confirmed) fallback = FEED_ROUNDS;      // chain holds what the last walk confirmed
    else switch (terminal) {
    case SHIN_OK:      // the window ends at a block boundary inside a member
        if (last) { F.err_off = S.file_off + n; return FEED_TRUNCATED; }
        break;
    case SHIN_MANY_ENDS: fallback = FEED_ENDS; break;
    case SHIN_IN_OVERRUN:
        if (last) { F.err_off = S.file_off + (start[term_chunk] >> 3); return FEED_TRUNCATED; }
        break;
    case SHIN_SPAN_END:
        // without a member end it is chunk 0 at a header that is none, and only a stream's first feed starts at a header (later
        // headers are parsed by the span that ends the member before them)
        if (res[term_chunk].n_ends == 0) { F.err_off = S.file_off; return FEED_NOT_GZIP; }
        break;
    default: F.status = terminal; F.err_off = S.member_off; return FEED_DATA;
    }

    // as many spans as out_cap holds
    uint32_t m = 0;
    uint64_t total = 0;
    while (m < chain.size() && total + res[chain[m]].produced <= out_cap) total += res[chain[m++]].produced;
    if (!chain.empty() && m == 0) { F.need = res[chain[0]].produced; return FEED_OUT_CAP; }
    const bool cut = m < chain.size();
    if (m == 0) return fallback;

    std::vector<Item> items(m);
    uint32_t valid = S.win_valid;
    total = 0;
    for (uint32_t i = 0; i < m; ++i) {
        const uint32_t j = chain[i];
        const ShinSpan &r = res[j];
        Item &it = items[i];
        it = Item{start[j], stop_of(j), total, j == 0 && S.at_header ? 1u : 0u, r.produced, valid, r.n_ends + 1, {0}, 0};
        for (uint32_t k = 0; k < r.n_ends; ++k) it.seg[k + 1] = r.ends[k].out_off;
        it.seg[r.n_ends + 1] = r.produced;
        valid = (uint32_t)std::min<uint64_t>(SHIN_WINDOW, r.n_ends ? r.produced - r.ends[r.n_ends - 1].out_off : (uint64_t)valid + r.produced);
        total += r.produced;
    }
    std::vector<ShinSpan> again(m);
    std::vector<uint32_t> bad(m, 0), crc((size_t)m * MAX_PIECES, 0);
    if ((F.backend_rc = be.decode(items.data(), m, total, again.data(), bad.data(), crc.data(), &F.c.n_marker_symbols)) != 0) return FEED_BACKEND;

    State T = S;
    for (uint32_t i = 0; i < m; ++i) {
        const ShinSpan &r = res[chain[i]], &a = again[i];
        if (a.status != r.status || a.produced != r.produced || a.end_bit != r.end_bit || a.n_ends != r.n_ends) { F.status = SHIN_SIZE_DIFFERS; F.err_off = T.member_off; return FEED_DATA; }
        if (bad[i]) { F.status = bad[i]; F.err_off = T.member_off; return FEED_DATA; }
        for (uint32_t k = 0; k <= r.n_ends; ++k) {
            const uint32_t piece = items[i].seg[k + 1] - items[i].seg[k];
            T.crc = shin_crc_shift(T.crc, piece) ^ crc[(size_t)i * MAX_PIECES + k];
            T.len += piece;
            if (k == r.n_ends) break;
            if (T.crc != r.ends[k].crc32 || (uint32_t)T.len != r.ends[k].isize) { F.status = T.crc != r.ends[k].crc32 ? SHIN_CRC : SHIN_ISIZE; F.err_off = T.member_off; return FEED_DATA; }
            T.member_off = T.file_off + r.ends[k].end_byte;
            T.crc = 0; T.len = 0;
            ++T.n_members; ++F.c.n_members;
        }
    }
    const ShinSpan &tail = res[chain[m - 1]];
    T.win_valid = valid;
    if (!cut && tail.status == SHIN_SPAN_END) { T.ended = true; F.consumed = n; }
    else { F.consumed = tail.end_bit >> 3; T.resume_bit = (uint32_t)(tail.end_bit & 7); }
    T.at_header = false;
    T.file_off += F.consumed;
    S = T;
    F.out_len = total;
    F.c.n_chunks = m; F.c.n_skipped = chain[m - 1] + 1 - m; F.c.n_window_steps = m;
    F.c.in_bytes = F.consumed; F.c.out_bytes = total;
    return cut ? FEED_OK : fallback;
}

}      // namespace shgz
