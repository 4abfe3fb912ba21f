// Host mirror of the general-gzip path (scrubby_amd/csrc/sh_gunzip.h over sh_inflate.h) for tests/test_gunzip_cpu.py: the chain walk, the
// layout and the CRC check are the very code the device path runs (shgz::feed); the stages are loops over the SHIN_FN functions the
// kernels call - the candidate test, the span decoder with the size and the marker sink, the window step, the resolve step.  Input,
// output and symbols live in heap blocks of exactly their sizes, so a sanitizer build sees any access outside them.
// With -DGUNZIP_MAIN the file is a program of its own that makes its streams with zlib and runs the table of cases: the sanitizer build.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>
#include "../scrubby_amd/csrc/sh_gunzip.h"

namespace {

struct HostSrc {
    const uint8_t *p;
    uint32_t byte(uint32_t pos) { return p[pos]; }
};
struct MarkSink {
    uint16_t *out;
    const uint8_t *in;
    uint32_t pos;
    void lit(uint32_t c) { out[pos++] = (uint16_t)c; }
    void match(uint32_t len, uint32_t dist) { for (uint32_t i = 0; i < len; ++i, ++pos) out[pos] = (uint16_t)(pos < dist ? shin_marker(pos, dist) : out[pos - dist]); }
    void raw(uint32_t in_pos, uint32_t n) { for (uint32_t i = 0; i < n; ++i) out[pos++] = in[in_pos + i]; }
};

// the first candidate of bit positions [lo_bit, hi_bit), as the lanes of k_gz_find test them: the quick test on 128 bits, then the decoder's own
uint64_t first_candidate(const uint8_t *in, uint64_t n, uint64_t lo_bit, uint64_t hi_bit, ShinTables *T, uint64_t *kinds)
{
    HostSrc src{in};
    for (uint64_t byte = lo_bit >> 3; byte < (hi_bit + 7) >> 3; ++byte) {
        const uint64_t w0 = shgz::load64(in, n, byte), w1 = shgz::load64(in, n, byte + 8), w2 = shgz::load64(in, n, byte + 16);
        for (uint32_t k = 0; k < 8; ++k) {
            const uint64_t p = 8 * byte + k;
            if (p < lo_bit || p >= hi_bit) continue;
            const uint64_t lo = k ? w0 >> k | w1 << (64 - k) : w0, hi = k ? w1 >> k | w2 << (64 - k) : w1;
            const uint32_t q = shin_candidate_quick(lo, hi, 8 * n - p, k);
            if (q == 0) continue;
            const bool full = shin_block_candidate(src, (uint32_t)n, p, T);
            if (q == 2 && !full) return ~1ull;      // the two tests must agree on a stored block
            if (!full) continue;
            if (!kinds) return p;
            ++kinds[q == 1 ? 0 : ((lo >> (3 + ((8 - ((k + 3) & 7)) & 7))) & 0xffff) ? 2 : 1];
        }
    }
    return SHIN_NO_START;
}

struct HostBackend {
    const uint8_t *in = nullptr;
    uint64_t n = 0;
    bool last = false;
    uint8_t *out = nullptr;
    std::vector<uint8_t> window = std::vector<uint8_t>(SHIN_WINDOW, 0);
    std::unique_ptr<ShinTables> T = std::make_unique<ShinTables>();
    uint32_t crc_table[256];
    HostBackend() { for (uint32_t i = 0; i < 256; ++i) crc_table[i] = shin_crc_table_entry(i); }

    int find(uint32_t C, uint32_t n_chunks, uint64_t *found)
    {
        for (uint32_t j = 1; j < n_chunks; ++j) {
            found[j] = first_candidate(in, n, 8ull * C * j, std::min<uint64_t>(8ull * C * (j + 1), 8 * n), T.get(), nullptr);
            if (found[j] == ~1ull) return 1;
        }
        return 0;
    }
    int size(const shgz::Job *jobs, uint32_t n_jobs, ShinSpan *res)
    {
        HostSrc src{in};
        for (uint32_t i = 0; i < n_jobs; ++i) {
            ShinSizeSink sink;
            shin_inflate_span(src, (uint32_t)n, last, jobs[i].start_bit, jobs[i].at_header != 0, jobs[i].stop_bit, sink, SHIN_SPAN_MAX_OUT, T.get(), &res[i], res[i].ends);
        }
        return 0;
    }
    int decode(const shgz::Item *items, uint32_t m, uint64_t total, ShinSpan *res, uint32_t *bad, uint32_t *crc, uint64_t *n_markers)
    {
        HostSrc src{in};
        std::unique_ptr<uint16_t[]> sym(new uint16_t[total ? total : 1]);      // exact extent
        std::vector<uint8_t> wins((size_t)(m + 1) * SHIN_WINDOW);
        memcpy(wins.data(), window.data(), SHIN_WINDOW);
        for (uint32_t i = 0; i < m; ++i) {
            const shgz::Item &it = items[i];
            MarkSink sink{sym.get() + it.out_off, in, 0};
            shin_inflate_span(src, (uint32_t)n, last, it.start_bit, it.at_header != 0, it.stop_bit, sink, it.produced, T.get(), &res[i], res[i].ends);
        }
        for (uint32_t i = 0; i < m; ++i) {      // the serial chain
            const shgz::Item &it = items[i];
            if (res[i].produced != it.produced) continue;      // the feed refuses it
            const uint8_t *prev = wins.data() + (size_t)i * SHIN_WINDOW;
            for (uint32_t b = 0; b < SHIN_WINDOW; ++b) wins[(size_t)(i + 1) * SHIN_WINDOW + b] = (uint8_t)shin_window_byte(b, prev, it.valid_in, sym.get() + it.out_off, it.produced, &bad[i]);
        }
        *n_markers = 0;
        for (uint32_t i = 0; i < m; ++i) {
            const shgz::Item &it = items[i];
            if (res[i].produced != it.produced) continue;
            const uint8_t *win = wins.data() + (size_t)i * SHIN_WINDOW;
            for (uint32_t p = 0; p < it.produced; ++p) {
                const uint32_t s = sym[it.out_off + p];
                *n_markers += s >= 256;
                out[it.out_off + p] = (uint8_t)shin_resolve(s, win, it.valid_in, &bad[i]);
            }
            for (uint32_t k = 0; k < it.n_seg; ++k) crc[(size_t)i * shgz::MAX_PIECES + k] = shin_crc_piece(crc_table, out + it.out_off + it.seg[k], it.seg[k + 1] - it.seg[k]);
        }
        memcpy(window.data(), wins.data() + (size_t)m * SHIN_WINDOW, SHIN_WINDOW);
        return 0;
    }
};

struct HostGunzip { shgz::State S; HostBackend be; };

}      // namespace

extern "C" void *gzh_open(uint32_t chunk_bytes)
{
    HostGunzip *g = new HostGunzip;
    g->S.chunk_bytes = chunk_bytes ? chunk_bytes : shgz::DEFAULT_CHUNK;
    return g;
}
extern "C" void gzh_close(void *h) { delete (HostGunzip *)h; }
extern "C" uint32_t gzh_max_rounds() { return shgz::MAX_ROUNDS; }

// One feed -> the outcome (shgz::Outcome).  starts: null, or one bit position per chunk (~0: none).  counts[9]: shgz::Counts;
// err[3]: status, file offset, bytes needed.  out receives out_len bytes (out_cap of room).
extern "C" int gzh_feed(void *h, const uint8_t *in, uint64_t n, int last, uint8_t *out, uint64_t out_cap, const uint64_t *starts, uint64_t *consumed, uint64_t *out_len,
                        uint64_t *counts, uint64_t *err)
{
    HostGunzip *g = (HostGunzip *)h;
    std::unique_ptr<uint8_t[]> zin(new uint8_t[n ? n : 1]), zout(new uint8_t[out_cap ? out_cap : 1]);      // exact extents
    if (n) memcpy(zin.get(), in, n);
    g->be.in = zin.get(); g->be.n = n; g->be.last = last != 0; g->be.out = zout.get();
    shgz::Feed F;
    const shgz::Outcome rc = shgz::feed(g->S, g->be, n, last != 0, out_cap, starts, F);
    if (F.out_len) memcpy(out, zout.get(), F.out_len);
    *consumed = F.consumed; *out_len = F.out_len;
    if (counts) memcpy(counts, &F.c, sizeof F.c);
    if (err) { err[0] = F.status; err[1] = F.err_off; err[2] = F.need; }
    g->be.in = nullptr; g->be.out = nullptr;
    return (int)rc;
}

// what the find stage gives: found[j], j >= 1, the first candidate of chunk j
extern "C" int gzh_find(const uint8_t *in, uint64_t n, uint32_t chunk_bytes, uint64_t *found)
{
    HostBackend be;
    be.in = in; be.n = n;
    return be.find(chunk_bytes, (uint32_t)((n + chunk_bytes - 1) / chunk_bytes), found);
}

// every candidate of in[0, n) by kind -> kinds[3]: dynamic, empty stored, non-empty stored
extern "C" int gzh_candidates(const uint8_t *in, uint64_t n, uint64_t *kinds)
{
    auto T = std::make_unique<ShinTables>();
    kinds[0] = kinds[1] = kinds[2] = 0;
    return first_candidate(in, n, 0, 8 * n, T.get(), kinds) == SHIN_NO_START ? 0 : 1;
}

#ifdef GUNZIP_MAIN
#include <zlib.h>
#include <string>

namespace {

typedef std::vector<uint8_t> Bytes;

// one gzip member by zlib; flush_at > 0: a flush of that kind after so many bytes; fields: FEXTRA + FNAME + FCOMMENT + FHCRC; name_len: FNAME of that length
Bytes gz(const Bytes &data, int level, int strategy = Z_DEFAULT_STRATEGY, size_t flush_at = 0, int flush = Z_SYNC_FLUSH, bool fields = false, size_t name_len = ~(size_t)0)
{
    z_stream zs{};
    deflateInit2(&zs, level, Z_DEFLATED, 15 + 16, 8, strategy);
    gz_header hd{};
    static const unsigned char extra[5] = {'X', 'Y', 1, 0, 7};
    if (fields) {
        hd.extra = (Bytef *)extra; hd.extra_len = 5; hd.name = (Bytef *)"reads.fastq"; hd.comment = (Bytef *)"a comment"; hd.hcrc = 1; hd.os = 3;
        deflateSetHeader(&zs, &hd);
    }
    const std::string name(name_len == ~(size_t)0 ? 0 : name_len, 'n');
    if (name_len != ~(size_t)0) { hd.name = (Bytef *)name.c_str(); hd.os = 3; deflateSetHeader(&zs, &hd); }
    Bytes out(deflateBound(&zs, (uLong)data.size()) + 2048);
    zs.next_out = out.data(); zs.avail_out = (uInt)out.size();
    zs.next_in = (Bytef *)data.data();
    if (flush_at && flush_at < data.size()) { zs.avail_in = (uInt)flush_at; deflate(&zs, flush); }
    zs.avail_in = (uInt)(data.data() + data.size() - zs.next_in);
    deflate(&zs, Z_FINISH);
    out.resize(zs.total_out);
    deflateEnd(&zs);
    return out;
}

// what gzread gives for the file: members one after another, a tail that is no gzip member ignored; false: an error
bool zlib_gunzip(const Bytes &file, Bytes *out)
{
    out->clear();
    z_stream zs{};
    inflateInit2(&zs, 15 + 16);
    zs.next_in = (Bytef *)file.data(); zs.avail_in = (uInt)file.size();
    Bytes buf(1 << 16);
    bool ok = false;
    for (bool first = true;; first = false) {
        if (zs.avail_in < 2 || zs.next_in[0] != 0x1f || zs.next_in[1] != 0x8b) { ok = !first || file.empty(); break; }
        int rc = Z_OK;
        while (rc == Z_OK) {
            zs.next_out = buf.data(); zs.avail_out = (uInt)buf.size();
            rc = inflate(&zs, Z_NO_FLUSH);
            out->insert(out->end(), buf.data(), buf.data() + (buf.size() - zs.avail_out));
            if (rc == Z_OK && zs.avail_in == 0 && zs.avail_out != 0) rc = Z_BUF_ERROR;
        }
        if (rc != Z_STREAM_END) break;
        inflateReset(&zs);
    }
    inflateEnd(&zs);
    return ok;
}

Bytes fastq_like(size_t n, uint32_t seed)
{
    std::string s;
    uint32_t x = seed * 2654435761u + 1;
    auto rnd = [&] { x ^= x << 13; x ^= x >> 17; x ^= x << 5; return x; };
    for (uint32_t i = 0; s.size() < n; ++i) {
        s += "@A00123:45:HXXXXXXX:" + std::to_string(1 + i % 4) + ":" + std::to_string(1101 + i / 977) + ":" + std::to_string(1000 + rnd() % 29000) + ":" + std::to_string(1000 + rnd() % 29000) + " 1:N:0:ACGTACGT\n";
        for (int k = 0; k < 150; ++k) s += "ACGT"[rnd() & 3];
        s += "\n+\n";
        for (int k = 0; k < 150; ++k) { const uint32_t r = rnd() % 100; s += r < 60 ? 'F' : r < 85 ? ':' : r < 95 ? ',' : '#'; }
        s += "\n";
    }
    s.resize(n);
    return Bytes(s.begin(), s.end());
}

int n_case = 0, n_bad = 0;

struct Run { int outcome; Bytes out; uint64_t counts[9]; uint64_t err[3]; };

// the whole file through feeds of `step` compressed bytes (0: one feed), the unconsumed rest presented again
Run run(const Bytes &file, uint32_t chunk, size_t step = 0, uint64_t out_cap = 4ull << 20, const uint64_t *starts = nullptr)
{
    Run r{};
    void *h = gzh_open(chunk);
    Bytes out(out_cap);
    size_t lo = 0, hi = step ? std::min(step, file.size()) : file.size();
    for (;;) {
        uint64_t consumed = 0, out_len = 0, counts[9];
        const int last = hi == file.size();
        r.outcome = gzh_feed(h, file.data() + lo, hi - lo, last, out.data(), out_cap, starts, &consumed, &out_len, counts, r.err);
        r.out.insert(r.out.end(), out.data(), out.data() + out_len);
        for (int i = 0; i < 9; ++i) r.counts[i] = i == 3 ? std::max(r.counts[i], counts[i]) : r.counts[i] + counts[i];
        if (r.outcome != shgz::FEED_OK) break;
        lo += consumed;
        if (last && (lo == hi || (consumed == 0 && out_len == 0))) break;      // else the output was full: the rest again
        if (!last) hi = std::min(file.size(), hi + step);
    }
    gzh_close(h);
    return r;
}

// a good stream: zlib's bytes, no fallback, the rounds below the bound
void good(const char *name, const Bytes &file, uint32_t chunk, size_t step = 0, uint64_t out_cap = 4ull << 20, bool may_fall_back = false)
{
    ++n_case;
    Bytes want;
    const bool zok = zlib_gunzip(file, &want);
    const Run r = run(file, chunk, step, out_cap);
    const bool fell = r.outcome == shgz::FEED_ROUNDS || r.outcome == shgz::FEED_ENDS;
    bool ok = zok && (r.outcome == shgz::FEED_OK ? r.out == want : may_fall_back && fell && r.out.size() <= want.size() && std::equal(r.out.begin(), r.out.end(), want.begin()));
    if (!may_fall_back && r.counts[3] >= shgz::MAX_ROUNDS) ok = false;
    if (!ok) { std::printf("%s (chunk %u, step %zu): outcome %d, %zu of %zu bytes, %llu rounds\n", name, chunk, step, r.outcome, r.out.size(), want.size(), (unsigned long long)r.counts[3]); ++n_bad; }
}

// a damaged stream: an error, or zlib's bytes
void damaged(const char *name, const Bytes &file, uint32_t chunk, bool must_fail)
{
    ++n_case;
    Bytes want;
    const bool zok = zlib_gunzip(file, &want);
    const Run r = run(file, chunk);
    const bool fell = r.outcome == shgz::FEED_ROUNDS || r.outcome == shgz::FEED_ENDS;
    // a fallback hands out what it decoded before: a prefix of what zlib gives before its own end or error
    const bool ok = r.outcome == shgz::FEED_OK ? !must_fail && zok && r.out == want : fell ? r.out.size() <= want.size() && std::equal(r.out.begin(), r.out.end(), want.begin()) : true;
    if (!ok) { std::printf("%s: outcome %d, zlib %s, %zu bytes against %zu\n", name, r.outcome, zok ? "ok" : "error", r.out.size(), want.size()); ++n_bad; }
}

Bytes cat(std::initializer_list<Bytes> parts)
{
    Bytes f;
    for (const Bytes &p : parts) f.insert(f.end(), p.begin(), p.end());
    return f;
}

}      // namespace

int main()
{
    const Bytes text = fastq_like(1 << 20, 1);
    for (int level : {1, 6, 9})
        for (uint32_t chunk : {1u << 10, 4u << 10, 16u << 10}) good("level 1 / 6 / 9", gz(text, level), chunk);
    good("feeds of 100 000 bytes, output for 300 000", gz(text, 6), 4 << 10, 100000, 300000);
    good("sync flush", gz(text, 6, Z_DEFAULT_STRATEGY, 500000, Z_SYNC_FLUSH), 4 << 10);
    good("full flush", gz(text, 6, Z_DEFAULT_STRATEGY, 500000, Z_FULL_FLUSH), 4 << 10);
    for (uint32_t chunk : {1u << 10, 16u << 10}) good("level 0", gz(text, 0), chunk);
    good("fixed blocks only", gz(text, 6, Z_FIXED), 4 << 10, 0, 4ull << 20, true);
    const Bytes part(text.begin(), text.begin() + 200000), none;
    good("three members, one empty", cat({gz(part, 6), gz(none, 6), gz(part, 1)}), 4 << 10);
    good("six members of 100 bytes in one span", cat({gz(Bytes(100, 'x'), 6), gz(Bytes(100, 'x'), 6), gz(Bytes(100, 'x'), 6), gz(Bytes(100, 'x'), 6), gz(Bytes(100, 'x'), 6), gz(Bytes(100, 'x'), 6)}),
         1 << 10, 0, 4ull << 20, true);
    good("header fields", cat({gz(part, 6, Z_DEFAULT_STRATEGY, 0, 0, true), gz(part, 9, Z_DEFAULT_STRATEGY, 0, 0, true)}), 4 << 10);
    {
        Bytes unit(30000), rep;
        uint32_t x = 5;
        for (auto &c : unit) { x = x * 1664525u + 1013904223u; c = "ACGT"[x >> 30]; }
        for (int i = 0; i < 40; ++i) rep.insert(rep.end(), unit.begin(), unit.end());
        good("30 000 bytes over four letters, 40 times", gz(rep, 6), 1 << 10);
        Bytes block(20000), rep2;
        for (auto &c : block) { x = x * 1664525u + 1013904223u; c = (uint8_t)(x >> 24); }
        for (int i = 0; i < 100; ++i) rep2.insert(rep2.end(), block.begin(), block.end());
        good("a random block of 20 000 bytes, 100 times", gz(rep2, 6), 1 << 10);
        good("a run of A", gz(Bytes(3 << 20, 'A'), 6), 1 << 10);
    }
    {      // a member end in the last byte of a chunk: a file name in the header makes the first member a multiple of 1024 bytes
        const size_t plain = gz(part, 6).size();
        const Bytes first = gz(part, 6, Z_DEFAULT_STRATEGY, 0, 0, false, (1024 - (plain + 1) % 1024) % 1024);
        if (first.size() % 1024 != 0) { std::printf("member end: %zu bytes\n", first.size()); ++n_bad; }
        good("a member end in the last byte of a chunk", cat({first, gz(part, 6)}), 1 << 10);
    }
    good("100 zero bytes behind the last member", cat({gz(part, 6), Bytes(100, 0)}), 4 << 10);
    good("100 other bytes behind the last member", cat({gz(part, 6), Bytes(100, 'q')}), 4 << 10);
    const Bytes small(text.begin(), text.begin() + 120000), file = gz(small, 6);
    uint32_t x = 99;
    for (int i = 0; i < 200; ++i) {
        x = x * 1664525u + 1013904223u;
        Bytes f = file;
        const size_t bit = x % (f.size() * 8);
        f[bit >> 3] ^= (uint8_t)(1u << (bit & 7));
        damaged("one bit flipped", f, 1 << 10, false);
    }
    for (int i = 0; i < 50; ++i) {
        x = x * 1664525u + 1013904223u;
        damaged("cut", Bytes(file.begin(), file.begin() + 1 + x % (file.size() - 1)), 1 << 10, true);
    }
    {
        ++n_case;
        const uint32_t chunk = 1 << 10, n_chunks = (uint32_t)((file.size() + chunk - 1) / chunk);
        const Run plain = run(file, chunk);
        std::vector<uint64_t> starts(n_chunks, SHIN_NO_START);
        gzh_find(file.data(), file.size(), chunk, starts.data());
        // every third chunk that has a start gets a random position of its own range instead
        uint64_t n_wrong = 0, k = 0;
        for (uint32_t j = 1; j < n_chunks; ++j)
            if (starts[j] != SHIN_NO_START && k++ % 3 == 0) { x = x * 1664525u + 1013904223u; starts[j] = 8ull * chunk * j + (starts[j] + 1 + x % (8 * chunk - 1)) % (8 * chunk); ++n_wrong; }
        const Run r = run(file, chunk, 0, 4ull << 20, starts.data());
        if (plain.outcome != shgz::FEED_OK || plain.out != small) { std::printf("wrong starts: the plain run\n"); ++n_bad; }
        else if (r.outcome != shgz::FEED_OK || r.out != small) { std::printf("wrong starts: outcome %d\n", r.outcome); ++n_bad; }
        else if (r.counts[2] < n_wrong) { std::printf("wrong starts: %llu redone, %llu wrong\n", (unsigned long long)r.counts[2], (unsigned long long)n_wrong); ++n_bad; }
    }
    if (n_bad) return 1;
    std::printf("%d cases ok\n", n_case);
    return 0;
}
#endif
