// Host build of the BGZF / DEFLATE decoder's pure parts (scrubby_amd/csrc/sh_inflate.h) for tests/test_inflate_cpu.py: the member scan,
// the decode tables, the block decoder over a sink that writes bytes, and CRC-32 in 64 pieces - the code every lane of k_inflate_member
// runs.  The input and output of a member are copied into heap blocks of exactly their sizes, so a sanitizer build sees any access
// outside the two extents.
// With -DINFLATE_MAIN the file is a program of its own that makes its members with zlib (and, for the 15-bit code, with dfh_encode of
// tests/deflate_host.cpp, which is then compiled into the program) and runs valid and corrupt ones: the sanitizer build.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>
#include "../scrubby_amd/csrc/sh_inflate.h"

namespace {

struct HostSrc {
    const uint8_t *p;
    uint32_t byte(uint32_t pos) { return p[pos]; }
};
struct HostSink {
    uint8_t *out;
    const uint8_t *in;
    uint32_t pos;
    void lit(uint32_t c) { out[pos++] = (uint8_t)c; }
    void match(uint32_t len, uint32_t dist) { for (uint32_t i = 0; i < len; ++i, ++pos) out[pos] = out[pos - dist]; }
    void raw(uint32_t in_pos, uint32_t n) { memcpy(out + pos, in + in_pos, n); pos += n; }
};

// the device's way: 64 equal pieces, each shifted by the bytes behind it
uint32_t crc_in_pieces(const uint8_t *p, uint32_t n)
{
    uint32_t table[256];
    for (uint32_t i = 0; i < 256; ++i) table[i] = shin_crc_table_entry(i);
    const uint32_t piece = (n + 63) / 64;
    uint32_t crc = 0;
    for (uint32_t lane = 0; lane < 64; ++lane) {
        const uint32_t lo = lane * piece < n ? lane * piece : n, hi = lo + piece < n ? lo + piece : n;
        if (hi > lo) crc ^= shin_crc_shift(shin_crc_piece(table, p + lo, hi - lo), n - hi);
    }
    return crc;
}

}      // namespace

extern "C" int inh_scan(const uint8_t *buf, uint64_t n, ShinMember *members, uint64_t cap, uint64_t *n_members, uint64_t *consumed)
{
    return shin_bgzf_scan(buf, n, members, cap, n_members, consumed);
}

// kind: 0 code-length code, 1 literal/length, 2 distance
extern "C" int inh_build(const uint8_t *lens, uint32_t n, int kind)
{
    auto T = std::make_unique<ShinTables>();
    if (kind == SHIN_KIND_CL) return shin_build_table(lens, n, SHIN_CL_BITS, kind, T->cl_fast, T->cl_sorted, T->cl_count, T->offs);
    if (kind == SHIN_KIND_LIT) return shin_build_table(lens, n, SHIN_LIT_BITS, kind, T->lit_fast, T->lit_sorted, T->lit_count, T->offs);
    return shin_build_table(lens, n, SHIN_DIST_BITS, kind, T->dist_fast, T->dist_sorted, T->dist_count, T->offs);
}

extern "C" uint32_t inh_crc(const uint8_t *p, uint32_t n) { return crc_in_pieces(p, n); }

// One member's raw DEFLATE data -> out[0, out_len).  info[5]: status, bytes produced, stored / fixed / dynamic blocks.  The status: the
// decoder's, or SHIN_CRC when it ended well and the bytes do not have `crc`.  `out` receives what was produced (out_len bytes of room).
extern "C" int inh_inflate(const uint8_t *in, uint32_t in_len, uint8_t *out, uint32_t out_len, uint32_t crc, uint32_t *info)
{
    std::unique_ptr<uint8_t[]> zin(new uint8_t[in_len ? in_len : 1]), zout(new uint8_t[out_len ? out_len : 1]);      // exact extents
    if (in_len) memcpy(zin.get(), in, in_len);
    auto T = std::make_unique<ShinTables>();
    HostSrc src{in_len ? zin.get() : nullptr};
    HostSink sink{out_len ? zout.get() : nullptr, src.p, 0};
    ShinResult r;
    shin_inflate_member(src, in_len, sink, out_len, T.get(), &r);
    if (r.status == SHIN_OK && crc_in_pieces(zout.get(), r.produced) != crc) r.status = SHIN_CRC;
    if (out && r.produced) memcpy(out, zout.get(), r.produced);
    if (info) { info[0] = r.status; info[1] = r.produced; info[2] = r.n_stored; info[3] = r.n_fixed; info[4] = r.n_dynamic; }
    return (int)r.status;
}

#ifdef INFLATE_MAIN
#include <zlib.h>
#include <string>

extern "C" int dfh_encode(const uint32_t *tok, uint64_t n_tok, uint8_t *out, uint64_t cap, uint64_t *out_len, uint8_t *lit_lens_out, uint8_t *dist_lens_out);

namespace {

typedef std::vector<uint8_t> Bytes;

uint32_t crc_of(const Bytes &d) { return d.empty() ? 0u : (uint32_t)crc32(0, d.data(), (uInt)d.size()); }

Bytes raw_deflate(const Bytes &data, int level, int strategy, size_t flush_at = 0, int flush = Z_FULL_FLUSH)
{
    z_stream zs{};
    deflateInit2(&zs, level, Z_DEFLATED, -15, 8, strategy);
    Bytes out(deflateBound(&zs, (uLong)data.size()) + 64);
    zs.next_out = out.data(); zs.avail_out = (uInt)out.size();
    zs.next_in = (Bytef *)data.data();
    if (flush_at && flush_at < data.size()) { zs.avail_in = (uInt)flush_at; deflate(&zs, flush); }
    zs.avail_in = (uInt)(data.data() + data.size() - zs.next_in);
    deflate(&zs, Z_FINISH);
    out.resize(zs.total_out);
    deflateEnd(&zs);
    return out;
}

Bytes bgzf_member(const Bytes &raw, const Bytes &data, const Bytes &extra_before = {}, const char *fname = nullptr, bool fhcrc = false)
{
    Bytes m = {0x1f, 0x8b, 8, (uint8_t)(4 | (fname ? 8 : 0) | (fhcrc ? 2 : 0)), 0, 0, 0, 0, 0, 0xff};
    const size_t xlen = extra_before.size() + 6;
    m.push_back((uint8_t)xlen); m.push_back((uint8_t)(xlen >> 8));
    m.insert(m.end(), extra_before.begin(), extra_before.end());
    const size_t bc = m.size();
    m.insert(m.end(), {66, 67, 2, 0, 0, 0});
    if (fname) { m.insert(m.end(), fname, fname + strlen(fname)); m.push_back(0); }
    if (fhcrc) { const uint32_t h = (uint32_t)crc32(0, m.data(), (uInt)m.size()); m.push_back((uint8_t)h); m.push_back((uint8_t)(h >> 8)); }
    m.insert(m.end(), raw.begin(), raw.end());
    const uint32_t crc = crc_of(data), isize = (uint32_t)data.size();
    for (int i = 0; i < 4; ++i) m.push_back((uint8_t)(crc >> (8 * i)));
    for (int i = 0; i < 4; ++i) m.push_back((uint8_t)(isize >> (8 * i)));
    const size_t bsize = m.size() - 1;
    m[bc + 4] = (uint8_t)bsize; m[bc + 5] = (uint8_t)(bsize >> 8);
    return m;
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
        for (int k = 0; k < 150; ++k) { const uint32_t r = rnd() % 100; s += r < 70 ? 'F' : r < 91 ? 'F' : r < 97 ? ':' : r < 99 ? ',' : '#'; }
        s += "\n";
    }
    s.resize(n);
    return Bytes(s.begin(), s.end());
}

int n_case = 0, n_bad = 0;

// a valid member: the bytes come back, the status is OK
void valid(const char *name, const Bytes &raw, const Bytes &data)
{
    ++n_case;
    Bytes out(data.size() + 1);
    uint32_t info[5];
    const int st = inh_inflate(raw.data(), (uint32_t)raw.size(), out.data(), (uint32_t)data.size(), crc_of(data), info);
    if (st != SHIN_OK || info[1] != data.size() || (!data.empty() && memcmp(out.data(), data.data(), data.size()) != 0)) { std::printf("%s: status %d, %u of %zu bytes\n", name, st, info[1], data.size()); ++n_bad; }
}

// a corrupt member: the status asked for (or, want < 0, any status but OK)
void corrupt(const char *name, const Bytes &raw, uint32_t isize, uint32_t crc, int want)
{
    ++n_case;
    Bytes out(isize + 1);
    uint32_t info[5];
    const int st = inh_inflate(raw.data(), (uint32_t)raw.size(), out.data(), isize, crc, info);
    if (want >= 0 ? st != want : st == SHIN_OK) { std::printf("%s: status %d, wanted %d\n", name, st, want); ++n_bad; }
}

}      // namespace

int main()
{
    const Bytes text = fastq_like(65280, 1);
    const uint32_t text_crc = crc_of(text);
    const struct { const char *name; int level, strategy; } shapes[] = {{"stored", 0, Z_DEFAULT_STRATEGY}, {"fixed", 6, Z_FIXED}, {"huffman only", 6, Z_HUFFMAN_ONLY},
                                                                        {"rle", 6, Z_RLE}, {"level 1", 1, Z_DEFAULT_STRATEGY}, {"level 6", 6, Z_DEFAULT_STRATEGY}, {"level 9", 9, Z_DEFAULT_STRATEGY}};
    for (const auto &s : shapes) valid(s.name, raw_deflate(text, s.level, s.strategy), text);
    valid("full flush in mid-member", raw_deflate(text, 6, Z_DEFAULT_STRATEGY, 30000, Z_FULL_FLUSH), text);
    valid("sync flush in mid-member", raw_deflate(text, 6, Z_DEFAULT_STRATEGY, 1234, Z_SYNC_FLUSH), text);
    for (size_t n : {(size_t)0, (size_t)1, (size_t)65536}) { const Bytes d = fastq_like(n, 2); valid("0, 1 and 65536 bytes", raw_deflate(d, 6, Z_DEFAULT_STRATEGY), d); }
    { const Bytes d(60000, 'A'); valid("a run of one byte", raw_deflate(d, 9, Z_DEFAULT_STRATEGY), d); }
    {
        Bytes d(32768);
        uint32_t x = 7;
        for (auto &c : d) { x = x * 1664525u + 1013904223u; c = (uint8_t)(x >> 24); }
        d.insert(d.end(), d.begin(), d.begin() + 300);      // a match at distance 32768 that reaches back to the first byte
        valid("a far match", raw_deflate(d, 9, Z_DEFAULT_STRATEGY), d);
        std::vector<uint32_t> tok(d.begin(), d.begin() + 32768);      // zlib stops 262 short of the window: the token writer makes distance 32768
        tok.push_back(0x80000000u | (32768 - 1) << 8 | (258 - 3));
        Bytes z(tok.size() * 6 + 1024);
        uint64_t zl = 0;
        if (dfh_encode(tok.data(), tok.size(), z.data(), z.size(), &zl, nullptr, nullptr) != 0) { std::printf("distance 32768: encode\n"); ++n_bad; }
        z.resize(zl);
        d.resize(32768 + 258);
        valid("distance 32768 back to the first byte", z, d);
    }
    {      // the end-of-block symbol and 21 literals with counts F(1)..F(22): Huffman's tree is a comb, the limiter acts, the literal code has 15-bit codes
        std::vector<uint32_t> tok;
        uint32_t f0 = 1, f1 = 2;
        for (uint32_t s = 0; s < 21; ++s) { for (uint32_t k = 0; k < f0; ++k) tok.push_back(65 + s); const uint32_t f = f0 + f1; f0 = f1; f1 = f; }
        Bytes z(tok.size() * 6 + 1024), d;
        uint64_t zl = 0;
        uint8_t lit_lens[286];
        const int rc = dfh_encode(tok.data(), tok.size(), z.data(), z.size(), &zl, lit_lens, nullptr);
        z.resize(zl);
        uint32_t mx = 0;
        for (uint8_t l : lit_lens) if (l > mx) mx = l;
        for (uint32_t t : tok) d.push_back((uint8_t)t);
        if (rc != 0 || mx != 15) { std::printf("15-bit code: encode %d, longest code %u\n", rc, mx); ++n_bad; }
        valid("15-bit literal codes", z, d);
    }
    // the scan
    {
        ++n_case;
        const Bytes raw = raw_deflate(text, 6, Z_DEFAULT_STRATEGY);
        Bytes file = bgzf_member(raw, text, {'X', 'Y', 3, 0, 1, 2, 3}, "reads.fastq", true);
        const size_t first = file.size();
        const Bytes second = bgzf_member(raw, text), eof = bgzf_member(raw_deflate({}, 6, Z_DEFAULT_STRATEGY), {});
        file.insert(file.end(), second.begin(), second.end());
        file.insert(file.end(), eof.begin(), eof.end());
        ShinMember m[8];
        uint64_t nm = 0, used = 0;
        int st = inh_scan(file.data(), file.size(), m, 8, &nm, &used);
        bool ok = st == 0 && nm == 3 && used == file.size() && m[1].file_off == first && m[0].in_len == raw.size() && m[0].out_len == text.size() && m[0].crc32 == text_crc && m[2].out_len == 0 && eof.size() == 28;
        for (size_t cut : {first + 5, first + 40, file.size() - eof.size() - 3}) {
            std::unique_ptr<uint8_t[]> part(new uint8_t[cut]);
            memcpy(part.get(), file.data(), cut);
            st = inh_scan(part.get(), cut, m, 8, &nm, &used);
            ok = ok && st == 1 && nm == 1 && used == first;
        }
        file[first + 3] = 0;      // a gzip member without FEXTRA
        st = inh_scan(file.data(), file.size(), m, 8, &nm, &used);
        ok = ok && st == 2 && nm == 1 && used == first;
        if (!ok) { std::printf("scan\n"); ++n_bad; }
    }
    // corrupt members
    const Bytes good = raw_deflate(text, 6, Z_DEFAULT_STRATEGY);
    for (size_t bit = 0; bit < good.size() * 8; bit += 61) {      // any status, the right bytes if it is OK by chance, and no access outside the extents
        Bytes z = good;
        z[bit >> 3] ^= (uint8_t)(1u << (bit & 7));
        Bytes out(text.size() + 1);
        uint32_t info[5];
        const int st = inh_inflate(z.data(), (uint32_t)z.size(), out.data(), (uint32_t)text.size(), text_crc, info);
        if (st == SHIN_OK && memcmp(out.data(), text.data(), text.size()) != 0) { std::printf("bit %zu flipped: OK with other bytes\n", bit); ++n_bad; }
    }
    ++n_case;
    { Bytes z = good; z[z.size() / 2] ^= 0x10; corrupt("one bit flipped", z, (uint32_t)text.size(), text_crc, -1); }
    { Bytes z = raw_deflate(text, 0, Z_DEFAULT_STRATEGY); z[3] ^= 1; corrupt("NLEN mismatch", z, (uint32_t)text.size(), text_crc, SHIN_STORED_LEN); }
    corrupt("block type 3", {0x07, 0x00}, 0, 0, SHIN_BAD_BTYPE);
    corrupt("distance 1 as the first token", {0x03, 0x02, 0x00, 0x00}, 3, 0, SHIN_DIST_FAR);      // fixed block: length symbol 257 (0000001), distance symbol 0 (00000)
    { Bytes z = good; z.pop_back(); corrupt("input one byte short", z, (uint32_t)text.size(), text_crc, SHIN_IN_OVERRUN); }
    corrupt("ISIZE one too small", good, (uint32_t)text.size() - 1, text_crc, SHIN_OUT_OVERRUN);
    corrupt("ISIZE one too large", good, (uint32_t)text.size() + 1, text_crc, SHIN_OUT_SHORT);
    corrupt("CRC off by one", good, (uint32_t)text.size(), text_crc + 1, SHIN_CRC);
    corrupt("no input at all", {}, 0, 0, SHIN_IN_OVERRUN);
    // tables
    ++n_case;
    {
        uint8_t over[4] = {1, 1, 1, 0}, inc[4] = {2, 2, 2, 0}, one[30] = {0}, none[30] = {0}, lit_one[286] = {0};
        one[7] = 1; lit_one[256] = 1;
        if (inh_build(over, 4, 2) != SHIN_BAD_LENGTHS || inh_build(inc, 4, 2) != SHIN_BAD_LENGTHS || inh_build(inc, 4, 1) != SHIN_BAD_LENGTHS || inh_build(one, 30, 2) != SHIN_OK ||
            inh_build(one, 19, 0) != SHIN_BAD_LENGTHS || inh_build(none, 30, 2) != SHIN_OK || inh_build(lit_one, 286, 1) != SHIN_OK) { std::printf("tables\n"); ++n_bad; }
    }
    if (n_bad) return 1;
    std::printf("%d cases ok\n", n_case);
    return 0;
}
#endif
