// Host build of the DEFLATE encoder's pure parts (scrubby_amd/csrc/sh_deflate.h) for tests/test_deflate_cpu.py: length-limited code
// lengths, canonical codes, the dynamic header and the token writer, driven the way k_deflate_block drives them - histograms of a token
// list, both codes, the header, then every token's bits - into one final block.
// With -DDEFLATE_MAIN the file is a program of its own that runs every case and inflates the streams with zlib (the sanitizer build).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../scrubby_amd/csrc/sh_deflate.h"

namespace {

inline uint32_t tok_match(uint32_t len, uint32_t dist) { return SHD_TOK_MATCH | (dist - 1) << 8 | (len - 3); }

// sum of 2^(limit - len) over the used symbols: 2^limit for a complete code
uint64_t kraft(const uint8_t *lens, uint32_t n, uint32_t limit)
{
    uint64_t k = 0;
    for (uint32_t s = 0; s < n; ++s) if (lens[s]) k += 1ull << (limit - lens[s]);
    return k;
}

// prefix-free and canonical: codes of one length ascend with the symbol, and no code is a prefix of another (checked on the un-reversed codes)
bool codes_ok(const uint8_t *lens, const uint16_t *codes, uint32_t n)
{
    for (uint32_t a = 0; a < n; ++a)
        for (uint32_t b = 0; b < n; ++b) {
            if (a == b || !lens[a] || !lens[b] || lens[a] > lens[b]) continue;
            const uint32_t ca = shd_bit_reverse(codes[a], lens[a]), cb = shd_bit_reverse(codes[b], lens[b]);
            if ((cb >> (lens[b] - lens[a])) == ca) return false;
            if (lens[a] == lens[b] && a < b && ca >= cb) return false;
        }
    return true;
}

}      // namespace

extern "C" uint32_t dfh_lengths(const uint32_t *freq, uint32_t n, uint32_t limit, int complete, uint8_t *lens)
{
    ShdHuffWork w;
    return shd_code_lengths(freq, n, limit, complete != 0, lens, &w);
}

extern "C" uint64_t dfh_kraft(const uint8_t *lens, uint32_t n, uint32_t limit) { return kraft(lens, n, limit); }

extern "C" int dfh_codes_ok(const uint8_t *lens, uint32_t n)
{
    std::vector<uint16_t> codes(n);
    shd_canonical_codes(lens, n, codes.data());
    return codes_ok(lens, codes.data(), n) ? 1 : 0;
}

// the code-length symbols the header of (lit_lens, dist_lens) uses: cl_freq[19]
extern "C" void dfh_cl_freq(const uint8_t *lit_lens, const uint8_t *dist_lens, uint32_t *cl_freq)
{
    uint32_t hlit = SHD_N_LIT, hdist = SHD_N_DIST;
    while (hlit > 257 && lit_lens[hlit - 1] == 0) --hlit;
    while (hdist > 1 && dist_lens[hdist - 1] == 0) --hdist;
    for (uint32_t s = 0; s < SHD_N_CL; ++s) cl_freq[s] = 0;
    shd_rle_lengths(lit_lens, hlit, dist_lens, hdist, cl_freq, nullptr, nullptr, nullptr);
}

// One final dynamic block over a token list (without the end-of-block token: it is added here).  lit_lens / dist_lens (286 / 30, nullable)
// receive the code lengths.  0, or: 1 Kraft sum of the literal code, 2 of the distance code, 3 codes not prefix-free, 4 the header's bit
// count, 5 the body's bit count differs from the histogram's, 6 out of space.
extern "C" int dfh_encode(const uint32_t *tok, uint64_t n_tok, uint8_t *out, uint64_t cap, uint64_t *out_len, uint8_t *lit_lens_out, uint8_t *dist_lens_out)
{
    std::vector<uint32_t> t(tok, tok + n_tok);
    t.push_back(SHD_EOB);
    uint32_t lit_freq[SHD_N_LIT] = {0}, dist_freq[SHD_N_DIST] = {0};
    shd_count_tokens(t.data(), t.size(), lit_freq, dist_freq);
    ShdHuffWork w;
    uint8_t lit_lens[SHD_N_LIT], dist_lens[SHD_N_DIST];
    uint16_t lit_codes[SHD_N_LIT], dist_codes[SHD_N_DIST];
    shd_code_lengths(lit_freq, SHD_N_LIT, 15, true, lit_lens, &w);
    const uint32_t n_dist = shd_code_lengths(dist_freq, SHD_N_DIST, 15, false, dist_lens, &w);
    if (kraft(lit_lens, SHD_N_LIT, 15) != 1u << 15) return 1;
    if (n_dist >= 2 ? kraft(dist_lens, SHD_N_DIST, 15) != 1u << 15 : kraft(dist_lens, SHD_N_DIST, 15) != (n_dist ? 1u << 14 : 0u)) return 2;
    shd_canonical_codes(lit_lens, SHD_N_LIT, lit_codes);
    shd_canonical_codes(dist_lens, SHD_N_DIST, dist_codes);
    if (!codes_ok(lit_lens, lit_codes, SHD_N_LIT) || !codes_ok(dist_lens, dist_codes, SHD_N_DIST)) return 3;
    ShdBitWriter bw;
    shd_bw_init(&bw, out, (size_t)cap);
    const uint64_t hdr = shd_write_dynamic_header(&bw, true, lit_lens, dist_lens, &w);
    if (hdr != bw.n_bits || hdr > 8 * SHD_HDR_MAX_BYTES) return 4;
    shd_write_tokens(&bw, t.data(), t.size(), lit_codes, lit_lens, dist_codes, dist_lens);
    if (bw.n_bits - hdr != shd_body_bits(lit_freq, dist_freq, lit_lens, dist_lens)) return 5;
    shd_bw_flush(&bw);
    if (bw.overflow) return 6;
    *out_len = bw.pos;
    if (lit_lens_out) memcpy(lit_lens_out, lit_lens, SHD_N_LIT);
    if (dist_lens_out) memcpy(dist_lens_out, dist_lens, SHD_N_DIST);
    return 0;
}

extern "C" uint64_t dfh_bound(uint64_t n, uint32_t block_bytes) { return shd_bound(n, block_bytes); }

// length / distance -> (symbol, extra bits, extra value), for the tables of RFC 1951 3.2.5
extern "C" void dfh_len_sym(uint32_t len, uint32_t *out3) { out3[0] = shd_len_sym(len, &out3[1], &out3[2]); }
extern "C" void dfh_dist_sym(uint32_t dist, uint32_t *out3) { out3[0] = shd_dist_sym(dist, &out3[1], &out3[2]); }

#ifdef DEFLATE_MAIN
#include <zlib.h>

namespace {

bool inflate_raw(const std::vector<uint8_t> &z, std::vector<uint8_t> &out, size_t expect)
{
    z_stream zs{};
    if (inflateInit2(&zs, -15) != Z_OK) return false;
    out.assign(expect + 16, 0);
    zs.next_in = (Bytef *)z.data(); zs.avail_in = (uInt)z.size();
    zs.next_out = out.data(); zs.avail_out = (uInt)out.size();
    const int rc = inflate(&zs, Z_FINISH);
    const bool ok = rc == Z_STREAM_END && zs.avail_in == 0;
    out.resize(zs.total_out);
    inflateEnd(&zs);
    return ok;
}

// what a token list means
std::vector<uint8_t> expand(const std::vector<uint32_t> &tok)
{
    std::vector<uint8_t> o;
    for (uint32_t t : tok) {
        if (!(t & SHD_TOK_MATCH)) { o.push_back((uint8_t)t); continue; }
        const uint32_t len = (t & 0xff) + 3, dist = ((t >> 8) & 0x7fff) + 1;
        for (uint32_t i = 0; i < len; ++i) o.push_back(o[o.size() - dist]);
    }
    return o;
}

int round_trip(const char *name, const std::vector<uint32_t> &tok)
{
    std::vector<uint8_t> z(tok.size() * 6 + 1024), back;
    uint64_t zl = 0;
    const int rc = dfh_encode(tok.data(), tok.size(), z.data(), z.size(), &zl, nullptr, nullptr);
    if (rc) { std::printf("%s: encode code %d\n", name, rc); return 1; }
    z.resize(zl);
    const std::vector<uint8_t> want = expand(tok);
    if (!inflate_raw(z, back, want.size()) || back != want) { std::printf("%s: zlib does not return the bytes\n", name); return 1; }
    return 0;
}

int lengths_case(const char *name, const std::vector<uint32_t> &freq, uint32_t limit, bool complete, uint32_t want_used, uint64_t want_kraft)
{
    std::vector<uint8_t> lens(freq.size());
    const uint32_t used = dfh_lengths(freq.data(), (uint32_t)freq.size(), limit, complete, lens.data());
    uint32_t mx = 0;
    for (size_t s = 0; s < freq.size(); ++s) { if (lens[s] > mx) mx = lens[s]; if (freq[s] && !lens[s]) { std::printf("%s: a used symbol has no code\n", name); return 1; } }
    if (used != want_used || mx > limit || kraft(lens.data(), (uint32_t)freq.size(), limit) != want_kraft || !dfh_codes_ok(lens.data(), (uint32_t)freq.size())) {
        std::printf("%s: used %u max %u kraft %llu\n", name, used, mx, (unsigned long long)kraft(lens.data(), (uint32_t)freq.size(), limit));
        return 1;
    }
    return 0;
}

}      // namespace

int main()
{
    int bad = 0, n_case = 0;
    std::vector<uint32_t> fib(24);
    fib[0] = fib[1] = 1;
    for (int i = 2; i < 24; ++i) fib[i] = fib[i - 1] + fib[i - 2];
    bad += lengths_case("fibonacci, limit 15", fib, 15, true, 24, 1u << 15); ++n_case;
    std::vector<uint32_t> fib19(fib.begin(), fib.begin() + 19);
    bad += lengths_case("fibonacci, limit 7", fib19, 7, true, 19, 1u << 7); ++n_case;
    std::vector<uint32_t> one(SHD_N_LIT, 0), two(SHD_N_LIT, 0), all(SHD_N_LIT);
    one[65] = 9; two[65] = 9; two[256] = 1;
    for (uint32_t s = 0; s < SHD_N_LIT; ++s) all[s] = 1 + (s * 7919u) % 1000;
    bad += lengths_case("one symbol, completed", one, 15, true, 2, 1u << 15); ++n_case;
    bad += lengths_case("two symbols", two, 15, true, 2, 1u << 15); ++n_case;
    bad += lengths_case("all 286", all, 15, true, SHD_N_LIT, 1u << 15); ++n_case;
    std::vector<uint32_t> d0(SHD_N_DIST, 0), d1(SHD_N_DIST, 0);
    d1[29] = 5;
    bad += lengths_case("no distance code", d0, 15, false, 0, 0); ++n_case;
    bad += lengths_case("one distance code", d1, 15, false, 1, 1u << 14); ++n_case;

    std::vector<uint32_t> t;
    for (int i = 0; i < 300; ++i) t.push_back((uint32_t)((i * 37) % 251));
    bad += round_trip("literals only", t); ++n_case;
    t = {'a', tok_match(3, 1)};
    bad += round_trip("length 3 at distance 1", t); ++n_case;
    t.clear();
    for (uint32_t i = 0; i < 32768; ++i) t.push_back((i * 2654435761u) >> 24);
    t.push_back(tok_match(258, 32768));
    bad += round_trip("length 258 at distance 32768", t); ++n_case;
    t = {0, 255, 0, 255, 255, 0};      // lengths 1..254 of the literal code are a run of 254 zeros: code 18 twice
    bad += round_trip("a run of zero code lengths", t); ++n_case;
    t = {1, 2};
    for (uint32_t len = 3; len <= 258; ++len) { t.push_back(len & 0xff); t.push_back(tok_match(len, 1 + (len * 127) % 2)); }      // every length symbol
    for (uint32_t d = 1, n = 0; d <= 32768 && n < 40000; d = d + 1 + d / 3) { while (n < d) { t.push_back((n * 31) & 0xff); ++n; } t.push_back(tok_match(3, d)); n += 3; }
    bad += round_trip("every length, many distances", t); ++n_case;
    if (bad) return 1;
    std::printf("%d cases ok\n", n_case);
    return 0;
}
#endif
