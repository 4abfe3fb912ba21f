// bam_host.cpp — csrc/sh_bam.h on the host with a main of its own, for the sanitizers (test_bam_cpu.py builds it with
// -fsanitize=address,undefined and runs it as a program).  The input is a file of cases: n_ref (int32), the first record's offset
// (uint64), a flag (uint32: 1 = every prefix too), the length (uint64) and the bytes of a header and its records, valid or corrupt.
// Every window is parsed on a heap block of exactly its extent, and the names go to a block of exactly their bound, so a read or a
// write past either is the sanitizer's to report.  What the functions answer is the Python tests' business; here they only have to stay
// inside their blocks, end, and agree with themselves from prefix to prefix.
#include "../scrubby_amd/csrc/sh_bam.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static int fail(const char *what, size_t c, uint64_t at)
{
    printf("case %zu: %s at %llu\n", c, what, (unsigned long long)at);
    return 1;
}

// the window text[0, n) on its own heap block
struct Block {
    uint8_t *p;
    Block(const uint8_t *text, uint64_t n) : p((uint8_t *)malloc(n ? n : 1)) { if (n) memcpy(p, text, n); }
    ~Block() { free(p); }
};

static int walk(const uint8_t *text, uint64_t n, uint64_t entry, int32_t n_ref, uint64_t *pos, ShbCounts *c)
{
    const Block b(text, n);
    const uint64_t cap = shb_names_bound(n - entry);
    uint8_t *names = (uint8_t *)malloc(cap);
    const ShbRule rule{0, 0.0, 0, n_ref};
    uint64_t len = 0, last_seg = ~0ull;
    *c = ShbCounts{};
    const int how = shb_walk(ShbPtrSrc{b.p}, n, entry, n, rule, names, cap, &len, pos, c, &last_seg);
    free(names);
    return how == SHB_WALK_CAP ? -1 : how;
}

int main(int argc, char **argv)
{
    if (argc < 2) { printf("usage: %s cases.bin\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
    size_t n_cases = 0;
    for (;; ++n_cases) {
        int32_t n_ref; uint64_t first, n; uint32_t every;
        if (fread(&n_ref, 4, 1, f) != 1) break;
        if (fread(&first, 8, 1, f) != 1 || fread(&every, 4, 1, f) != 1 || fread(&n, 8, 1, f) != 1) return fail("short case header", n_cases, 0);
        std::vector<uint8_t> text(n);
        if (n && fread(text.data(), 1, n, f) != n) return fail("short case", n_cases, 0);
        // the header, from every prefix: MORE until it is whole, then the same answer
        for (uint64_t cut = 0; cut <= first + 8 && cut <= n; ++cut) {
            const Block b(text.data(), cut);
            int32_t refs = -1; uint64_t at = 0;
            const int st = shb_header(ShbPtrSrc{b.p}, cut, &refs, &at);
            if (cut < first ? st != SHB_HDR_MORE : (st != SHB_HDR_OK || refs != n_ref || at != first)) return fail("header", n_cases, cut);
        }
        // the whole window
        uint64_t end = 0; ShbCounts whole;
        const int how = walk(text.data(), n, first, n_ref, &end, &whole);
        if (how < 0 || how == SHB_WALK_OPEN) return fail("the whole window does not end at a record's end or at a broken one", n_cases, end);
        {
            const Block b(text.data(), n);
            uint64_t plausible = 0;
            for (uint64_t p = 0; p < n; ++p) plausible += shb_record_ok(ShbPtrSrc{b.p}, p, n, n_ref);
            if (plausible < whole.n_records) return fail("fewer plausible positions than records", n_cases, plausible);
        }
        if (!every) continue;
        // every prefix: the positions its end touches, and the walk - it ends at a record start of the whole walk, with no more records
        for (uint64_t cut = first; cut <= n; ++cut) {
            {
                const Block b(text.data(), cut);
                for (uint64_t p = cut > SHB_HALO + 8 ? cut - SHB_HALO - 8 : 0; p < cut; ++p) (void)shb_record_ok(ShbPtrSrc{b.p}, p, cut, n_ref);
                for (uint64_t p = cut > 8 ? cut - 8 : 0; p <= cut; ++p) (void)shb_complete(ShbPtrSrc{b.p}, p, cut);
            }
            uint64_t pos = 0; ShbCounts c;
            const int h = walk(text.data(), cut, first, n_ref, &pos, &c);
            if (h < 0 || pos > cut || c.n_records > whole.n_records) return fail("prefix", n_cases, cut);
            if (h == SHB_WALK_BROKEN && (how != SHB_WALK_BROKEN || pos != end)) return fail("a prefix is broken where the whole is not", n_cases, cut);
        }
    }
    fclose(f);
    printf("%zu cases ok\n", n_cases);
    return 0;
}
