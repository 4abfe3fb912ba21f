// The closed-form band of ksw_extd2 (scrubby_amd/csrc/sh_ksw_band.h) for tests/test_ksw_band_cpu.py: every anti-diagonal of one shape, as the
// kernels' fill loops walk them (up to the first diagonal on which the band has left the matrix).
#include "../scrubby_amd/csrc/sh_ksw_band.h"

// out: 4 int32 per diagonal (st0, en0, st, en), room for qlen + tlen - 1 of them; returns how many were written
extern "C" int32_t kbh_ranges(int32_t qlen, int32_t tlen, int32_t w, int32_t *out)
{
    const int32_t ww = ksw_band_width(qlen, tlen, w);
    int32_t n = 0;
    for (int32_t r = 0; r < qlen + tlen - 1; ++r) {
        const KswBand b = ksw_band(r, qlen, tlen, ww);
        if (b.st0 > b.en0) break;
        out[4 * n] = b.st0; out[4 * n + 1] = b.en0; out[4 * n + 2] = b.st; out[4 * n + 3] = b.en;
        ++n;
    }
    return n;
}
