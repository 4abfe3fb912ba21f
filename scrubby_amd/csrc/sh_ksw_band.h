// The band of ksw_extd2 in closed form (sh_align.h: ksw_extd2_core's fill loops and ksw_backtrack_dev), free of HIP so that a host compiler
// can include it (tests/ksw_band_host.cpp).  Anti-diagonal r = i + j of a qlen x tlen matrix with band width w holds the target cells
// [st0, en0]; the kernels compute the range rounded to whole groups of 16: st down to a multiple of 16, en up to one less than a multiple
// of 16.  The direction bytes of diagonal r start at column st, so the backtrack needs (st, en) of every diagonal it crosses: it takes them
// from here instead of from two arrays the fill used to write.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define KB_FN __host__ __device__ inline
#else
#define KB_FN inline
#endif

struct KswBand { int32_t st0, en0, st, en; };      // st0 > en0: the band has left the matrix (the fill stops there, z-dropped)

// w < 0 means no band: max(qlen, tlen), as ksw_extd2 resolves it
KB_FN int32_t ksw_band_width(int32_t qlen, int32_t tlen, int32_t w) { return w < 0 ? (tlen > qlen ? tlen : qlen) : w; }

// w: resolved (ksw_band_width)
KB_FN KswBand ksw_band(int32_t r, int32_t qlen, int32_t tlen, int32_t w)
{
    KswBand b;
    int32_t st = 0, en = tlen - 1;
    if (st < r - qlen + 1) st = r - qlen + 1;
    if (en > r) en = r;
    if (st < (r - w + 1) >> 1) st = (r - w + 1) >> 1;
    if (en > (r + w) >> 1) en = (r + w) >> 1;
    b.st0 = st; b.en0 = en;
    b.st = st / 16 * 16; b.en = (en + 16) / 16 * 16 - 1;
    return b;
}
