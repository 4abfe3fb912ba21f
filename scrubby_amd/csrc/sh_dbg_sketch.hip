// sh_dbg_sketch.hip — test aid: the three minimizer state machines of sh_sketch.h, called directly (tests/test_sketch_gpu.py).
//
// SketchState, SketchPacked and SketchStateDyn are reached through classify alone, where their output shows as n_mini and as whatever the
// later stages make of the seeds.  Here one lane sketches one sequence of a batch, one launch per form, and every push comes back in
// emission order as (hash, y = pos << 1 | strand).  Each form is driven as its contract in sh_sketch.h says and as its caller in
// sh_classify.hip does; bases are decoded with sh_nt4.  Nothing in the code under test knows about this file.
#include "sh_common.h"
#include "sh_sketch.h"

#define DBGS_MAX_SEQ (1 << 20)
enum { SK_STATE = 0, SK_PACKED = 1, SK_DYN = 2, SK_N };

struct DbgSketchArgs {
    const uint8_t *bases; const uint64_t *offsets; uint32_t n_seq; int32_t w, k;
    uint64_t *hash; uint32_t *y; int32_t *count;
    uint64_t *ring_x; uint32_t *ring_y;      // SK_DYN: w entries per lane
};

// the pushes of sequence s go to [offsets[s] - offsets[0] + s, + len + 1); a push beyond that is counted and not written
struct DbgSketchOut {
    uint64_t *hash; uint32_t *y; uint32_t cap, n;
    __device__ inline void put(uint64_t h, uint32_t yy) { if (n < cap) { hash[n] = h; y[n] = yy; } ++n; }
};

template <int W, int FORM>
__global__ __launch_bounds__(64) void k_dbg_sketch(DbgSketchArgs a)
{
    const uint32_t s = blockIdx.x * 64 + threadIdx.x;
    if (s >= a.n_seq) return;
    const uint64_t o_beg = a.offsets[s];
    const uint32_t len = (uint32_t)(a.offsets[s + 1] - o_beg);
    const uint8_t *seq = a.bases + o_beg;
    const uint64_t at = o_beg - a.offsets[0] + s;
    DbgSketchOut out{a.hash + at, a.y + at, len + 1, 0};
    if constexpr (FORM == SK_STATE) {
        SketchState<W> st;
        st.init(a.k);
        auto emit = [&](uint64_t x, uint32_t y) { out.put(x >> 8, y); };
        for (uint32_t i0 = 0; i0 < len; i0 += W) {
            auto one = [&](auto Pc) {
                constexpr int P = decltype(Pc)::value;
                const uint32_t i = i0 + P;
                if (i < len) st.template step<P>(sh_nt4(seq[i]), i, emit);
            };
            [&]<int... Ps>(std::integer_sequence<int, Ps...>) { (one(std::integral_constant<int, Ps>{}), ...); }
            (std::make_integer_sequence<int, W>{});
        }
        st.finish(emit);
    } else if constexpr (FORM == SK_PACKED) {
        SketchPacked<W> st;
        st.init(a.k);
        auto emit = [&](uint64_t packed) { const uint64_t e = sh_packed_entry(packed); out.put(e >> 18, (uint32_t)e & 0x3ffffu); };
        for (uint32_t i0 = 0; i0 < len; i0 += W) {
            auto one = [&](auto Pc) {
                constexpr int P = decltype(Pc)::value;
                const uint32_t i = i0 + P;
                if (i < len) st.template step<P>(sh_nt4(seq[i]), i, emit, emit);
            };
            [&]<int... Ps>(std::integer_sequence<int, Ps...>) { (one(std::integral_constant<int, Ps>{}), ...); }
            (std::make_integer_sequence<int, W>{});
            st.block_end();
        }
        st.finish(emit);
    } else {
        SketchStateDyn st;
        st.init(a.ring_x + (size_t)s * W, a.ring_y + (size_t)s * W, a.w, a.k);
        auto emit = [&](uint64_t x, uint32_t y) { out.put(x >> 8, y); };
        for (uint32_t i = 0; i < len; ++i) st.step(sh_nt4(seq[i]), i, emit);
        st.finish(emit);
    }
    a.count[s] = (int32_t)out.n;
}

template <int W>
static void launch_dbg_sketch(const DbgSketchArgs &a, int form)
{
    const dim3 grid((a.n_seq + 63) / 64), block(64);
    if (form == SK_STATE) hipLaunchKernelGGL((k_dbg_sketch<W, SK_STATE>), grid, block, 0, 0, a);
    else if (form == SK_PACKED) hipLaunchKernelGGL((k_dbg_sketch<W, SK_PACKED>), grid, block, 0, 0, a);
    else hipLaunchKernelGGL((k_dbg_sketch<W, SK_DYN>), grid, block, 0, 0, a);
}

extern "C" sh_status sh_dbg_sketch(int32_t device, const uint8_t *bases, const uint64_t *offsets, int32_t n_seq, int32_t w, int32_t k, int32_t form,
                                   uint64_t *hash, uint32_t *y, int32_t *count)
{
    SH_CHECK(offsets && hash && y && count && n_seq > 0 && n_seq <= DBGS_MAX_SEQ, SH_ERR_BAD_ARG, "sh_dbg_sketch: bad argument");
    SH_CHECK(form >= 0 && form < SK_N, SH_ERR_BAD_ARG, "sh_dbg_sketch: unknown form %d", form);
    SH_CHECK(w == 5 || w == 10 || w == 11 || w == 19, SH_ERR_BAD_ARG, "sh_dbg_sketch: w = %d is not an instantiated window (5, 10, 11, 19)", w);
    SH_CHECK(k >= 1 && (k & 1) && k <= (form == SK_PACKED ? 23 : 27), SH_ERR_BAD_ARG, "sh_dbg_sketch: form %d takes odd k <= %d, not %d", form, form == SK_PACKED ? 23 : 27, k);
    for (int32_t i = 0; i < n_seq; ++i) {
        SH_CHECK(offsets[i] <= offsets[i + 1], SH_ERR_BAD_ARG, "sh_dbg_sketch: offsets decrease at sequence %d", i);
        SH_CHECK(form != SK_PACKED || offsets[i + 1] - offsets[i] <= 1024, SH_ERR_BAD_ARG, "sh_dbg_sketch: the packed form takes sequences of at most 1024 bases (sequence %d)", i);
    }
    const uint64_t o0 = offsets[0], n_bases = offsets[n_seq] - o0;
    SH_CHECK(n_bases < (1ULL << 30) && (bases || n_bases == 0), SH_ERR_BAD_ARG, "sh_dbg_sketch: bases missing or beyond 2^30");
    const size_t n_out = (size_t)n_bases + (size_t)n_seq;
    SH_HIP(hipSetDevice(device));
    uint8_t *d_bases = nullptr; uint64_t *d_off = nullptr, *d_hash = nullptr, *d_rx = nullptr; uint32_t *d_y = nullptr, *d_ry = nullptr; int32_t *d_cnt = nullptr;
    auto run = [&]() -> sh_status {
        std::vector<uint64_t> rel((size_t)n_seq + 1);
        for (int32_t i = 0; i <= n_seq; ++i) rel[(size_t)i] = offsets[i] - o0;
        SH_HIP(hipMalloc(&d_bases, (size_t)n_bases + 16)); SH_HIP(hipMalloc(&d_off, 8 * ((size_t)n_seq + 1)));
        SH_HIP(hipMalloc(&d_hash, 8 * n_out)); SH_HIP(hipMalloc(&d_y, 4 * n_out)); SH_HIP(hipMalloc(&d_cnt, 4 * (size_t)n_seq));
        if (n_bases) SH_HIP(hipMemcpy(d_bases, bases + o0, (size_t)n_bases, hipMemcpyHostToDevice));
        SH_HIP(hipMemcpy(d_off, rel.data(), 8 * ((size_t)n_seq + 1), hipMemcpyHostToDevice));
        SH_HIP(hipMemset(d_hash, 0xff, 8 * n_out)); SH_HIP(hipMemset(d_y, 0xff, 4 * n_out)); SH_HIP(hipMemset(d_cnt, 0xff, 4 * (size_t)n_seq));
        DbgSketchArgs a{d_bases, d_off, (uint32_t)n_seq, w, k, d_hash, d_y, d_cnt, nullptr, nullptr};
        if (form == SK_DYN) {
            SH_HIP(hipMalloc(&d_rx, 8 * (size_t)n_seq * (size_t)w)); SH_HIP(hipMalloc(&d_ry, 4 * (size_t)n_seq * (size_t)w));
            a.ring_x = d_rx; a.ring_y = d_ry;
        }
        switch (w) {
        case 5: launch_dbg_sketch<5>(a, form); break;
        case 10: launch_dbg_sketch<10>(a, form); break;
        case 11: launch_dbg_sketch<11>(a, form); break;
        default: launch_dbg_sketch<19>(a, form); break;
        }
        SH_HIP(hipGetLastError());
        SH_HIP(hipDeviceSynchronize());
        SH_HIP(hipMemcpy(hash, d_hash, 8 * n_out, hipMemcpyDeviceToHost)); SH_HIP(hipMemcpy(y, d_y, 4 * n_out, hipMemcpyDeviceToHost));
        SH_HIP(hipMemcpy(count, d_cnt, 4 * (size_t)n_seq, hipMemcpyDeviceToHost));
        return SH_OK;
    };
    const sh_status st = run();
    hipFree(d_bases); hipFree(d_off); hipFree(d_hash); hipFree(d_y); hipFree(d_cnt); hipFree(d_rx); hipFree(d_ry);
    return st;
}
