// sh_dbg_align.hip — test aids: the two alignment kernels of the extension stage, called directly (tests/test_ksw_gpu.py).
//
// ksw_extd2_core (sh_align.h) and lr_ksw_ll_wave (sh_long.h) are otherwise reached through classify alone, where their inputs are what
// chaining hands over and their output shows as n_regs / n_aligned / dp_max.  Here a batch of hand-picked cases runs in one launch, one
// 64-lane block per case, through the product's own dispatch (ksw_extd2_wave for the short-read stage, lr_align_pair for the long-read
// one) and everything the kernels return comes back.  Nothing in the kernels under test knows about this file.
#include "sh_common.h"
#include "sh_long.h"

#define DBG_MAX_LEN 4096        // bases per sequence of a case
#define DBG_MAX_CASES 4096

__host__ __device__ inline int32_t dbg_n_col(int32_t qlen, int32_t tlen, int32_t w)
{
    const int32_t ww = w < 0 ? (tlen > qlen ? tlen : qlen) : w;
    int32_t nc = qlen < tlen ? qlen : tlen;
    return (((nc < ww + 1 ? nc : ww + 1) + 15) / 16 + 1) * 16;
}
__host__ __device__ inline unsigned long long dbg_p_need(int32_t qlen, int32_t tlen, int32_t w)
{
    return (unsigned long long)(qlen + tlen - 1) * (unsigned long long)dbg_n_col(qlen, tlen, w);
}
// the storage form ksw_extd2_wave (route 0) / lr_align_pair (route 1) dispatch to: their conditions, restated
__host__ __device__ inline int32_t dbg_form(int32_t route, int32_t qlen, int32_t tlen, int32_t w)
{
    const int32_t T16 = (tlen + 15) / 16 * 16, Q16 = (qlen + 15) / 16 * 16;
    const bool mem_lds = T16 <= AL_T16 && Q16 <= AL_Q16;
    if (route == 0 && mem_lds && dbg_p_need(qlen, tlen, w) <= AL_P) return 0;
    return mem_lds ? 1 : 2;
}
// the wave's working memory, as the long-read stage lays it out: room for cap_k x cap_k bases and cap_p direction bytes
__host__ __device__ inline LongSizes dbg_sizes(uint32_t cap_k, unsigned long long cap_p)
{
    LongSizes z{};
    z.cap_q = cap_k; z.cap_t = cap_k; z.cap_k = cap_k; z.cap_p = cap_p; z.phase = 1;
    return z;
}

__global__ void __launch_bounds__(64) k_dbg_ksw_extd2(const uint8_t *blob, const sh_dbg_ksw_case *cases, uint8_t *scratch, unsigned long long per_wave,
                                                      uint32_t cap_k, unsigned long long cap_p, const unsigned long long *cigar_off, sh_dbg_ksw_result *out, uint32_t *out_cigar)
{
    __shared__ AlignLds Ls;
    const sh_dbg_ksw_case c = cases[blockIdx.x];
    LongWs W;
    long_ws_carve(&W, scratch + (unsigned long long)blockIdx.x * per_wave, dbg_sizes(cap_k, cap_p));
    AlignScratch A{};
    A.kmem = W.kmem; A.kH = W.kH; A.koff = W.koff; A.kp = W.kp; A.ez_cigar = W.ez_cigar; A.tcap = W.cap_k; A.qcap = W.cap_k; A.pcap = W.cap_p;
    const uint8_t *query = blob + c.q_off, *target = blob + c.t_off;
    // the scores as both stages derive them from the options
    const int8_t sc_mch = (int8_t)(c.a < 0 ? -c.a : c.a), sc_mis = (int8_t)(c.b > 0 ? -c.b : c.b), sc_amb = (int8_t)(c.sc_ambi > 0 ? -c.sc_ambi : c.sc_ambi);
    const int8_t sc_N = sc_amb == 0 ? (int8_t)(-c.e2) : sc_amb;
    Ez ez;
    ez_reset(ez);
    int32_t form = dbg_form(c.route, c.qlen, c.tlen, c.w);
    if (c.route == 0) {
        ksw_extd2_wave(c.qlen, query, true, c.tlen, target, true, sc_mch, sc_mis, sc_N, c.q, c.e, c.q2, c.e2, c.w, c.zdrop, c.end_bonus, c.flag, ez, W.ez_cigar, A, Ls);
    } else {
        LongParams P{};
        P.q = c.q; P.e = c.e; P.q2 = c.q2; P.e2 = c.e2;
        LongCtx C;
        C.P = &P; C.AP = nullptr; C.I = nullptr; C.W = &W; C.Ls = &Ls; C.A = A; C.clk = nullptr;
        C.qlen = c.qlen; C.read = blockIdx.x;
        C.sc_mch = sc_mch; C.sc_mis = sc_mis; C.sc_amb = sc_amb; C.sc_N = sc_N;
        C.probe_why = 0; C.need_big = false; C.err = 0;
        if (!lr_align_pair(C, c.qlen, query, c.tlen, target, c.w, c.end_bonus, c.zdrop, c.flag, ez)) { ez_reset(ez); form = C.need_big ? -1 : -2; }
    }
    if (al_lane() == 0) {
        sh_dbg_ksw_result r;
        r.max = ez.max; r.zdropped = ez.zdropped; r.max_q = ez.max_q; r.max_t = ez.max_t; r.mqe = ez.mqe; r.mqe_t = ez.mqe_t; r.mte = ez.mte; r.mte_q = ez.mte_q;
        r.score = ez.score; r.reach_end = ez.reach_end; r.n_cigar = ez.n_cigar; r.form = form;
        r.cigar_off = cigar_off[blockIdx.x];
        out[blockIdx.x] = r;
        const int32_t room = c.qlen + c.tlen;      // a CIGAR has at most one word per base
        for (int32_t i = 0; i < ez.n_cigar && i < room; ++i) out_cigar[r.cigar_off + (uint64_t)i] = W.ez_cigar[i];      // lane 0 wrote them
    }
}

static bool dbg_seq_ok(const uint8_t *blob, uint64_t blob_len, uint64_t off, int32_t len)
{
    if (len < 1 || len > DBG_MAX_LEN || off > blob_len || (uint64_t)len > blob_len - off) return false;
    for (int32_t i = 0; i < len; ++i) if (blob[off + (uint64_t)i] > 4) return false;
    return true;
}

extern "C" sh_status sh_dbg_ksw_extd2(int32_t device, const uint8_t *blob, uint64_t blob_len, const sh_dbg_ksw_case *cases, int32_t n_cases,
                                      sh_dbg_ksw_result *out, uint32_t *out_cigar, uint64_t cigar_cap)
{
    SH_CHECK(blob && cases && out && out_cigar && n_cases > 0 && n_cases <= DBG_MAX_CASES, SH_ERR_BAD_ARG, "sh_dbg_ksw_extd2: bad argument");
    // the scratch of every wave holds the largest case of the batch that is not marked `unsized`
    uint32_t cap_k = 32; unsigned long long cap_p = 16, n_cigar_words = 0;
    std::vector<unsigned long long> cigar_off((size_t)n_cases);
    for (int32_t i = 0; i < n_cases; ++i) {
        const sh_dbg_ksw_case &c = cases[i];
        SH_CHECK(dbg_seq_ok(blob, blob_len, c.q_off, c.qlen) && dbg_seq_ok(blob, blob_len, c.t_off, c.tlen), SH_ERR_BAD_ARG, "sh_dbg_ksw_extd2: case %d: sequence outside the blob, longer than %d or not codes 0..4", i, DBG_MAX_LEN);
        SH_CHECK((c.route == 0 || c.route == 1) && c.a >= -127 && c.a <= 127 && c.b >= -127 && c.b <= 127 && c.sc_ambi >= -127 && c.sc_ambi <= 127 &&
                 c.q >= 0 && c.q <= 127 && c.e >= 0 && c.e <= 127 && c.q2 >= 0 && c.q2 <= 127 && c.e2 >= 0 && c.e2 <= 127, SH_ERR_BAD_ARG, "sh_dbg_ksw_extd2: case %d: route or scores out of range", i);
        cigar_off[(size_t)i] = n_cigar_words;
        n_cigar_words += (unsigned long long)(c.qlen + c.tlen);      // a CIGAR has at most one word per base
        if (c.unsized) continue;
        const uint32_t T16 = (uint32_t)(c.tlen + 15) / 16 * 16, Q16 = (uint32_t)(c.qlen + 15) / 16 * 16;
        if (T16 + 16 > cap_k) cap_k = T16 + 16;
        if (Q16 + 16 > cap_k) cap_k = Q16 + 16;
        const unsigned long long pn = dbg_p_need(c.qlen, c.tlen, c.w);
        if (pn > cap_p) cap_p = pn;
    }
    SH_CHECK(n_cigar_words <= cigar_cap, SH_ERR_BAD_ARG, "sh_dbg_ksw_extd2: the CIGAR buffer holds %llu words, the batch needs %llu", (unsigned long long)cigar_cap, n_cigar_words);
    // an unsized case must be one the code under test turns away (the tests of ksw_extd2_core and lr_align_pair, restated); all in LDS nothing tests the scratch
    auto turned_away = [&](const sh_dbg_ksw_case &c) {
        const uint32_t T16 = (uint32_t)(c.tlen + 15) / 16 * 16, Q16 = (uint32_t)(c.qlen + 15) / 16 * 16;
        const bool p_big = dbg_p_need(c.qlen, c.tlen, c.w) > cap_p;
        if (c.route == 1) return (uint32_t)c.tlen + 16 > cap_k || (uint32_t)c.qlen + 16 > cap_k || p_big;
        return dbg_form(0, c.qlen, c.tlen, c.w) != 0 && (T16 > cap_k || Q16 + 16 > cap_k + 32 || p_big || (uint32_t)(c.qlen + c.tlen) > 2 * cap_k);
    };
    for (int32_t i = 0; i < n_cases; ++i)
        SH_CHECK(!cases[i].unsized || turned_away(cases[i]), SH_ERR_BAD_ARG, "sh_dbg_ksw_extd2: case %d is marked unsized but fits the batch's scratch or runs in LDS alone", i);
    SH_HIP(hipSetDevice(device));
    const unsigned long long per_wave = long_ws_carve(nullptr, nullptr, dbg_sizes(cap_k, cap_p));
    uint8_t *d_blob = nullptr, *d_scratch = nullptr; sh_dbg_ksw_case *d_cases = nullptr; sh_dbg_ksw_result *d_out = nullptr; uint32_t *d_cigar = nullptr; unsigned long long *d_off = nullptr;
    auto run = [&]() -> sh_status {
        SH_HIP(hipMalloc(&d_blob, blob_len + 16)); SH_HIP(hipMalloc(&d_scratch, per_wave * (unsigned long long)n_cases));
        SH_HIP(hipMalloc(&d_cases, sizeof(sh_dbg_ksw_case) * (size_t)n_cases)); SH_HIP(hipMalloc(&d_out, sizeof(sh_dbg_ksw_result) * (size_t)n_cases));
        SH_HIP(hipMalloc(&d_cigar, 4 * (size_t)(n_cigar_words + 1))); SH_HIP(hipMalloc(&d_off, 8 * (size_t)n_cases));
        SH_HIP(hipMemset(d_blob, 0, blob_len + 16)); SH_HIP(hipMemset(d_cigar, 0, 4 * (size_t)(n_cigar_words + 1)));
        SH_HIP(hipMemcpy(d_blob, blob, blob_len, hipMemcpyHostToDevice));
        SH_HIP(hipMemcpy(d_cases, cases, sizeof(sh_dbg_ksw_case) * (size_t)n_cases, hipMemcpyHostToDevice));
        SH_HIP(hipMemcpy(d_off, cigar_off.data(), 8 * (size_t)n_cases, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_dbg_ksw_extd2, dim3((uint32_t)n_cases), dim3(64), 0, 0, d_blob, d_cases, d_scratch, per_wave, cap_k, cap_p, d_off, d_out, d_cigar);
        SH_HIP(hipGetLastError());
        SH_HIP(hipDeviceSynchronize());
        SH_HIP(hipMemcpy(out, d_out, sizeof(sh_dbg_ksw_result) * (size_t)n_cases, hipMemcpyDeviceToHost));
        if (n_cigar_words) SH_HIP(hipMemcpy(out_cigar, d_cigar, 4 * (size_t)n_cigar_words, hipMemcpyDeviceToHost));
        return SH_OK;
    };
    const sh_status st = run();
    hipFree(d_blob); hipFree(d_scratch); hipFree(d_cases); hipFree(d_out); hipFree(d_cigar); hipFree(d_off);
    return st;
}

// ---- the local alignment behind the inversion test ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) k_dbg_ksw_ll(const uint8_t *blob, const sh_dbg_ll_case *cases, uint8_t *scratch, unsigned long long per_wave, uint32_t cap_k,
                                                   sh_dbg_ll_result *out)
{
    const sh_dbg_ll_case c = cases[blockIdx.x];
    LongWs W;
    long_ws_carve(&W, scratch + (unsigned long long)blockIdx.x * per_wave, dbg_sizes(cap_k, 0));
    const int8_t sc_mch = (int8_t)(c.a < 0 ? -c.a : c.a), sc_mis = (int8_t)(c.b > 0 ? -c.b : c.b), sc_amb = (int8_t)(c.sc_ambi > 0 ? -c.sc_ambi : c.sc_ambi);
    int32_t qe, te;
    const int32_t score = lr_ksw_ll_wave(c.qlen, blob + c.q_off, c.tlen, blob + c.t_off, sc_mch, sc_mis, sc_amb, c.gapo, c.gape, qe, te, W.lH, W.lE, W.lHmax);
    if (al_lane() == 0) { sh_dbg_ll_result r; r.score = score; r.qe = qe; r.te = te; r.pad = 0; out[blockIdx.x] = r; }
}

extern "C" sh_status sh_dbg_ksw_ll(int32_t device, const uint8_t *blob, uint64_t blob_len, const sh_dbg_ll_case *cases, int32_t n_cases, sh_dbg_ll_result *out)
{
    SH_CHECK(blob && cases && out && n_cases > 0 && n_cases <= DBG_MAX_CASES, SH_ERR_BAD_ARG, "sh_dbg_ksw_ll: bad argument");
    uint32_t cap_k = 32;      // the callers of lr_ksw_ll_wave ask for qlen + 16 <= cap_k and tlen + 16 <= cap_k
    for (int32_t i = 0; i < n_cases; ++i) {
        const sh_dbg_ll_case &c = cases[i];
        SH_CHECK(dbg_seq_ok(blob, blob_len, c.q_off, c.qlen) && dbg_seq_ok(blob, blob_len, c.t_off, c.tlen), SH_ERR_BAD_ARG, "sh_dbg_ksw_ll: case %d: sequence outside the blob, longer than %d or not codes 0..4", i, DBG_MAX_LEN);
        SH_CHECK(c.a >= -127 && c.a <= 127 && c.b >= -127 && c.b <= 127 && c.sc_ambi >= -127 && c.sc_ambi <= 127 && c.gapo >= 0 && c.gapo <= 127 && c.gape >= 0 && c.gape <= 127,
                 SH_ERR_BAD_ARG, "sh_dbg_ksw_ll: case %d: scores out of range", i);
        if ((uint32_t)c.qlen + 16 > cap_k) cap_k = (uint32_t)c.qlen + 16;
        if ((uint32_t)c.tlen + 16 > cap_k) cap_k = (uint32_t)c.tlen + 16;
    }
    SH_HIP(hipSetDevice(device));
    const unsigned long long per_wave = long_ws_carve(nullptr, nullptr, dbg_sizes(cap_k, 0));
    uint8_t *d_blob = nullptr, *d_scratch = nullptr; sh_dbg_ll_case *d_cases = nullptr; sh_dbg_ll_result *d_out = nullptr;
    auto run = [&]() -> sh_status {
        SH_HIP(hipMalloc(&d_blob, blob_len + 16)); SH_HIP(hipMalloc(&d_scratch, per_wave * (unsigned long long)n_cases));
        SH_HIP(hipMalloc(&d_cases, sizeof(sh_dbg_ll_case) * (size_t)n_cases)); SH_HIP(hipMalloc(&d_out, sizeof(sh_dbg_ll_result) * (size_t)n_cases));
        SH_HIP(hipMemset(d_blob, 0, blob_len + 16));
        SH_HIP(hipMemcpy(d_blob, blob, blob_len, hipMemcpyHostToDevice));
        SH_HIP(hipMemcpy(d_cases, cases, sizeof(sh_dbg_ll_case) * (size_t)n_cases, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_dbg_ksw_ll, dim3((uint32_t)n_cases), dim3(64), 0, 0, d_blob, d_cases, d_scratch, per_wave, cap_k, d_out);
        SH_HIP(hipGetLastError());
        SH_HIP(hipDeviceSynchronize());
        SH_HIP(hipMemcpy(out, d_out, sizeof(sh_dbg_ll_result) * (size_t)n_cases, hipMemcpyDeviceToHost));
        return SH_OK;
    };
    const sh_status st = run();
    hipFree(d_blob); hipFree(d_scratch); hipFree(d_cases); hipFree(d_out);
    return st;
}
