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

// ---- the region bookkeeping of the short-read stage: align_read_wave over caller-made chains (tests/test_regs_gpu.py) ------------------------
static_assert(sizeof(sh_dbg_chain_rec) == sizeof(ChainRec) && sizeof(sh_dbg_align_params) == sizeof(AlignParams), "the test aid's structures are the kernels' own");
#define DBG_GUARD 4096u         // bytes of DBG_GUARD_BYTE on either side of a wave's scratch
#define DBG_GUARD_BYTE 0xA5

struct DbgRegsArgs {
    AlignIn in; AlignParams P;
    const uint32_t *list; const int32_t *mode; const unsigned long long *top_z;
    uint8_t *scratch; unsigned long long per_wave;      // per_wave: guard + layout + guard
    uint32_t max_read_len, reg_cap, row_cap;
    sh_dbg_regs_out *out; uint32_t *book; int32_t *keep;
};

template <class LDS>
__global__ void __launch_bounds__(64) k_dbg_regs_short(DbgRegsArgs a)
{
    __shared__ LDS Ls;
    __shared__ uint32_t s_ovf;
    const uint32_t r = a.list[blockIdx.x];
    if (threadIdx.x == 0) s_ovf = 0;
    __syncthreads();
    AlignScratch A;
    align_scratch_carve(A, a.scratch + (unsigned long long)r * a.per_wave + DBG_GUARD, a.max_read_len, a.reg_cap);
    AlignRowsHook hk{a.book + (size_t)r * a.row_cap * 2, a.keep + (size_t)r * a.row_cap * 8, a.row_cap, a.row_cap, 0u, 0u};
    AlignOut o;
    const int32_t mode = a.mode[r];
    const bool done = align_read_wave<LDS, false, AlignRowsHook>(a.in, a.P, r, mode != 0, A, Ls, o, &s_ovf, mode == 2 ? a.top_z[r] : 0ull, &hk);
    __syncthreads();
    if (threadIdx.x == 0) {
        sh_dbg_regs_out w{};
        w.n_aligned = o.n_aligned; w.n_regs = o.n_regs; w.dp_max = o.dp_max; w.sig = o.sig; w.overflow = s_ovf; w.done = done ? 1 : 0;
        w.n_book = hk.n_book; w.n_keep = hk.n_keep;
        a.out[r] = w;
    }
}

// how many bytes of the two guard bands of wave r's scratch no longer hold DBG_GUARD_BYTE (after k_dbg_regs_short, on the same stream)
__global__ void __launch_bounds__(64) k_dbg_regs_guard(const uint8_t *scratch, unsigned long long per_wave, sh_dbg_regs_out *out)
{
    const uint8_t *lo = scratch + (unsigned long long)blockIdx.x * per_wave, *hi = lo + per_wave - DBG_GUARD;
    uint32_t bad = 0;
    for (uint32_t i = threadIdx.x; i < DBG_GUARD; i += 64) bad += (lo[i] != DBG_GUARD_BYTE) + (hi[i] != DBG_GUARD_BYTE);
    if (bad) atomicAdd(&out[blockIdx.x].guard, bad);
}

extern "C" sh_status sh_dbg_regs_short(int32_t device, const uint8_t *ref_packed, const uint64_t *cstart, uint32_t n_contigs, const uint8_t *bases,
                                       const uint64_t *offsets, uint32_t n_reads, const uint64_t *cx, const uint32_t *cq, uint64_t n_anchors,
                                       const sh_dbg_chain_rec *recs, uint32_t n_recs, const uint32_t *head, const sh_dbg_align_params *params,
                                       uint32_t reg_cap, uint32_t max_read_len, const int32_t *mode, uint32_t row_cap,
                                       sh_dbg_regs_out *out, uint32_t *book, int32_t *keep)
{
    SH_CHECK(ref_packed && cstart && bases && offsets && cx && cq && recs && head && params && mode && out && book && keep, SH_ERR_BAD_ARG, "sh_dbg_regs_short: null argument");
    SH_CHECK(n_contigs >= 1 && n_contigs < (1u << 30) && n_reads >= 1 && n_reads <= DBG_MAX_CASES && n_recs >= 1 && n_anchors >= 1 && row_cap >= 1, SH_ERR_BAD_ARG, "sh_dbg_regs_short: bad count");
    const sh_dbg_align_params &P = *params;
    SH_CHECK(P.k >= 1 && P.k <= 255 && P.e >= 1 && reg_cap >= 1 && reg_cap <= (1u << 20) && max_read_len >= 1 && max_read_len <= (1u << 20), SH_ERR_BAD_ARG,
             "sh_dbg_regs_short: k < 1, e < 1, reg_cap or max_read_len out of range");
    for (uint32_t c = 0; c < n_contigs; ++c) SH_CHECK(cstart[c + 1] > cstart[c] && cstart[c + 1] - cstart[c] < (1ull << 31), SH_ERR_BAD_ARG, "sh_dbg_regs_short: contig %u is empty or too long", c);
    std::vector<unsigned long long> top_z((size_t)n_reads, 0ull);
    std::vector<uint32_t> list_all, list_top;
    for (uint32_t r = 0; r < n_reads; ++r) {
        SH_CHECK(offsets[r + 1] > offsets[r] && offsets[r + 1] - offsets[r] < (1ull << 24), SH_ERR_BAD_ARG, "sh_dbg_regs_short: read %u is empty or too long", r);
        SH_CHECK(mode[r] >= 0 && mode[r] <= 2, SH_ERR_BAD_ARG, "sh_dbg_regs_short: read %u: mode %d", r, mode[r]);
        const int64_t qlen = (int64_t)(offsets[r + 1] - offsets[r]);
        uint32_t steps = 0;
        for (uint32_t h = head[r]; h != ~0u; h = recs[h].next, ++steps) {
            SH_CHECK(h < n_recs && steps < n_recs, SH_ERR_BAD_ARG, "sh_dbg_regs_short: read %u: the chain list leaves the table or does not end in ~0u", r);
            const sh_dbg_chain_rec &rc = recs[h];
            SH_CHECK(rc.cnt >= 1 && rc.off < n_anchors && rc.cnt <= n_anchors - rc.off && rc.score >= 0, SH_ERR_BAD_ARG, "sh_dbg_regs_short: record %u: no anchors, anchors outside the arrays or a negative score", h);
            const uint64_t hi = cx[rc.off] >> 32;
            const uint32_t rid = (uint32_t)(hi & 0x7fffffffu);
            SH_CHECK(rid < n_contigs, SH_ERR_BAD_ARG, "sh_dbg_regs_short: record %u: contig %u", h, rid);
            const int64_t clen = (int64_t)(cstart[rid + 1] - cstart[rid]);
            for (uint32_t j = 0; j < rc.cnt; ++j) {
                const uint64_t x = cx[rc.off + j]; const int64_t rp = (int64_t)(uint32_t)x, qp = (int64_t)cq[rc.off + j];
                SH_CHECK(x >> 32 == hi, SH_ERR_BAD_ARG, "sh_dbg_regs_short: record %u: anchor %u on another contig or strand", h, j);
                SH_CHECK(rp + 1 >= P.k && rp < clen && qp + 1 >= P.k && qp < qlen, SH_ERR_BAD_ARG, "sh_dbg_regs_short: record %u: anchor %u outside its contig or the read", h, j);
                SH_CHECK(j == 0 || ((uint32_t)cx[rc.off + j - 1] < (uint32_t)x && cq[rc.off + j - 1] < cq[rc.off + j]), SH_ERR_BAD_ARG, "sh_dbg_regs_short: record %u: anchors not ascending in x and q at %u", h, j);
            }
            const unsigned long long z = chain_z(cx[rc.off], cq[rc.off], P.k, rc.score, rc.cnt, region_hash((int32_t)qlen), (uint64_t)rc.yfl << 32);
            SH_CHECK(rc.z == z, SH_ERR_BAD_ARG, "sh_dbg_regs_short: record %u: z is not the key of its chain", h);
            if (z > top_z[r]) top_z[r] = z;
        }
        (mode[r] == 2 ? list_top : list_all).push_back(r);
    }
    SH_HIP(hipSetDevice(device));
    const unsigned long long per_wave = align_scratch_layout(max_read_len, reg_cap, nullptr, nullptr, nullptr) + 2ull * DBG_GUARD;
    const uint64_t ref_bytes = (cstart[n_contigs] + 1) / 2, n_bases = offsets[n_reads];
    std::vector<void *> dev;
    auto up = [&](void **d, const void *h, size_t bytes) -> sh_status {
        SH_HIP(hipMalloc(d, bytes + 16)); dev.push_back(*d);
        SH_HIP(hipMemset(*d, 0, bytes + 16));
        if (h && bytes) SH_HIP(hipMemcpy(*d, h, bytes, hipMemcpyHostToDevice));
        return SH_OK;
    };
    auto run = [&]() -> sh_status {
        DbgRegsArgs a{};
        void *d_ref, *d_cs, *d_bases, *d_off, *d_cx, *d_cq, *d_recs, *d_head, *d_mode, *d_top, *d_list, *d_out, *d_book, *d_keep, *d_scratch;
        sh_status st;
        if ((st = up(&d_ref, ref_packed, ref_bytes)) != SH_OK || (st = up(&d_cs, cstart, 8 * ((size_t)n_contigs + 1))) != SH_OK || (st = up(&d_bases, bases, n_bases)) != SH_OK ||
            (st = up(&d_off, offsets, 8 * ((size_t)n_reads + 1))) != SH_OK || (st = up(&d_cx, cx, 8 * n_anchors)) != SH_OK || (st = up(&d_cq, cq, 4 * n_anchors)) != SH_OK ||
            (st = up(&d_recs, recs, sizeof(ChainRec) * (size_t)n_recs)) != SH_OK || (st = up(&d_head, head, 4 * (size_t)n_reads)) != SH_OK ||
            (st = up(&d_mode, mode, 4 * (size_t)n_reads)) != SH_OK || (st = up(&d_top, top_z.data(), 8 * (size_t)n_reads)) != SH_OK ||
            (st = up(&d_list, nullptr, 4 * (size_t)n_reads)) != SH_OK || (st = up(&d_out, nullptr, sizeof(sh_dbg_regs_out) * (size_t)n_reads)) != SH_OK ||
            (st = up(&d_book, nullptr, 8 * (size_t)n_reads * row_cap)) != SH_OK || (st = up(&d_keep, nullptr, 32 * (size_t)n_reads * row_cap)) != SH_OK) return st;
        SH_HIP(hipMalloc(&d_scratch, per_wave * n_reads)); dev.push_back(d_scratch);
        SH_HIP(hipMemset(d_scratch, DBG_GUARD_BYTE, per_wave * n_reads));
        a.in.ref = (const uint8_t *)d_ref; a.in.cstart = (const uint64_t *)d_cs; a.in.n_contigs = n_contigs; a.in.bases = (const uint8_t *)d_bases; a.in.offsets = (const uint64_t *)d_off;
        a.in.cx = (const uint64_t *)d_cx; a.in.cq = (const uint32_t *)d_cq; a.in.recs = (const ChainRec *)d_recs; a.in.head = (const uint32_t *)d_head;
        memcpy(&a.P, params, sizeof(AlignParams));
        a.mode = (const int32_t *)d_mode; a.top_z = (const unsigned long long *)d_top; a.scratch = (uint8_t *)d_scratch; a.per_wave = per_wave;
        a.max_read_len = max_read_len; a.reg_cap = reg_cap; a.row_cap = row_cap;
        a.out = (sh_dbg_regs_out *)d_out; a.book = (uint32_t *)d_book; a.keep = (int32_t *)d_keep;
        if (!list_all.empty()) SH_HIP(hipMemcpy(d_list, list_all.data(), 4 * list_all.size(), hipMemcpyHostToDevice));
        if (!list_top.empty()) SH_HIP(hipMemcpy((uint32_t *)d_list + list_all.size(), list_top.data(), 4 * list_top.size(), hipMemcpyHostToDevice));
        if (!list_all.empty()) { a.list = (const uint32_t *)d_list; hipLaunchKernelGGL(k_dbg_regs_short<AlignLds>, dim3((uint32_t)list_all.size()), dim3(64), 0, 0, a); SH_HIP(hipGetLastError()); }
        if (!list_top.empty()) { a.list = (const uint32_t *)d_list + list_all.size(); hipLaunchKernelGGL(k_dbg_regs_short<AlignLdsTop>, dim3((uint32_t)list_top.size()), dim3(64), 0, 0, a); SH_HIP(hipGetLastError()); }
        hipLaunchKernelGGL(k_dbg_regs_guard, dim3(n_reads), dim3(64), 0, 0, (const uint8_t *)d_scratch, per_wave, (sh_dbg_regs_out *)d_out);
        SH_HIP(hipGetLastError());
        SH_HIP(hipDeviceSynchronize());
        SH_HIP(hipMemcpy(out, d_out, sizeof(sh_dbg_regs_out) * (size_t)n_reads, hipMemcpyDeviceToHost));
        SH_HIP(hipMemcpy(book, d_book, 8 * (size_t)n_reads * row_cap, hipMemcpyDeviceToHost));
        SH_HIP(hipMemcpy(keep, d_keep, 32 * (size_t)n_reads * row_cap, hipMemcpyDeviceToHost));
        return SH_OK;
    };
    const sh_status st = run();
    for (void *d : dev) hipFree(d);
    return st;
}

// ---- the same bookkeeping of the long-read stage: lr_set_parent0 + lr_select_sub0 over caller-made regions -----------------------------------
#define DBG_MAX_LREGS 4096
__global__ void __launch_bounds__(64) k_dbg_regs_long(const int32_t *tab, const sh_dbg_lreg_case *cases, LReg *regs, uint64_t *cov, int32_t *wpri, int32_t *tmp, int32_t *n_kept, int32_t *rows)
{
    if (threadIdx.x != 0) return;      // lane 0, as in the product
    const sh_dbg_lreg_case c = cases[blockIdx.x];
    LReg *R = regs + c.off;
    for (int32_t i = 0; i < c.n; ++i) {
        const int32_t *t = tab + (c.off + (uint64_t)i) * 9;
        LReg r{};
        r.id = i; r.parent = LR_PARENT_UNSET; r.div = -1.0f;
        r.score = t[0]; r.cnt = t[1]; r.qs = t[2]; r.qe = t[3]; r.rs = t[4]; r.re = t[5]; r.rev = t[6]; r.rid = t[7]; r.inv = t[8];
        r.as = i;      // no anchors here: the field carries the row's place in the table through the compaction
        R[i] = r;
    }
    lr_set_parent0(c.mask_level, c.n, R, cov + c.off, wpri + c.off);
    const int32_t k = lr_select_sub0(c.pri_ratio, c.min_diff, c.best_n, c.min_strand_sc, c.n, R, tmp + c.off);
    n_kept[blockIdx.x] = k;
    for (int32_t i = 0; i < k; ++i) {
        int32_t *o = rows + (c.off + (uint64_t)i) * 6;
        o[0] = R[i].as; o[1] = R[i].id; o[2] = R[i].parent; o[3] = R[i].subsc; o[4] = R[i].n_sub; o[5] = R[i].strand_retained;
    }
}

extern "C" sh_status sh_dbg_regs_long(int32_t device, const int32_t *tab, uint64_t n_rows, const sh_dbg_lreg_case *cases, int32_t n_cases, int32_t *n_kept, int32_t *rows)
{
    SH_CHECK(tab && cases && n_kept && rows && n_rows >= 1 && n_cases > 0 && n_cases <= DBG_MAX_CASES, SH_ERR_BAD_ARG, "sh_dbg_regs_long: bad argument");
    uint64_t at = 0;      // the cases lie one behind the other: no two share rows (they are rewritten in place)
    for (int32_t i = 0; i < n_cases; ++i) {
        const sh_dbg_lreg_case &c = cases[i];
        SH_CHECK(c.n >= 1 && c.n <= DBG_MAX_LREGS && c.off >= at && c.off <= n_rows && (uint64_t)c.n <= n_rows - c.off, SH_ERR_BAD_ARG,
                 "sh_dbg_regs_long: case %d: outside the table, overlapping the case before it, or not 1..%d regions", i, DBG_MAX_LREGS);
        at = c.off + (uint64_t)c.n;
        for (int32_t j = 0; j < c.n; ++j) SH_CHECK(tab[(c.off + (uint64_t)j) * 9 + 3] > tab[(c.off + (uint64_t)j) * 9 + 2], SH_ERR_BAD_ARG, "sh_dbg_regs_long: case %d: region %d is empty on the query", i, j);
    }
    SH_HIP(hipSetDevice(device));
    int32_t *d_tab = nullptr, *d_wpri = nullptr, *d_tmp = nullptr, *d_kept = nullptr, *d_rows = nullptr; sh_dbg_lreg_case *d_cases = nullptr; LReg *d_regs = nullptr; uint64_t *d_cov = nullptr;
    auto run = [&]() -> sh_status {
        SH_HIP(hipMalloc(&d_tab, 36 * n_rows)); SH_HIP(hipMalloc(&d_cases, sizeof(sh_dbg_lreg_case) * (size_t)n_cases)); SH_HIP(hipMalloc(&d_regs, sizeof(LReg) * n_rows));
        SH_HIP(hipMalloc(&d_cov, 8 * n_rows)); SH_HIP(hipMalloc(&d_wpri, 4 * n_rows)); SH_HIP(hipMalloc(&d_tmp, 4 * n_rows + 4));
        SH_HIP(hipMalloc(&d_kept, 4 * (size_t)n_cases)); SH_HIP(hipMalloc(&d_rows, 24 * n_rows));
        SH_HIP(hipMemset(d_rows, 0xff, 24 * n_rows)); SH_HIP(hipMemset(d_kept, 0xff, 4 * (size_t)n_cases));
        SH_HIP(hipMemcpy(d_tab, tab, 36 * n_rows, hipMemcpyHostToDevice));
        SH_HIP(hipMemcpy(d_cases, cases, sizeof(sh_dbg_lreg_case) * (size_t)n_cases, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_dbg_regs_long, dim3((uint32_t)n_cases), dim3(64), 0, 0, d_tab, d_cases, d_regs, d_cov, d_wpri, d_tmp, d_kept, d_rows);
        SH_HIP(hipGetLastError());
        SH_HIP(hipDeviceSynchronize());
        SH_HIP(hipMemcpy(n_kept, d_kept, 4 * (size_t)n_cases, hipMemcpyDeviceToHost));
        SH_HIP(hipMemcpy(rows, d_rows, 24 * n_rows, hipMemcpyDeviceToHost));
        return SH_OK;
    };
    const sh_status st = run();
    hipFree(d_tab); hipFree(d_cases); hipFree(d_regs); hipFree(d_cov); hipFree(d_wpri); hipFree(d_tmp); hipFree(d_kept); hipFree(d_rows);
    return st;
}
