// sh_dbg_chain.hip — test aid: the chaining DP and backtrack variants of sh_chain.h, called directly (tests/test_chain_gpu.py).
//
// sh_chain.h holds seven implementations of mg_lchain_dp and six ways to run mg_chain_backtrack, all reached through classify alone, where
// their output shows as n_chain / best_score.  Here a batch of hand-picked anchor sets runs one launch per DP variant, one block per case,
// with the block size and the LDS objects of the kernels that call the variant in the product, and f, p, t and the chain list come back.
// Nothing in the functions under test knows about this file.
#include "sh_common.h"
#include "sh_chain.h"

#define DBGC_MAX_CASES 16384
#define DBGC_MAX_N (1 << 20)          // anchors of one case
#define DBGC_SMALL_CAP 32
#define DBGC_NTHR_BLOCK 256           // k_sort_top<1024, 2, 256>
#define DBGC_NTHR_TILED 512           // k_giant_top

enum { DP_NONE = 0, DP_SEQ, DP_MASK, DP_SMALL, DP_WAVE, DP_RING, DP_PF_BLOCK, DP_PF_TILED, DP_N };
enum { BT_NONE = 0, BT_SMALL, BT_MASK, BT_HEAP, BT_WAVE_TOP, BT_BLOCK_TOP, BT_QUICK, BT_N };

struct DbgChainJob { sh_dbg_chain_case c; float pen_gap, pen_skip; unsigned long long o; };

// what a backtrack hands over, recorded: (zi, end_i, score, cnt, zf) per accepted chain, by one lane
struct DbgEmit {
    int32_t *rec, *cnt; int32_t cap; bool on;
    __device__ inline void operator()(int64_t zi, int64_t end_i, int32_t sc, int64_t n_anch, int32_t zf) const
    {
        if (!on) return;
        const int32_t s = *cnt;
        if (s < cap) { int32_t *r = rec + 5 * (size_t)s; r[0] = (int32_t)zi; r[1] = (int32_t)end_i; r[2] = sc; r[3] = (int32_t)n_anch; r[4] = zf; }
        *cnt = s + 1;
    }
    __device__ inline bool done(int32_t) const { return false; }
};

__device__ inline ChainParams dbg_chain_params(const DbgChainJob &J)
{
    ChainParams P{};      // the occurrence, pair and ext fields stay off
    const sh_dbg_chain_case &c = J.c;
    P.k = c.k; P.is_sr = c.is_sr; P.min_cnt = c.min_cnt; P.min_sc = c.min_sc; P.max_gap = c.max_gap; P.max_gap_ref = c.max_gap_ref;
    P.max_frag_len = c.max_frag_len; P.bw = c.bw; P.max_skip = c.max_skip; P.max_iter = c.max_iter;
    P.pen_gap = J.pen_gap; P.pen_skip = J.pen_skip; P.flag_stop = INT32_MAX;
    return P;
}

struct DbgChainBufs {
    const DbgChainJob *jobs; const uint32_t *order;
    const uint64_t *x; const uint32_t *qm, *qu;       // q with and without the cluster-start marks
    const int32_t *f_in, *p_in;
    int32_t *f, *pt, *p2, *t2; uint64_t *z;
    sh_dbg_chain_result *out; int32_t *of, *op, *ot, *chains;
};

// the variants one lane or one wave runs: DP 0..5, backtrack 0..4 and 6
__global__ void __launch_bounds__(64) k_dbg_chain_lane(DbgChainBufs B)
{
    __shared__ RingMem s_ring;
    __shared__ uint32_t s_lo[DBGC_SMALL_CAP * 64];
    __shared__ uint32_t s_aux[DBGC_SMALL_CAP * 64];
    __shared__ uint16_t s_q[DBGC_SMALL_CAP * 64];
    __shared__ uint8_t s_g[DBGC_SMALL_CAP * 64];
    const uint32_t ci = B.order[blockIdx.x], lane = threadIdx.x, act = ci & 63u;      // the single-lane variants run on lane (case % 64)
    const DbgChainJob J = B.jobs[ci];
    const sh_dbg_chain_case c = J.c;
    const ChainParams P = dbg_chain_params(J);
    const int32_t n = c.n;
    const uint64_t *x = B.x + c.off; const uint32_t *qm = B.qm + c.off, *qu = B.qu + c.off;
    int32_t *f = B.f + J.o, *pt = B.pt + 2 * J.o;
    SliceStore S{x, qm, f, pt};
    SmallStore<DBGC_SMALL_CAP> SS;
    SS.lo = s_lo + lane; SS.aux = s_aux + lane; SS.qv = s_q + lane; SS.gv = s_g + lane;
    DbgEmit em{B.chains + 5 * J.o, &B.out[ci].n_emit, n, false};
    int32_t ret = 0, bt_ret = 0, n_u = 0, best = 0;
    const bool small = c.dp == DP_SMALL;

    switch (c.dp) {      // uniform
    case DP_NONE:
        for (int32_t i = (int32_t)lane; i < n; i += 64) { f[i] = B.f_in[J.o + i]; pt[2 * i] = B.p_in[J.o + i]; pt[2 * i + 1] = 0; }
        break;
    case DP_SEQ:
        if (lane == act) {
            LargeStore LS{};
            LS.x = const_cast<uint64_t *>(x); LS.q = const_cast<uint32_t *>(qu); LS.f = f; LS.p = B.p2 + J.o; LS.t = B.t2 + J.o;
            ret = chain_dp<LargeStore, int64_t>(LS, (int64_t)n, c.qlen, P) ? 1 : 0;
            for (int32_t i = 0; i < n; ++i) { pt[2 * i] = LS.p[i]; pt[2 * i + 1] = LS.t[i]; }
        }
        break;
    case DP_MASK:
        if (lane == act) ret = chain_dp_mask(S, n, c.qlen, P) ? 1 : 0;
        break;
    case DP_SMALL:
        if (lane == act) {
            for (int32_t i = 0; i < n; ++i) SS.set_raw(i, x[i], qu[i]);
            SS.sort_finalize(n);
            ret = chain_dp_mask(SS, n, c.qlen, P) ? 1 : 0;
        }
        break;
    case DP_WAVE:
        ret = chain_dp_wave(S, n, c.qlen, P, lane) ? 1 : 0;
        break;
    case DP_RING:
        ret = chain_dp_ring(x, qm, f, pt, n, c.qlen, P, lane, s_ring) ? 1 : 0;
        break;
    }
    if (c.dp == DP_SEQ || c.dp == DP_MASK || c.dp == DP_SMALL) ret = wave_bcast(ret, (int)act);
    wave_mem_sync();
    __syncthreads();

    switch (c.bt) {      // uniform
    case BT_SMALL:
        if (lane == act) { em.on = true; backtrack_small(S, n, P, n_u, best, c.first_only != 0); }
        break;
    case BT_MASK:
        if (lane == act) {
            em.on = true;
            if (small) backtrack_mask(SS, n, P, n_u, best, c.first_only != 0, em);
            else backtrack_mask(S, n, P, n_u, best, c.first_only != 0, em);
        }
        break;
    case BT_HEAP:
        if (lane == act) { em.on = true; backtrack_heap<SliceStore, int32_t, DbgEmit>(S, n, P, B.z + J.o, n_u, best, c.first_only != 0, em); }
        break;
    case BT_WAVE_TOP:
        em.on = lane == 0;
        backtrack_wave_top(S, n, P, n_u, best, em, lane);
        break;
    case BT_QUICK:
        bt_ret = first_chain_quick(f, pt, n, P, lane);
        break;
    }
    wave_mem_sync();
    __syncthreads();
    const uint32_t rep = (c.bt == BT_WAVE_TOP || c.bt == BT_QUICK || (c.bt == BT_NONE && (c.dp == DP_WAVE || c.dp == DP_RING || c.dp == DP_NONE))) ? 0u : act;
    if (lane == rep) {
        sh_dbg_chain_result &r = B.out[ci];
        r.ret = ret; r.bt_ret = bt_ret; r.n_u = n_u; r.best = best;
        int32_t *of = B.of + J.o, *op = B.op + J.o, *ot = B.ot + J.o;
        if (small) for (int32_t i = 0; i < n; ++i) { of[i] = SS.F(i); op[i] = SS.Pm(i); ot[i] = SS.T(i); }
        else for (int32_t i = 0; i < n; ++i) { of[i] = f[i]; op[i] = pt[2 * i]; ot[i] = pt[2 * i + 1]; }
    }
}

// the variants a block runs: par_fill_block / par_fill_tiled, and backtrack_block_top behind them or over uploaded f / p
template <int NTHR, bool TILED>
__global__ void __launch_bounds__(NTHR) k_dbg_chain_block(DbgChainBufs B)
{
    __shared__ ParFillLds s_pf;
    __shared__ long long s_top[18];
    __shared__ uint32_t s_cf[TOPBT_MAX], s_ci[TOPBT_MAX];
    __shared__ int32_t s_cn;
    const uint32_t ci = B.order[blockIdx.x], tid = threadIdx.x;
    const DbgChainJob J = B.jobs[ci];
    const sh_dbg_chain_case c = J.c;
    const ChainParams P = dbg_chain_params(J);
    const int32_t n = c.n;
    const uint64_t *x = B.x + c.off; const uint32_t *qm = B.qm + c.off;
    int32_t *f = B.f + J.o, *pt = B.pt + 2 * J.o;
    bool ret = true, bt_ret = false;
    int32_t n_u = 0, best = 0;
    if constexpr (TILED) {
        __shared__ PfTile s_tile;
        ret = par_fill_tiled(x, qm, f, pt, (uint32_t)n, c.qlen, P, tid, NTHR, s_pf, s_tile, (uint32_t)c.g_min);
    } else if (c.dp == DP_PF_BLOCK) {
        ret = par_fill_block(x, qm, f, pt, (uint32_t)n, c.qlen, P, tid, NTHR, s_pf);
    } else {
        for (int32_t i = (int32_t)tid; i < n; i += NTHR) { f[i] = B.f_in[J.o + i]; pt[2 * i] = B.p_in[J.o + i]; pt[2 * i + 1] = 0; }
    }
    __threadfence_block();
    __syncthreads();
    if (c.bt == BT_BLOCK_TOP && ret) {      // uniform
        SliceStore S{x, qm, f, pt};
        ChainSink sink{};      // best == nullptr
        const DbgEmit em{B.chains + 5 * J.o, &B.out[ci].n_emit, n, tid == 0};
        bt_ret = backtrack_block_top(S, n, P, n_u, best, em, sink, 0u, tid, NTHR, s_top, s_cf, s_ci, &s_cn, (uint32_t)c.top_cap);
    }
    __threadfence_block();
    __syncthreads();
    if (tid == 0) { sh_dbg_chain_result &r = B.out[ci]; r.ret = ret ? 1 : 0; r.bt_ret = bt_ret ? 1 : 0; r.n_u = n_u; r.best = best; }
    if (ret) for (int32_t i = (int32_t)tid; i < n; i += NTHR) { B.of[J.o + i] = f[i]; B.op[J.o + i] = pt[2 * i]; B.ot[J.o + i] = pt[2 * i + 1]; }
}

extern "C" sh_status sh_dbg_chain(int32_t device, const uint64_t *x, const uint32_t *q, uint64_t n_total, const sh_dbg_chain_case *cases, int32_t n_cases,
                                  const int32_t *f_in, const int32_t *p_in, sh_dbg_chain_result *out, int32_t *f, int32_t *p, int32_t *t, int32_t *chains)
{
    SH_CHECK(x && q && cases && f_in && p_in && out && f && p && t && chains && n_cases > 0 && n_cases <= DBGC_MAX_CASES && n_total > 0, SH_ERR_BAD_ARG, "sh_dbg_chain: bad argument");
    std::vector<DbgChainJob> jobs((size_t)n_cases);
    std::vector<uint32_t> order[DP_N];
    unsigned long long o = 0;
    for (int32_t i = 0; i < n_cases; ++i) {
        const sh_dbg_chain_case &c = cases[i];
        SH_CHECK(c.n >= 1 && c.n <= DBGC_MAX_N && c.off <= n_total && (uint64_t)c.n <= n_total - c.off, SH_ERR_BAD_ARG, "sh_dbg_chain: case %d: anchors outside the arrays", i);
        SH_CHECK(c.dp >= 0 && c.dp < DP_N && c.bt >= 0 && c.bt < BT_N, SH_ERR_BAD_ARG, "sh_dbg_chain: case %d: unknown variant", i);
        const bool block_dp = c.dp == DP_PF_BLOCK || c.dp == DP_PF_TILED, block_bt = c.bt == BT_BLOCK_TOP;
        SH_CHECK(!(block_bt && c.dp != DP_NONE && !block_dp) && !(block_dp && c.bt != BT_NONE && !block_bt), SH_ERR_BAD_ARG, "sh_dbg_chain: case %d: backtrack %d does not go with DP %d", i, c.bt, c.dp);
        SH_CHECK(c.dp != DP_SMALL || c.bt == BT_NONE || c.bt == BT_MASK, SH_ERR_BAD_ARG, "sh_dbg_chain: case %d: over the SmallStore only backtrack_mask runs", i);
        SH_CHECK(c.k >= 1 && c.k <= (1 << 20) && c.qlen >= 1 && c.bw >= 0 && c.max_gap >= 0 && c.max_skip >= 0 && c.max_iter >= 1 && c.min_cnt >= 0 && c.min_sc >= 0, SH_ERR_BAD_ARG, "sh_dbg_chain: case %d: options out of range", i);
        SH_CHECK(!block_bt || (c.top_cap >= 1 && c.top_cap <= TOPBT_MAX), SH_ERR_BAD_ARG, "sh_dbg_chain: case %d: top_cap outside 1..%d", i, TOPBT_MAX);
        // what a variant cannot take
        SH_CHECK(!((c.dp == DP_MASK || c.bt == BT_MASK) && c.n > 64), SH_ERR_BAD_ARG, "sh_dbg_chain: case %d: the mask variants hold 64 anchors, not %d", i, c.n);
        SH_CHECK(c.dp != DP_RING || c.max_iter <= RING_TMAX_ITER, SH_ERR_BAD_ARG, "sh_dbg_chain: case %d: the ring takes max_iter <= %d", i, RING_TMAX_ITER);
        const uint64_t *cx = x + c.off; const uint32_t *cq = q + c.off;
        if (c.dp == DP_SMALL) {
            SH_CHECK(c.n <= DBGC_SMALL_CAP && (int64_t)c.k * c.n <= 65535, SH_ERR_BAD_ARG, "sh_dbg_chain: case %d: the SmallStore holds %d anchors and 16 bits of f", i, DBGC_SMALL_CAP);
            for (int32_t j = 0; j < c.n; ++j) SH_CHECK((cq[j] & 0x7fffffffu) <= 65535u, SH_ERR_BAD_ARG, "sh_dbg_chain: case %d: the SmallStore holds 16 bits of q", i);
        } else {
            for (int32_t j = 1; j < c.n; ++j) SH_CHECK(cx[j - 1] <= cx[j], SH_ERR_BAD_ARG, "sh_dbg_chain: case %d: anchors not sorted by x", i);
        }
        if (c.dp == DP_MASK || c.dp == DP_WAVE || c.dp == DP_RING)      // one cluster: SliceStore knows no groups
            SH_CHECK((cx[0] >> 32) == (cx[c.n - 1] >> 32), SH_ERR_BAD_ARG, "sh_dbg_chain: case %d: variant %d takes one strand of one contig", i, c.dp);
        if (block_dp) {
            SH_CHECK(cq[0] >> 31, SH_ERR_BAD_ARG, "sh_dbg_chain: case %d: the first anchor must carry the cluster-start mark", i);
            for (int32_t j = 0; j < c.n; ++j)      // the fills index a table of PF_MAX_Q query positions once they have let qlen pass
                SH_CHECK(c.qlen > PF_MAX_Q || (cq[j] & 0x7fffffffu) < PF_MAX_Q, SH_ERR_BAD_ARG, "sh_dbg_chain: case %d: q beyond the query position table", i);
        }
        if (c.dp == DP_NONE)
            for (int32_t j = 0; j < c.n; ++j) SH_CHECK(p_in[o + (unsigned)j] >= -1 && p_in[o + (unsigned)j] < j && f_in[o + (unsigned)j] >= 0, SH_ERR_BAD_ARG, "sh_dbg_chain: case %d: uploaded f / p are no DP state", i);
        jobs[(size_t)i].c = c;
        jobs[(size_t)i].pen_gap = chain_pen_of(c.chain_gap_scale, c.k);
        jobs[(size_t)i].pen_skip = chain_pen_of(c.chain_skip_scale, c.k);
        jobs[(size_t)i].o = o;
        order[c.dp == DP_NONE && block_bt ? DP_PF_BLOCK : c.dp].push_back((uint32_t)i);
        o += (unsigned long long)c.n;
    }
    const size_t tot = (size_t)o;
    std::vector<uint32_t> qu((size_t)n_total);
    for (uint64_t i = 0; i < n_total; ++i) qu[(size_t)i] = q[i] & 0x7fffffffu;
    SH_HIP(hipSetDevice(device));
    DbgChainBufs B{};
    uint64_t *d_x = nullptr, *d_z = nullptr; uint32_t *d_qm = nullptr, *d_qu = nullptr, *d_order = nullptr; DbgChainJob *d_jobs = nullptr;
    int32_t *d_fin = nullptr, *d_pin = nullptr, *d_f = nullptr, *d_pt = nullptr, *d_p2 = nullptr, *d_t2 = nullptr, *d_of = nullptr, *d_op = nullptr, *d_ot = nullptr, *d_ch = nullptr;
    sh_dbg_chain_result *d_out = nullptr;
    auto run = [&]() -> sh_status {
        SH_HIP(hipMalloc(&d_x, 8 * (size_t)n_total)); SH_HIP(hipMalloc(&d_qm, 4 * (size_t)n_total)); SH_HIP(hipMalloc(&d_qu, 4 * (size_t)n_total));
        SH_HIP(hipMalloc(&d_jobs, sizeof(DbgChainJob) * (size_t)n_cases)); SH_HIP(hipMalloc(&d_order, 4 * (size_t)n_cases)); SH_HIP(hipMalloc(&d_out, sizeof(sh_dbg_chain_result) * (size_t)n_cases));
        SH_HIP(hipMalloc(&d_fin, 4 * tot)); SH_HIP(hipMalloc(&d_pin, 4 * tot)); SH_HIP(hipMalloc(&d_f, 4 * tot)); SH_HIP(hipMalloc(&d_pt, 8 * tot)); SH_HIP(hipMalloc(&d_p2, 4 * tot));
        SH_HIP(hipMalloc(&d_t2, 4 * tot)); SH_HIP(hipMalloc(&d_z, 8 * tot)); SH_HIP(hipMalloc(&d_of, 4 * tot)); SH_HIP(hipMalloc(&d_op, 4 * tot)); SH_HIP(hipMalloc(&d_ot, 4 * tot));
        SH_HIP(hipMalloc(&d_ch, 20 * tot));
        SH_HIP(hipMemcpy(d_x, x, 8 * (size_t)n_total, hipMemcpyHostToDevice)); SH_HIP(hipMemcpy(d_qm, q, 4 * (size_t)n_total, hipMemcpyHostToDevice));
        SH_HIP(hipMemcpy(d_qu, qu.data(), 4 * (size_t)n_total, hipMemcpyHostToDevice));
        SH_HIP(hipMemcpy(d_jobs, jobs.data(), sizeof(DbgChainJob) * (size_t)n_cases, hipMemcpyHostToDevice));
        SH_HIP(hipMemcpy(d_fin, f_in, 4 * tot, hipMemcpyHostToDevice)); SH_HIP(hipMemcpy(d_pin, p_in, 4 * tot, hipMemcpyHostToDevice));
        SH_HIP(hipMemset(d_out, 0, sizeof(sh_dbg_chain_result) * (size_t)n_cases));
        SH_HIP(hipMemset(d_f, 0, 4 * tot)); SH_HIP(hipMemset(d_pt, 0, 8 * tot)); SH_HIP(hipMemset(d_p2, 0, 4 * tot)); SH_HIP(hipMemset(d_t2, 0, 4 * tot)); SH_HIP(hipMemset(d_z, 0, 8 * tot));
        SH_HIP(hipMemset(d_of, 0, 4 * tot)); SH_HIP(hipMemset(d_op, 0, 4 * tot)); SH_HIP(hipMemset(d_ot, 0, 4 * tot)); SH_HIP(hipMemset(d_ch, 0, 20 * tot));
        B.jobs = d_jobs; B.x = d_x; B.qm = d_qm; B.qu = d_qu; B.f_in = d_fin; B.p_in = d_pin; B.f = d_f; B.pt = d_pt; B.p2 = d_p2; B.t2 = d_t2; B.z = d_z;
        B.out = d_out; B.of = d_of; B.op = d_op; B.ot = d_ot; B.chains = d_ch;
        uint32_t at = 0;
        for (int v = 0; v < DP_N; ++v) {      // one launch per DP variant
            const uint32_t m = (uint32_t)order[v].size();
            if (!m) continue;
            SH_HIP(hipMemcpy(d_order + at, order[v].data(), 4 * (size_t)m, hipMemcpyHostToDevice));
            B.order = d_order + at;
            if (v == DP_PF_TILED) hipLaunchKernelGGL((k_dbg_chain_block<DBGC_NTHR_TILED, true>), dim3(m), dim3(DBGC_NTHR_TILED), 0, 0, B);
            else if (v == DP_PF_BLOCK) hipLaunchKernelGGL((k_dbg_chain_block<DBGC_NTHR_BLOCK, false>), dim3(m), dim3(DBGC_NTHR_BLOCK), 0, 0, B);
            else hipLaunchKernelGGL(k_dbg_chain_lane, dim3(m), dim3(64), 0, 0, B);
            SH_HIP(hipGetLastError());
            at += m;
        }
        SH_HIP(hipDeviceSynchronize());
        SH_HIP(hipMemcpy(out, d_out, sizeof(sh_dbg_chain_result) * (size_t)n_cases, hipMemcpyDeviceToHost));
        SH_HIP(hipMemcpy(f, d_of, 4 * tot, hipMemcpyDeviceToHost)); SH_HIP(hipMemcpy(p, d_op, 4 * tot, hipMemcpyDeviceToHost)); SH_HIP(hipMemcpy(t, d_ot, 4 * tot, hipMemcpyDeviceToHost));
        SH_HIP(hipMemcpy(chains, d_ch, 20 * tot, hipMemcpyDeviceToHost));
        return SH_OK;
    };
    const sh_status st = run();
    hipFree(d_x); hipFree(d_qm); hipFree(d_qu); hipFree(d_jobs); hipFree(d_order); hipFree(d_out); hipFree(d_fin); hipFree(d_pin); hipFree(d_f); hipFree(d_pt);
    hipFree(d_p2); hipFree(d_t2); hipFree(d_z); hipFree(d_of); hipFree(d_op); hipFree(d_ot); hipFree(d_ch);
    return st;
}

// ---- the block sort of the repeat path (block_merge_sort, sh_wave.h), called directly (tests/test_block_sort_gpu.py) ----
// One block per case with the LDS buffers of k_sort_lds<SORT_LDS_C>: load, sort, store whichever buffer the result ended in.
#define DBGS_MAX_N 4096               // SORT_LDS_C

struct DbgSortBufs { const sh_dbg_sort_case *cases; const uint32_t *order; const uint64_t *x; const uint32_t *q; uint64_t *ox; uint32_t *oq; };

template <int NTHR>
__global__ void __launch_bounds__(NTHR) k_dbg_block_sort(DbgSortBufs B)
{
    __shared__ uint64_t s_x[2][DBGS_MAX_N];
    __shared__ uint32_t s_q[2][DBGS_MAX_N];
    const sh_dbg_sort_case c = B.cases[B.order[blockIdx.x]];
    const uint32_t tid = threadIdx.x, n = (uint32_t)c.n;      // 1 <= n <= DBGS_MAX_N: checked before the launch
    for (uint32_t i = tid; i < n; i += NTHR) { s_x[0][i] = B.x[c.off + i]; s_q[0][i] = B.q[c.off + i]; }
    __syncthreads();
    const bool fl = block_merge_sort(&s_x[0][0], &s_q[0][0], &s_x[1][0], &s_q[1][0], n);
    const uint64_t *rx = fl ? s_x[1] : s_x[0]; const uint32_t *rq = fl ? s_q[1] : s_q[0];
    for (uint32_t i = tid; i < n; i += NTHR) { B.ox[c.off + i] = rx[i]; B.oq[c.off + i] = rq[i]; }
}

extern "C" sh_status sh_dbg_block_sort(int32_t device, const uint64_t *x, const uint32_t *q, uint64_t n_total, const sh_dbg_sort_case *cases, int32_t n_cases,
                                       uint64_t *out_x, uint32_t *out_q)
{
    SH_CHECK(x && q && cases && out_x && out_q && n_cases > 0 && n_cases <= DBGC_MAX_CASES && n_total > 0, SH_ERR_BAD_ARG, "sh_dbg_block_sort: bad argument");
    static const int32_t nthr_of[4] = {64, 128, 256, 512};
    std::vector<uint32_t> order[4];
    for (int32_t i = 0; i < n_cases; ++i) {
        const sh_dbg_sort_case &c = cases[i];
        SH_CHECK(c.n >= 1 && c.n <= DBGS_MAX_N && c.off <= n_total && (uint64_t)c.n <= n_total - c.off, SH_ERR_BAD_ARG, "sh_dbg_block_sort: case %d: 1..%d pairs inside the arrays, not %d at %llu", i, DBGS_MAX_N, c.n, (unsigned long long)c.off);
        int v = 0;
        while (v < 4 && nthr_of[v] != c.nthr) ++v;
        SH_CHECK(v < 4, SH_ERR_BAD_ARG, "sh_dbg_block_sort: case %d: 64, 128, 256 or 512 threads, not %d", i, c.nthr);
        order[v].push_back((uint32_t)i);
    }
    SH_HIP(hipSetDevice(device));
    uint64_t *d_x = nullptr, *d_ox = nullptr; uint32_t *d_q = nullptr, *d_oq = nullptr, *d_order = nullptr; sh_dbg_sort_case *d_cases = nullptr;
    auto run = [&]() -> sh_status {
        const size_t nt = (size_t)n_total;
        SH_HIP(hipMalloc(&d_x, 8 * nt)); SH_HIP(hipMalloc(&d_ox, 8 * nt)); SH_HIP(hipMalloc(&d_q, 4 * nt)); SH_HIP(hipMalloc(&d_oq, 4 * nt));
        SH_HIP(hipMalloc(&d_order, 4 * (size_t)n_cases)); SH_HIP(hipMalloc(&d_cases, sizeof(sh_dbg_sort_case) * (size_t)n_cases));
        SH_HIP(hipMemcpy(d_x, x, 8 * nt, hipMemcpyHostToDevice)); SH_HIP(hipMemcpy(d_q, q, 4 * nt, hipMemcpyHostToDevice));
        SH_HIP(hipMemcpy(d_cases, cases, sizeof(sh_dbg_sort_case) * (size_t)n_cases, hipMemcpyHostToDevice));
        SH_HIP(hipMemset(d_ox, 0, 8 * nt)); SH_HIP(hipMemset(d_oq, 0xff, 4 * nt));      // pairs no case covers come back as (0, ~0u)
        DbgSortBufs B{d_cases, nullptr, d_x, d_q, d_ox, d_oq};
        uint32_t at = 0;
        for (int v = 0; v < 4; ++v) {      // one launch per thread count
            const uint32_t m = (uint32_t)order[v].size();
            if (!m) continue;
            SH_HIP(hipMemcpy(d_order + at, order[v].data(), 4 * (size_t)m, hipMemcpyHostToDevice));
            B.order = d_order + at;
            if (v == 0) hipLaunchKernelGGL(k_dbg_block_sort<64>, dim3(m), dim3(64), 0, 0, B);
            else if (v == 1) hipLaunchKernelGGL(k_dbg_block_sort<128>, dim3(m), dim3(128), 0, 0, B);
            else if (v == 2) hipLaunchKernelGGL(k_dbg_block_sort<256>, dim3(m), dim3(256), 0, 0, B);
            else hipLaunchKernelGGL(k_dbg_block_sort<512>, dim3(m), dim3(512), 0, 0, B);
            SH_HIP(hipGetLastError());
            at += m;
        }
        SH_HIP(hipDeviceSynchronize());
        SH_HIP(hipMemcpy(out_x, d_ox, 8 * nt, hipMemcpyDeviceToHost)); SH_HIP(hipMemcpy(out_q, d_oq, 4 * nt, hipMemcpyDeviceToHost));
        return SH_OK;
    };
    const sh_status st = run();
    hipFree(d_x); hipFree(d_ox); hipFree(d_q); hipFree(d_oq); hipFree(d_order); hipFree(d_cases);
    return st;
}

// ---- the repeat path's late anchors (stage_anchors, sh_chain.h), called directly (tests/test_stage_anchors_gpu.py) ----
// Per case a read of 1..64 seed records and a range [c0, c0 + m) of its anchors.  First the definition: one thread per case runs seed_filter
// on a copy of the records and walks the seeds in order, make_anchor per occurrence (what gen_anchors does), keeping the range; it also leaves
// the read's anchor count.  Then one block of nthr threads per case stages the range into the first LDS sort buffer, scratch in the second,
// as the sort kernels do, and stores it.  A range that reaches past the read's anchors is not staged.
struct DbgStageBufs {
    const sh_dbg_stage_case *cases; const uint32_t *order; const uint4 *rec; uint4 *rec_copy; const uint64_t *pos;
    uint64_t *ox, *rx; uint32_t *oq, *rq, *total; ChainParams P; int32_t max_occ;
};

__global__ void __launch_bounds__(64) k_dbg_stage_ref(DbgStageBufs B)
{
    if (threadIdx.x != 0) return;
    const sh_dbg_stage_case c = B.cases[blockIdx.x];
    uint4 *mine = B.rec_copy + 64 * (size_t)blockIdx.x;
    for (int32_t i = 0; i < c.n_seed; ++i) { uint4 r = B.rec[c.rec_off + i]; r.z &= SH_REC_OCC_MASK; mine[i] = r; }
    const SeedView sv{mine, 1u, (uint32_t)c.n_seed};
    int64_t n_a = 0; int32_t rep_len = 0;
    seed_filter(sv, c.qlen, B.max_occ, B.P, n_a, rep_len);
    B.total[blockIdx.x] = n_a > 0xffffffffll ? 0xffffffffu : (uint32_t)n_a;
    uint64_t at = 0;
    for (uint32_t i = 0; i < sv.n; ++i) {
        const uint4 s = sv.get(i);
        if (s.z >> 31) continue;
        const uint32_t occ = s.z & SH_REC_OCC_MASK;
        const uint64_t w1 = (uint64_t)s.y << 32 | s.x;
        for (uint32_t t = 0; t < occ; ++t, ++at) {
            if (at < c.c0 || at >= (uint64_t)c.c0 + c.m) continue;
            uint64_t x; uint32_t q;
            make_anchor(occ == 1 ? w1 : B.pos[(w1 >> SH_SLOT_NBITS) + t], s.w, c.qlen, B.P.k, x, q);
            B.rx[c.out_off + (at - c.c0)] = x; B.rq[c.out_off + (at - c.c0)] = q;
        }
    }
}

template <int NTHR>
__global__ void __launch_bounds__(NTHR) k_dbg_stage(DbgStageBufs B)
{
    __shared__ uint64_t s_x[2][DBGS_MAX_N];
    __shared__ uint32_t s_q[2][DBGS_MAX_N];
    static_assert(STAGE_SCRATCH_U32 * 4 <= 8 * 256, "the scratch fits the second sort buffer of the smallest class");
    const uint32_t ci = B.order[blockIdx.x];
    const sh_dbg_stage_case c = B.cases[ci];
    const uint32_t tid = threadIdx.x;
    if ((uint64_t)c.c0 + c.m > B.total[ci]) return;      // uniform
    stage_anchors(B.rec + c.rec_off, (uint32_t)c.n_seed, c.qlen, B.pos, B.max_occ, B.P, c.c0, c.m, &s_x[0][0], &s_q[0][0], tid, (uint32_t)NTHR, (uint32_t *)&s_x[1][0]);
    __syncthreads();
    for (uint32_t i = tid; i < c.m; i += NTHR) { B.ox[c.out_off + i] = s_x[0][i]; B.oq[c.out_off + i] = s_q[0][i]; }
}

extern "C" sh_status sh_dbg_stage_anchors(int32_t device, const uint32_t *records, uint64_t n_records, const uint64_t *positions, uint64_t n_positions,
                                          int32_t k, int32_t max_occ, int32_t max_max_occ, int32_t occ_dist, const sh_dbg_stage_case *cases, int32_t n_cases,
                                          uint64_t n_out, uint64_t *out_x, uint32_t *out_q, uint64_t *ref_x, uint32_t *ref_q, uint32_t *total)
{
    SH_CHECK(records && positions && cases && out_x && out_q && ref_x && ref_q && total && n_cases > 0 && n_cases <= DBGC_MAX_CASES && n_records > 0 &&
             n_positions > 0 && n_out > 0 && k > 0 && k <= 31 && max_occ >= 0, SH_ERR_BAD_ARG, "sh_dbg_stage_anchors: bad argument");
    static const int32_t nthr_of[4] = {64, 128, 256, 512};
    std::vector<uint32_t> order[4];
    for (int32_t i = 0; i < n_cases; ++i) {
        const sh_dbg_stage_case &c = cases[i];
        SH_CHECK(c.n_seed >= 1 && c.n_seed <= 64 && c.rec_off <= n_records && (uint64_t)c.n_seed <= n_records - c.rec_off, SH_ERR_BAD_ARG, "sh_dbg_stage_anchors: case %d: 1..64 seed records inside the array, not %d at %llu", i, c.n_seed, (unsigned long long)c.rec_off);
        SH_CHECK(c.m >= 1 && c.m <= DBGS_MAX_N && c.c0 <= (1u << 30) && c.out_off <= n_out && (uint64_t)c.m <= n_out - c.out_off && c.qlen > 0, SH_ERR_BAD_ARG, "sh_dbg_stage_anchors: case %d: 1..%d anchors from %u inside the outputs, not %u at %llu", i, DBGS_MAX_N, c.c0, c.m, (unsigned long long)c.out_off);
        uint64_t sum = 0;
        for (int32_t j = 0; j < c.n_seed; ++j) {      // every occurrence list inside positions[]
            const uint32_t *r = records + 4 * (c.rec_off + (uint64_t)j);
            const uint64_t w1 = (uint64_t)r[1] << 32 | r[0], occ = r[2] & SH_REC_OCC_MASK, slot = w1 >> SH_SLOT_NBITS;
            SH_CHECK(occ >= 1 && (occ == 1 || (slot <= n_positions && occ <= n_positions - slot)), SH_ERR_BAD_ARG, "sh_dbg_stage_anchors: case %d, seed %d: %llu occurrences at %llu of %llu", i, j, (unsigned long long)occ, (unsigned long long)slot, (unsigned long long)n_positions);
            sum += occ;
        }
        SH_CHECK(sum <= (1u << 24), SH_ERR_BAD_ARG, "sh_dbg_stage_anchors: case %d: %llu occurrences", i, (unsigned long long)sum);
        int v = 0;
        while (v < 4 && nthr_of[v] != c.nthr) ++v;
        SH_CHECK(v < 4, SH_ERR_BAD_ARG, "sh_dbg_stage_anchors: case %d: 64, 128, 256 or 512 threads, not %d", i, c.nthr);
        order[v].push_back((uint32_t)i);
    }
    SH_HIP(hipSetDevice(device));
    uint4 *d_rec = nullptr, *d_copy = nullptr; uint64_t *d_pos = nullptr, *d_ox = nullptr, *d_rx = nullptr; uint32_t *d_oq = nullptr, *d_rq = nullptr, *d_total = nullptr, *d_order = nullptr;
    sh_dbg_stage_case *d_cases = nullptr;
    auto run = [&]() -> sh_status {
        const size_t no = (size_t)n_out, nc = (size_t)n_cases;
        SH_HIP(hipMalloc(&d_rec, 16 * (size_t)n_records)); SH_HIP(hipMalloc(&d_copy, 16 * 64 * nc)); SH_HIP(hipMalloc(&d_pos, 8 * (size_t)n_positions));
        SH_HIP(hipMalloc(&d_ox, 8 * no)); SH_HIP(hipMalloc(&d_rx, 8 * no)); SH_HIP(hipMalloc(&d_oq, 4 * no)); SH_HIP(hipMalloc(&d_rq, 4 * no));
        SH_HIP(hipMalloc(&d_total, 4 * nc)); SH_HIP(hipMalloc(&d_order, 4 * nc)); SH_HIP(hipMalloc(&d_cases, sizeof(sh_dbg_stage_case) * nc));
        SH_HIP(hipMemcpy(d_rec, records, 16 * (size_t)n_records, hipMemcpyHostToDevice)); SH_HIP(hipMemcpy(d_pos, positions, 8 * (size_t)n_positions, hipMemcpyHostToDevice));
        SH_HIP(hipMemcpy(d_cases, cases, sizeof(sh_dbg_stage_case) * nc, hipMemcpyHostToDevice));
        SH_HIP(hipMemset(d_ox, 0, 8 * no)); SH_HIP(hipMemset(d_rx, 0, 8 * no)); SH_HIP(hipMemset(d_oq, 0xff, 4 * no)); SH_HIP(hipMemset(d_rq, 0xff, 4 * no));      // what no case covers: (0, ~0u)
        DbgStageBufs B{d_cases, nullptr, d_rec, d_copy, d_pos, d_ox, d_rx, d_oq, d_rq, d_total, ChainParams{}, max_occ};
        B.P.k = k; B.P.max_occ = max_occ; B.P.max_max_occ = max_max_occ; B.P.occ_dist = occ_dist;      // what the filter and make_anchor read
        hipLaunchKernelGGL(k_dbg_stage_ref, dim3((uint32_t)n_cases), dim3(64), 0, 0, B);
        SH_HIP(hipGetLastError());
        uint32_t at = 0;
        for (int v = 0; v < 4; ++v) {      // one launch per thread count
            const uint32_t m = (uint32_t)order[v].size();
            if (!m) continue;
            SH_HIP(hipMemcpy(d_order + at, order[v].data(), 4 * (size_t)m, hipMemcpyHostToDevice));
            B.order = d_order + at;
            if (v == 0) hipLaunchKernelGGL(k_dbg_stage<64>, dim3(m), dim3(64), 0, 0, B);
            else if (v == 1) hipLaunchKernelGGL(k_dbg_stage<128>, dim3(m), dim3(128), 0, 0, B);
            else if (v == 2) hipLaunchKernelGGL(k_dbg_stage<256>, dim3(m), dim3(256), 0, 0, B);
            else hipLaunchKernelGGL(k_dbg_stage<512>, dim3(m), dim3(512), 0, 0, B);
            SH_HIP(hipGetLastError());
            at += m;
        }
        SH_HIP(hipDeviceSynchronize());
        SH_HIP(hipMemcpy(out_x, d_ox, 8 * no, hipMemcpyDeviceToHost)); SH_HIP(hipMemcpy(out_q, d_oq, 4 * no, hipMemcpyDeviceToHost));
        SH_HIP(hipMemcpy(ref_x, d_rx, 8 * no, hipMemcpyDeviceToHost)); SH_HIP(hipMemcpy(ref_q, d_rq, 4 * no, hipMemcpyDeviceToHost));
        SH_HIP(hipMemcpy(total, d_total, 4 * nc, hipMemcpyDeviceToHost));
        return SH_OK;
    };
    const sh_status st = run();
    hipFree(d_rec); hipFree(d_copy); hipFree(d_pos); hipFree(d_ox); hipFree(d_rx); hipFree(d_oq); hipFree(d_rq); hipFree(d_total); hipFree(d_order); hipFree(d_cases);
    return st;
}
