// sh_dbg_long.hip — test aid: the long join of sh_long.h (mg_lchain_rmq on one wave), called directly (tests/test_long_join_gpu.py).
//
// lr_rmq_fill<NR, TREE, FAT> is reached through whole classify calls alone, where a wrong predecessor at one of its edges (the ring's last
// block, the tie rule, the replayed tree, a run of lr_coop) changes a chain and not necessarily a flag.  Here a table of hand-made anchor sets
// runs one launch per instance the product launches (they differ in LDS), one 64-lane block per case, called the way lr_chains_wave and
// lr_coop call them, and f, p, n_tie, the return value and the backtrack's chains come back.  Every array a case's block writes lies between
// two bands of DBGL_GUARD_BYTE; the result says how many of those bytes changed.  Nothing in the functions under test knows about this file.
#include "sh_common.h"
#include "sh_long.h"
#include <map>

#define DBGL_MAX_CASES 16384
#define DBGL_MAX_N (1 << 20)          // anchors of one case
#define DBGL_GUARD 4096
#define DBGL_GUARD_BYTE 0xA5
#define DBGL_TRY(call) do { const sh_status st_ = (call); if (st_ != SH_OK) return st_; } while (0)

enum { LF_NONE = 0, LF_512, LF_4096, LF_4096_FAT, LF_TREE_1024, LF_TREE_4096, LF_ONE_LANE, LF_RUNS, LF_COOP, LF_N };
enum { LB_NONE = 0, LB_LANE0, LB_WAVE, LB_N };

struct DbgLongJob {
    sh_dbg_long_case c; unsigned long long o;
    int32_t *f, *p, *t, *v; uint64_t *u; double *pri, *bmin; SKey *sk, *sk2; RqNode *rq0, *rq1;
};
struct DbgLongBufs {
    const DbgLongJob *jobs; const uint32_t *order; const LAnchor *a; const int32_t *f_in, *p_in, *cuts;
    sh_dbg_long_result *out; LongCoop coop;
};

__device__ inline LongParams dbg_long_params(const sh_dbg_long_case &c)
{
    LongParams P{};      // what the join and lr_coop read; everything else stays off
    P.k = c.k; P.min_cnt = c.min_cnt; P.min_sc = c.min_sc; P.max_gap = c.max_gap; P.bw_long = c.bw_long;
    P.max_skip = c.max_skip; P.rmq_inner_dist = c.rmq_inner_dist; P.rmq_size_cap = c.rmq_size_cap;
    P.pen_gap = c.pen_gap; P.pen_skip = c.pen_skip; P.coop_min = c.coop_min; P.coop_run = c.coop_run; P.coop_check = 0;
    return P;
}

template <int NR, bool TREE, bool FAT>
__global__ void __launch_bounds__(64) k_dbg_long(DbgLongBufs B)
{
    __shared__ RmqLdsT<NR, FAT> RL;
    constexpr int TCAP = TREE ? (NR >= 4096 ? 1792 : 1664) : 1;      // k_long_chains
    __shared__ RqLdsMem<TCAP> TM;
    RqLds TL{};
    if (TREE) TL.init(TM);
    const int32_t lane = (int32_t)threadIdx.x;
    const DbgLongJob J = B.jobs[B.order[blockIdx.x]];
    const sh_dbg_long_case c = J.c;
    const LongParams P = dbg_long_params(c);
    const LongCoop coop = B.coop;
    const int32_t n = c.n;
    const LAnchor *a = B.a + c.off;
    bool ok = true;
    int32_t tie = 0;

    if constexpr (TREE) {
        if (c.fill == LF_RUNS) {      // the runs as lr_coop_take and the local branch of lr_coop_fill fill them
            const int32_t *cut = B.cuts + c.cut_off;
            for (int32_t i = 0; i <= c.n_cut; ++i) {
                const int32_t j0 = i == 0 ? 0 : cut[i - 1], j1 = i == c.n_cut ? n : cut[i];
                int32_t tr = 0;
                if (ok && !lr_rmq_fill<NR, true, FAT>(P, P.max_gap, P.bw_long, j1 - j0, a + j0, J.f + j0, J.p + j0, J.pri + j0, J.bmin + (j0 / 64 + i), RL, tr, nullptr, TL, j0)) ok = false;
                tie += tr;
            }
        } else if (c.fill == LF_COOP && n >= P.coop_min) {
            ok = lr_coop_fill<NR, FAT>(P, coop, blockIdx.x, n, a, J.f, J.p, J.pri, J.bmin, J.t, RL, TL, tie);
        } else {
            ok = lr_rmq_fill<NR, true, FAT>(P, P.max_gap, P.bw_long, n, a, J.f, J.p, J.pri, J.bmin, RL, tie, nullptr, TL);
        }
    } else {
        if (c.fill == LF_NONE) {
            for (int32_t i = lane; i < n; i += 64) { J.f[i] = B.f_in[J.o + i]; J.p[i] = B.p_in[J.o + i]; }
        } else if (c.fill == LF_ONE_LANE) {
            for (int32_t i = lane; i < n; i += 64) J.t[i] = 0;
            lr_sync();
            ok = lr_rmq_fill_tree(P, P.max_gap, P.bw_long, n, a, J.f, J.p, J.t, J.rq0, J.rq1, n + 2);
        } else {
            ok = lr_rmq_fill<NR, false, FAT>(P, P.max_gap, P.bw_long, n, a, J.f, J.p, J.pri, J.bmin, RL, tie);
        }
    }
    lr_sync();

    int32_t n_z = 0, res[3] = {0, 0, 0};
    bool ovf = false;
    if (c.bt != LB_NONE && ok) {      // mg_chain_backtrack as lr_chains_wave sets it up: the candidates compacted, sorted by (f, index)
        for (int32_t i0 = 0; i0 < n; i0 += 64) {
            const int32_t i = i0 + lane;
            const bool cd = i < n && J.f[i] >= P.min_sc;
            const uint64_t m = __ballot(cd);
            if (cd) { const int32_t d = n_z + (int32_t)prefix_popc64(m); J.sk[d].k = (uint64_t)(uint32_t)J.f[i]; J.sk[d].v = (uint64_t)i; }
            n_z += (int32_t)__popcll(m);
        }
        lr_sync();
        lr_sort(J.sk, J.sk2, n_z);
        for (int32_t i = lane; i < n; i += 64) J.t[i] = 0;
        lr_sync();
        int32_t n_v = 0, best = 0;
        if (c.bt == LB_WAVE) res[0] = lr_backtrack_wave(J.sk, n_z, n, J.f, J.p, J.t, J.v, J.u, (uint32_t)c.cap_u, P.min_cnt, P.min_sc, c.max_drop, n_v, best, ovf);
        else if (lane == 0) res[0] = lr_backtrack0(J.sk, n_z, J.f, J.p, J.t, J.v, J.u, (uint32_t)c.cap_u, P.min_cnt, P.min_sc, c.max_drop, n_v, best, ovf);
        res[1] = n_v; res[2] = best;
        lr_sync();
    }
    if (lane == 0) {
        sh_dbg_long_result &r = B.out[B.order[blockIdx.x]];
        r.ok = ok ? 1 : 0; r.n_tie = tie; r.n_u = res[0]; r.n_v = res[1]; r.best = res[2]; r.ovf = ovf ? 1 : 0; r.n_z = n_z;
    }
}

extern "C" sh_status sh_dbg_long_join(int32_t device, const uint64_t *x, const uint64_t *y, uint64_t n_total, const sh_dbg_long_case *cases, int32_t n_cases,
                                      const int32_t *f_in, const int32_t *p_in, const int32_t *cuts, sh_dbg_long_result *out,
                                      int32_t *f, int32_t *p, int32_t *t, uint64_t *u, int32_t *v)
{
    SH_CHECK(x && y && cases && f_in && p_in && out && f && p && t && u && v && n_cases > 0 && n_cases <= DBGL_MAX_CASES && n_total > 0,
             SH_ERR_BAD_ARG, "sh_dbg_long_join: bad argument");
    struct Span { unsigned long long at, bytes; };
    struct Lay { Span f, p, t, v, u, pri, bmin, sk, sk2, rq0, rq1; unsigned long long lo, hi; };
    std::vector<DbgLongJob> jobs((size_t)n_cases);
    std::vector<Lay> lay((size_t)n_cases);
    std::vector<uint32_t> order[5];
    // lr_coop_take fills a run with the LongParams of the wave that TAKES it (in the product one launch has one LongParams), so the cases that
    // share a queue must agree on everything the fill reads: one launch per (ring, q_cap, fill options)
    std::map<std::vector<int32_t>, std::vector<uint32_t>> coop_order;
    unsigned long long o = 0, bytes = 0;
    uint64_t n_cuts_total = 0;      // cuts[] reaches as far as the cases say
    for (int32_t i = 0; i < n_cases; ++i) {
        const sh_dbg_long_case &c = cases[i];
        SH_CHECK(c.n >= 1 && c.n <= DBGL_MAX_N && c.off <= n_total && (uint64_t)c.n <= n_total - c.off, SH_ERR_BAD_ARG, "sh_dbg_long_join: case %d: anchors outside the arrays", i);
        SH_CHECK(c.fill >= 0 && c.fill < LF_N && c.bt >= 0 && c.bt < LB_N, SH_ERR_BAD_ARG, "sh_dbg_long_join: case %d: unknown variant", i);
        SH_CHECK((c.fill != LF_RUNS && c.fill != LF_COOP) || c.ring == 1024 || c.ring == 4096, SH_ERR_BAD_ARG, "sh_dbg_long_join: case %d: the runs take the ring of 1024 or 4096 anchors, not %d", i, c.ring);
        SH_CHECK(c.k >= 1 && c.k <= 255 && c.max_gap >= 0 && c.bw_long >= 0 && c.max_skip >= 0 && c.rmq_size_cap >= 0 && c.min_cnt >= 0 && c.min_sc >= 0 && c.max_drop >= 0 &&
                 c.cap_u >= 1 && c.coop_min >= 1 && c.coop_run >= 2 && c.q_cap >= 0 && c.q_cap <= (1 << 20), SH_ERR_BAD_ARG, "sh_dbg_long_join: case %d: options out of range", i);
        const uint64_t *cx = x + c.off, *cy = y + c.off;
        const uint64_t max_dist = (uint64_t)(c.max_gap > c.bw_long ? c.max_gap : c.bw_long);
        int32_t n_starts = 0;
        for (int32_t j = 0; j < c.n; ++j) {
            SH_CHECK(j == 0 || cx[j - 1] <= cx[j], SH_ERR_BAD_ARG, "sh_dbg_long_join: case %d: anchors not ascending in x at %d", i, j);
            SH_CHECK((cy[j] >> 32) == (uint64_t)c.k, SH_ERR_BAD_ARG, "sh_dbg_long_join: case %d: anchor %d has a q_span other than k (the ring scores with k)", i, j);
            const int64_t xl = (int64_t)(int32_t)(uint32_t)cx[j], yl = (int64_t)(int32_t)(uint32_t)cy[j];
            SH_CHECK(xl >= 0 && yl >= 0 && xl + yl <= INT32_MAX, SH_ERR_BAD_ARG, "sh_dbg_long_join: case %d: x + y of anchor %d beyond int32", i, j);
            if (j > 0 && ((cx[j] >> 32) != (cx[j - 1] >> 32) || cx[j] > cx[j - 1] + max_dist)) ++n_starts;
        }
        if (c.fill == LF_RUNS) {
            SH_CHECK(c.n_cut >= 0 && c.n_cut < c.n && c.cut_off <= (1ull << 32) && (c.n_cut == 0 || cuts), SH_ERR_BAD_ARG, "sh_dbg_long_join: case %d: %d cuts at %llu", i, c.n_cut, (unsigned long long)c.cut_off);
            if (c.cut_off + (uint64_t)c.n_cut > n_cuts_total) n_cuts_total = c.cut_off + (uint64_t)c.n_cut;
            int32_t last = 0;
            for (int32_t q = 0; q < c.n_cut; ++q) {
                const int32_t j = cuts[c.cut_off + (uint64_t)q];
                SH_CHECK(j > last && j < c.n && ((cx[j] >> 32) != (cx[j - 1] >> 32) || cx[j] > cx[j - 1] + max_dist), SH_ERR_BAD_ARG, "sh_dbg_long_join: case %d: cut %d at %d is no stretch start", i, q, j);
                last = j;
            }
        }
        if (c.fill == LF_NONE)
            for (int32_t j = 0; j < c.n; ++j) SH_CHECK(p_in[o + (unsigned)j] >= -1 && p_in[o + (unsigned)j] < j && f_in[o + (unsigned)j] >= 0, SH_ERR_BAD_ARG, "sh_dbg_long_join: case %d: uploaded f / p are no chaining state", i);
        DbgLongJob &J = jobs[(size_t)i];
        J.c = c; J.o = o;
        // the case's arrays, each between two guard bands (what lies between an array's end and the next 16 bytes belongs to the band)
        Lay &Y = lay[(size_t)i];
        const unsigned long long nn = (unsigned long long)c.n;
        const unsigned long long n_runs = c.fill == LF_RUNS ? (unsigned long long)c.n_cut + 1 : c.fill == LF_COOP ? (unsigned long long)n_starts + 1 : 0;
        Y.lo = bytes;
        auto take = [&](Span &s, unsigned long long b) { bytes += DBGL_GUARD; s.at = bytes; s.bytes = b; bytes += (b + 15) & ~15ull; };
        take(Y.f, 4 * nn); take(Y.p, 4 * nn); take(Y.t, 4 * nn); take(Y.v, 4 * nn);
        take(Y.u, 8 * ((unsigned long long)c.cap_u < nn ? (unsigned long long)c.cap_u : nn));
        take(Y.pri, 8 * nn); take(Y.bmin, 8 * (nn / 64 + 1 + n_runs));
        take(Y.sk, sizeof(SKey) * nn); take(Y.sk2, sizeof(SKey) * nn);
        take(Y.rq0, c.fill == LF_ONE_LANE ? sizeof(RqNode) * (nn + 2) : 0); take(Y.rq1, c.fill == LF_ONE_LANE ? sizeof(RqNode) * (nn + 2) : 0);
        bytes += DBGL_GUARD;
        Y.hi = bytes;
        switch (c.fill) {
        case LF_NONE: case LF_512: case LF_ONE_LANE: order[0].push_back((uint32_t)i); break;
        case LF_4096: order[1].push_back((uint32_t)i); break;
        case LF_4096_FAT: order[2].push_back((uint32_t)i); break;
        case LF_TREE_1024: order[3].push_back((uint32_t)i); break;
        case LF_TREE_4096: order[4].push_back((uint32_t)i); break;
        case LF_RUNS: order[c.ring == 1024 ? 3 : 4].push_back((uint32_t)i); break;
        default: {
            int32_t pg, ps;
            memcpy(&pg, &c.pen_gap, 4); memcpy(&ps, &c.pen_skip, 4);
            coop_order[{c.ring, c.q_cap, c.k, c.max_gap, c.bw_long, c.max_skip, c.rmq_inner_dist, c.rmq_size_cap, pg, ps}].push_back((uint32_t)i);
            break;
        }
        }
        o += nn;
    }
    const size_t tot = (size_t)o;
    std::vector<LAnchor> an((size_t)n_total);
    for (uint64_t i = 0; i < n_total; ++i) { an[(size_t)i].x = x[i]; an[(size_t)i].y = y[i]; }
    SH_HIP(hipSetDevice(device));
    uint8_t *d_mem = nullptr, *d_q = nullptr; LAnchor *d_a = nullptr; DbgLongJob *d_jobs = nullptr; uint32_t *d_order = nullptr;
    int32_t *d_fin = nullptr, *d_pin = nullptr, *d_cuts = nullptr; sh_dbg_long_result *d_out = nullptr;
    std::vector<uint8_t> back;
    auto run = [&]() -> sh_status {
        SH_HIP(hipMalloc(&d_mem, (size_t)bytes)); SH_HIP(hipMemset(d_mem, DBGL_GUARD_BYTE, (size_t)bytes));
        for (int32_t i = 0; i < n_cases; ++i) {
            DbgLongJob &J = jobs[(size_t)i]; const Lay &Y = lay[(size_t)i];
            J.f = (int32_t *)(d_mem + Y.f.at); J.p = (int32_t *)(d_mem + Y.p.at); J.t = (int32_t *)(d_mem + Y.t.at); J.v = (int32_t *)(d_mem + Y.v.at);
            J.u = (uint64_t *)(d_mem + Y.u.at); J.pri = (double *)(d_mem + Y.pri.at); J.bmin = (double *)(d_mem + Y.bmin.at);
            J.sk = (SKey *)(d_mem + Y.sk.at); J.sk2 = (SKey *)(d_mem + Y.sk2.at); J.rq0 = (RqNode *)(d_mem + Y.rq0.at); J.rq1 = (RqNode *)(d_mem + Y.rq1.at);
        }
        SH_HIP(hipMalloc(&d_a, sizeof(LAnchor) * (size_t)n_total)); SH_HIP(hipMalloc(&d_jobs, sizeof(DbgLongJob) * (size_t)n_cases));
        SH_HIP(hipMalloc(&d_order, 4 * (size_t)n_cases)); SH_HIP(hipMalloc(&d_out, sizeof(sh_dbg_long_result) * (size_t)n_cases));
        SH_HIP(hipMalloc(&d_fin, 4 * tot)); SH_HIP(hipMalloc(&d_pin, 4 * tot)); SH_HIP(hipMalloc(&d_cuts, 4 * (size_t)(n_cuts_total ? n_cuts_total : 1)));
        SH_HIP(hipMemcpy(d_a, an.data(), sizeof(LAnchor) * (size_t)n_total, hipMemcpyHostToDevice));
        SH_HIP(hipMemcpy(d_jobs, jobs.data(), sizeof(DbgLongJob) * (size_t)n_cases, hipMemcpyHostToDevice));
        SH_HIP(hipMemcpy(d_fin, f_in, 4 * tot, hipMemcpyHostToDevice)); SH_HIP(hipMemcpy(d_pin, p_in, 4 * tot, hipMemcpyHostToDevice));
        if (n_cuts_total) SH_HIP(hipMemcpy(d_cuts, cuts, 4 * (size_t)n_cuts_total, hipMemcpyHostToDevice));
        SH_HIP(hipMemset(d_out, 0, sizeof(sh_dbg_long_result) * (size_t)n_cases));
        DbgLongBufs B{};
        B.jobs = d_jobs; B.a = d_a; B.f_in = d_fin; B.p_in = d_pin; B.cuts = d_cuts; B.out = d_out;
        uint32_t at = 0;
        auto launch = [&](int inst, const std::vector<uint32_t> &ord) -> sh_status {
            const uint32_t m = (uint32_t)ord.size();
            SH_HIP(hipMemcpy(d_order + at, ord.data(), 4 * (size_t)m, hipMemcpyHostToDevice));
            B.order = d_order + at;
            switch (inst) {
            case 0: hipLaunchKernelGGL((k_dbg_long<512, false, false>), dim3(m), dim3(64), 0, 0, B); break;
            case 1: hipLaunchKernelGGL((k_dbg_long<4096, false, false>), dim3(m), dim3(64), 0, 0, B); break;
            case 2: hipLaunchKernelGGL((k_dbg_long<4096, false, true>), dim3(m), dim3(64), 0, 0, B); break;
            case 3: hipLaunchKernelGGL((k_dbg_long<1024, true, false>), dim3(m), dim3(64), 0, 0, B); break;
            default: hipLaunchKernelGGL((k_dbg_long<4096, true, false>), dim3(m), dim3(64), 0, 0, B); break;
            }
            SH_HIP(hipGetLastError());
            at += m;
            return SH_OK;
        };
        for (int inst = 0; inst < 5; ++inst) if (!order[inst].empty()) DBGL_TRY(launch(inst, order[inst]));      // one launch per instance
        // lr_coop_fill: one launch per (ring, q_cap, fill options), its cases the owners of one queue
        size_t q_bytes = 0;
        for (const auto &kv : coop_order) {
            const size_t cap = (size_t)(kv.first[1] > 0 ? kv.first[1] : 1), m = kv.second.size();
            const size_t need = 16 * cap + 4 * cap + 256 + sizeof(LongCoopDesc) * m + 64;
            if (need > q_bytes) q_bytes = need;
        }
        if (q_bytes) SH_HIP(hipMalloc(&d_q, q_bytes));
        for (const auto &kv : coop_order) {
            const size_t cap = (size_t)(kv.first[1] > 0 ? kv.first[1] : 1);
            SH_HIP(hipDeviceSynchronize());      // (the queue's memory is reused)
            SH_HIP(hipMemset(d_q, 0, q_bytes));
            LongCoop Q{};
            size_t qo = 0;
            Q.items = (uint4 *)(d_q + qo); qo += 16 * cap;
            Q.ready = (uint32_t *)(d_q + qo); qo += (4 * cap + 63) & ~(size_t)63;
            Q.q_res = (uint32_t *)(d_q + qo); Q.q_head = Q.q_res + 1; Q.active = Q.q_res + 2; Q.n_reads = Q.q_res + 3; qo += 64;
            Q.desc = (LongCoopDesc *)(d_q + qo);
            Q.cap = (uint32_t)kv.first[1];
            B.coop = Q;
            DBGL_TRY(launch(kv.first[0] == 1024 ? 3 : 4, kv.second));
        }
        SH_HIP(hipDeviceSynchronize());
        SH_HIP(hipMemcpy(out, d_out, sizeof(sh_dbg_long_result) * (size_t)n_cases, hipMemcpyDeviceToHost));
        back.resize((size_t)bytes);
        SH_HIP(hipMemcpy(back.data(), d_mem, (size_t)bytes, hipMemcpyDeviceToHost));
        return SH_OK;
    };
    const sh_status st = run();
    hipFree(d_mem); hipFree(d_q); hipFree(d_a); hipFree(d_jobs); hipFree(d_order); hipFree(d_out); hipFree(d_fin); hipFree(d_pin); hipFree(d_cuts);
    if (st != SH_OK) return st;
    for (int32_t i = 0; i < n_cases; ++i) {
        const DbgLongJob &J = jobs[(size_t)i]; const Lay &Y = lay[(size_t)i];
        const size_t nn = (size_t)J.c.n;
        memcpy(f + J.o, back.data() + Y.f.at, 4 * nn); memcpy(p + J.o, back.data() + Y.p.at, 4 * nn);
        memcpy(t + J.o, back.data() + Y.t.at, 4 * nn); memcpy(v + J.o, back.data() + Y.v.at, 4 * nn);
        memset(u + J.o, 0, 8 * nn);
        memcpy(u + J.o, back.data() + Y.u.at, (size_t)Y.u.bytes);
        const Span *sp[11] = {&Y.f, &Y.p, &Y.t, &Y.v, &Y.u, &Y.pri, &Y.bmin, &Y.sk, &Y.sk2, &Y.rq0, &Y.rq1};
        uint64_t changed = 0;
        unsigned long long g0 = Y.lo;
        for (int s = 0; s <= 11; ++s) {      // the bands: before the first array, between two arrays, behind the last
            const unsigned long long g1 = s < 11 ? sp[s]->at : Y.hi;
            for (unsigned long long b = g0; b < g1; ++b) changed += back[(size_t)b] != DBGL_GUARD_BYTE;
            if (s < 11) g0 = sp[s]->at + sp[s]->bytes;
        }
        out[i].guard = changed;
    }
    return SH_OK;
}

// ---- lr_sort alone: one wave per case over n distinct (k, v) pairs, payload i = the pair's place in the case ----
struct DbgLrSortBufs { const sh_dbg_lr_sort_case *cases; SKey *a, *tmp; };

__global__ void __launch_bounds__(64) k_dbg_lr_sort(DbgLrSortBufs B)
{
    const sh_dbg_lr_sort_case c = B.cases[blockIdx.x];
    lr_sort(B.a + c.off, B.tmp + c.off, c.n);
}

extern "C" sh_status sh_dbg_lr_sort(int32_t device, const uint64_t *k, const uint64_t *v, const sh_dbg_lr_sort_case *cases, int32_t n_cases,
                                    uint64_t *out_k, uint64_t *out_v, uint32_t *out_i)
{
    SH_CHECK(k && v && cases && out_k && out_v && out_i && n_cases > 0 && n_cases <= DBGL_MAX_CASES, SH_ERR_BAD_ARG, "sh_dbg_lr_sort: bad argument");
    uint64_t n_total = 1;      // the arrays reach as far as the cases say
    for (int32_t i = 0; i < n_cases; ++i) {
        SH_CHECK(cases[i].n >= 0 && cases[i].n <= DBGL_MAX_N && cases[i].off <= (1ull << 32), SH_ERR_BAD_ARG, "sh_dbg_lr_sort: case %d: %d pairs at %llu", i, cases[i].n, (unsigned long long)cases[i].off);
        if (cases[i].off + (uint64_t)cases[i].n > n_total) n_total = cases[i].off + (uint64_t)cases[i].n;
    }
    std::vector<SKey> keys((size_t)n_total);
    for (uint64_t i = 0; i < n_total; ++i) { keys[(size_t)i].k = k[i]; keys[(size_t)i].v = v[i]; keys[(size_t)i].i = ~0u; keys[(size_t)i].pad = 0; }
    for (int32_t i = 0; i < n_cases; ++i) {
        const sh_dbg_lr_sort_case &c = cases[i];
        for (int32_t j = 0; j < c.n; ++j) keys[(size_t)c.off + (size_t)j].i = (uint32_t)j;
    }
    SH_HIP(hipSetDevice(device));
    SKey *d_a = nullptr, *d_tmp = nullptr; sh_dbg_lr_sort_case *d_cases = nullptr;
    auto run = [&]() -> sh_status {
        const size_t nt = (size_t)n_total;
        SH_HIP(hipMalloc(&d_a, sizeof(SKey) * nt)); SH_HIP(hipMalloc(&d_tmp, sizeof(SKey) * nt)); SH_HIP(hipMalloc(&d_cases, sizeof(sh_dbg_lr_sort_case) * (size_t)n_cases));
        SH_HIP(hipMemcpy(d_a, keys.data(), sizeof(SKey) * nt, hipMemcpyHostToDevice)); SH_HIP(hipMemset(d_tmp, 0, sizeof(SKey) * nt));
        SH_HIP(hipMemcpy(d_cases, cases, sizeof(sh_dbg_lr_sort_case) * (size_t)n_cases, hipMemcpyHostToDevice));
        DbgLrSortBufs B{d_cases, d_a, d_tmp};
        hipLaunchKernelGGL(k_dbg_lr_sort, dim3((uint32_t)n_cases), dim3(64), 0, 0, B);
        SH_HIP(hipGetLastError());
        SH_HIP(hipDeviceSynchronize());
        SH_HIP(hipMemcpy(keys.data(), d_a, sizeof(SKey) * nt, hipMemcpyDeviceToHost));
        return SH_OK;
    };
    const sh_status st = run();
    hipFree(d_a); hipFree(d_tmp); hipFree(d_cases);
    if (st != SH_OK) return st;
    for (uint64_t i = 0; i < n_total; ++i) { out_k[i] = keys[(size_t)i].k; out_v[i] = keys[(size_t)i].v; out_i[i] = keys[(size_t)i].i; }
    return SH_OK;
}
