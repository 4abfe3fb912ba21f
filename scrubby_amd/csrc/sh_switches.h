// sh_switches.h — the SCRUBBY_HIP_* environment switches of the classify path (sh_classify.hip), each name once.  Host only: no HIP.
//   context group: read once by sh_ctx_create and baked into ChainParams, LongParams and the buffer sizes.  Whoever keeps a context for a later
//                  call (the pool of sh_classify_batch, the cache of sh_reads_run) keys it on shi_switches_sig().
//   call group:    read once by every sh_classify_device call, before its first chunk; may change between two calls on one context.
#pragma once
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>

// bits of K3Args::dbg (K2Args::dbg: DBG_STATS only) = CallSwitches::dbg: the value of SCRUBBY_HIP_DBG with the behaviour switches below folded in
enum : int32_t {
    DBG_NO_CHAIN_LDS = 1,          // k_sort_lds does not chain    } timing A/Bs, the answers are then wrong: SCRUBBY_HIP_DBG bits that
    DBG_NO_CHAIN_GIANT = 2,        // k_giant_chain does not chain } only count together with SCRUBBY_HIP_AB_NOCHAIN
    DBG_STATS = 16,                // the kernels count what the [dbg] statistics lines print
    DBG_NO_CLUSTER_DP = 32,        // k_cluster_dp is not launched
    DBG_NO_GROUP_PROBE = 64,       // k_group_probe is not launched, k_sort_lds tries no group first
    DBG_NO_PARFILL = 128,          // = SCRUBBY_HIP_NO_PARFILL
    DBG_NO_LOCAL_CLUSTER = 256,    // k_local_cluster is not launched
    DBG_NO_TOPBT = 512,            // = SCRUBBY_HIP_NO_TOPBT
    DBG_LOCUS_TOP1 = 1024,         // = SCRUBBY_HIP_LOCUS_TOP1
};

constexpr int64_t SW_UNSET = INT64_MIN;      // default of a switch whose absence means "what the code works out"
constexpr int64_t SW_TOPBT_MAX = 64, SW_COOP_MIN = 12288, SW_COOP_RUN = 3072;      // TOPBT_MAX (sh_chain.h), LR_COOP_MIN / _RUN (sh_long.h): sh_classify.hip asserts it

struct CtxSwitches {
    int64_t arena_bytes, ext_bytes, ext_reg_cap, lext_a, lext_big_a, lext_p_bytes, lext_big_p_bytes, stage_bytes, streams;
    int64_t no_flag_stop, no_pair, pair_min_anchors, no_s1, no_lemma;
    int64_t rmq_exact_max, rmq_one_lane, e2_join_min, coop_min, coop_run, coop_check;
};
struct CallSwitches {
    // SCRUBBY_HIP_DBG is tested in two ways, kept apart: dbg_set (set to any value, "0" too) prints the [dbg] summary lines and starts the wave
    // clocks; bit DBG_STATS of dbg makes the kernels count and prints the statistics lines
    int64_t dbg, dbg_set, dbg_exact, ab_nochain, no_parfill, no_topbt, locus_top1;
    int64_t giant_fanin;      // 2 or 4; 0: the variable holds something else
    int64_t pft_gmin, top_max, no_locus, no_probe, no_cl_lds, giant_bins_down, giant_waves;
    int64_t side_pick;        // g | f << 8, or -1
    int64_t side, k2_late, no_coop, giants_plain, no_follow;
};

// type: P present (1 when set to anything), I int, M MiB and K KiB (held in bytes), 2 the pair "g,f" of side streams 0..2.  A value that is set is
// clamped to lo..hi; one that is not is `def`.
template <class S> struct SwDef { const char *name; char type; int64_t def, lo, hi; int64_t S::*field; };
#define SW_ANY INT64_MIN, INT64_MAX
static const SwDef<CtxSwitches> SW_CTX[] = {
    {"SCRUBBY_HIP_ARENA_MB", 'M', SW_UNSET, SW_ANY, &CtxSwitches::arena_bytes},                // the chain arena (default: 4 KiB per read, 4 GiB at least)
    {"SCRUBBY_HIP_EXT_MB", 'M', SW_UNSET, SW_ANY, &CtxSwitches::ext_bytes},                    // extension stage: the chain hand-over buffers (tests: SH_SPLIT)
    {"SCRUBBY_HIP_EXT_REGCAP", 'I', 16384, 65, INT64_MAX, &CtxSwitches::ext_reg_cap},          // tests: chains of a read the full procedure takes
    {"SCRUBBY_HIP_LEXT_A", 'I', SW_UNSET, 64, INT64_MAX, &CtxSwitches::lext_a},                // tests: chain anchors of the first working-memory size
    {"SCRUBBY_HIP_LEXT_BIG_A", 'I', SW_UNSET, 1024, INT64_MAX, &CtxSwitches::lext_big_a},      // tests: reads beyond the second size
    {"SCRUBBY_HIP_LEXT_P_KB", 'K', SW_UNSET, SW_ANY, &CtxSwitches::lext_p_bytes},              // tests: direction bytes of the first size
    {"SCRUBBY_HIP_LEXT_BIG_P_KB", 'K', SW_UNSET, SW_ANY, &CtxSwitches::lext_big_p_bytes},      // tests: alignments beyond the second size
    {"SCRUBBY_HIP_STAGE_MB", 'M', SW_UNSET, SW_ANY, &CtxSwitches::stage_bytes},                // tests: raw anchors waiting for k_lr_locus
    {"SCRUBBY_HIP_STREAMS", 'I', 1, SW_ANY, &CtxSwitches::streams},                            // bit 0: K2 on a side stream (0: on the main stream)
    {"SCRUBBY_HIP_NO_FLAG_STOP", 'P', 0, SW_ANY, &CtxSwitches::no_flag_stop},                  // A/B: the DP does not stop at the first chain that decides
    {"SCRUBBY_HIP_NO_PAIR", 'P', 0, SW_ANY, &CtxSwitches::no_pair},                            // A/B: no pair test (ChainParams::pair_dq_*)
    {"SCRUBBY_HIP_PAIR_MIN", 'I', 32, SW_ANY, &CtxSwitches::pair_min_anchors},                 // k_expand's pair test: reads of more anchors than this
    {"SCRUBBY_HIP_NO_S1", 'P', 0, SW_ANY, &CtxSwitches::no_s1},                                // A/B: no k_pair_pass mode 2 (ChainParams::ext_s1)
    {"SCRUBBY_HIP_NO_LEMMA", 'P', 0, SW_ANY, &CtxSwitches::no_lemma},                          // A/B: no ChainParams::ext_lemma
    {"SCRUBBY_HIP_RMQ_EXACT_MAX", 'I', -1, SW_ANY, &CtxSwitches::rmq_exact_max},               // long join: chain anchors a read may take to the literal tree (-1 every read, 0 none)
    {"SCRUBBY_HIP_RMQ_ONE_LANE", 'I', 0, SW_ANY, &CtxSwitches::rmq_one_lane},                  // not 0: reads beyond the 4096-anchor ring are chained by the one-lane trees
    {"SCRUBBY_HIP_E2_JOIN_MIN", 'I', INT32_MAX, SW_ANY, &CtxSwitches::e2_join_min},            // exact passes: joins of more anchors go to the 4096-anchor ring
    {"SCRUBBY_HIP_COOP_MIN", 'I', SW_COOP_MIN, 1, INT64_MAX, &CtxSwitches::coop_min},          // lr_coop_fill: reads with fewer anchors in the join stay with their wave
    {"SCRUBBY_HIP_COOP_RUN", 'I', SW_COOP_RUN, 2, INT64_MAX, &CtxSwitches::coop_run},          // lr_coop_fill: anchors of a shared stretch, at least
    {"SCRUBBY_HIP_COOP_CHECK", 'P', 0, SW_ANY, &CtxSwitches::coop_check},                      // debugging: lr_coop_fill joins once more in one piece and compares
};
static const SwDef<CallSwitches> SW_CALL[] = {
    {"SCRUBBY_HIP_DBG", 'I', SW_UNSET, SW_ANY, &CallSwitches::dbg},                            // [dbg] lines on stderr; bit mask, see the enum above
    {"SCRUBBY_HIP_DBG_EXACT", 'P', 0, SW_ANY, &CallSwitches::dbg_exact},                       // with _DBG: one line per read of the exact passes
    {"SCRUBBY_HIP_AB_NOCHAIN", 'P', 0, SW_ANY, &CallSwitches::ab_nochain},                     // lets bits 1 and 2 of _DBG through
    {"SCRUBBY_HIP_NO_PARFILL", 'P', 0, SW_ANY, &CallSwitches::no_parfill},                     // A/B: every cluster chained by the sequential DP
    {"SCRUBBY_HIP_NO_TOPBT", 'P', 0, SW_ANY, &CallSwitches::no_topbt},                         // A/B: clusters visited one by one even when the read's DP is done
    {"SCRUBBY_HIP_LOCUS_TOP1", 'P', 0, SW_ANY, &CallSwitches::locus_top1},                     // tests: k_lr_locus keeps the largest run of windows only
    {"SCRUBBY_HIP_GIANT_FANIN", 'I', 4, SW_ANY, &CallSwitches::giant_fanin},                   // A/B and tests: runs a giant-read merge pass merges, 4 or 2
    {"SCRUBBY_HIP_PFT_GMIN", 'I', 32768, 1, INT64_MAX, &CallSwitches::pft_gmin},               // tests: par_fill_tiled gives reads of this many anchors eight lanes per anchor
    {"SCRUBBY_HIP_TOPBT_MAX", 'I', SW_TOPBT_MAX, 1, SW_TOPBT_MAX, &CallSwitches::top_max},     // tests: candidates a read may have at its top score
    {"SCRUBBY_HIP_NO_LOCUS", 'P', 0, SW_ANY, &CallSwitches::no_locus},                         // A/B: k_lr_locus thins out no read
    {"SCRUBBY_HIP_NO_PROBE", 'P', 0, SW_ANY, &CallSwitches::no_probe},                         // A/B: no alignment probe (and so no k_lr_locus)
    {"SCRUBBY_HIP_NO_CL_LDS", 'P', 0, SW_ANY, &CallSwitches::no_cl_lds},                       // A/B: the LDS classes feed k_cluster_dp's queue no clusters
    {"SCRUBBY_HIP_GIANT_BINS_DOWN", 'I', 0, SW_ANY, &CallSwitches::giant_bins_down},           // A/B: size bins more that go to the giants' launch
    {"SCRUBBY_HIP_GIANT_WAVES", 'I', SW_UNSET, 1, INT64_MAX, &CallSwitches::giant_waves},      // A/B: waves of the giants' launch (default 64)
    {"SCRUBBY_HIP_SIDE_PICK", '2', -1, SW_ANY, &CallSwitches::side_pick},                      // pins the side streams of the giants' launch and the follower, no probe
    {"SCRUBBY_HIP_SIDE", 'I', -1, SW_ANY, &CallSwitches::side},                                // 1 / 0: the sort classes side by side, or nothing of them beside the caller's stream; 2: only the leftover k_sort_lds kernels aside (default: by chunk size, 1 or 2)
    {"SCRUBBY_HIP_K2_LATE", 'I', -1, SW_ANY, &CallSwitches::k2_late},                          // 1: K2 starts beside the second pass's giant kernels
    {"SCRUBBY_HIP_NO_COOP", 'P', 0, SW_ANY, &CallSwitches::no_coop},                           // A/B: no long join shared among waves (lr_coop_fill)
    {"SCRUBBY_HIP_GIANTS_PLAIN", 'P', 0, SW_ANY, &CallSwitches::giants_plain},                 // A/B: the giants on the plain instance of the chains kernel, and no lr_coop_fill
    {"SCRUBBY_HIP_NO_FOLLOW", 'P', 0, SW_ANY, &CallSwitches::no_follow},                       // A/B: the regions kernel's second size after the first, not beside it
};
#undef SW_ANY

template <class S, size_t N> inline S sw_read(const SwDef<S> (&defs)[N])
{
    S s{};
    for (const SwDef<S> &d : defs) {
        const char *e = getenv(d.name);
        int64_t v = d.def;
        int g = 0, f = 0;
        if (e && d.type == 'P') v = 1;
        else if (e && d.type == 'I') v = atoi(e);
        else if (e && d.type == 'M') v = (int64_t)((uint64_t)atoll(e) << 20);
        else if (e && d.type == 'K') v = (int64_t)((uint64_t)atoll(e) << 10);
        else if (e && sscanf(e, "%d,%d", &g, &f) == 2 && g >= 0 && g < 3 && f >= 0 && f < 3) v = g | f << 8;
        s.*d.field = e ? (v < d.lo ? d.lo : v > d.hi ? d.hi : v) : v;
    }
    return s;
}
inline CtxSwitches shi_ctx_switches() { return sw_read(SW_CTX); }
inline CallSwitches shi_call_switches()
{
    CallSwitches c = sw_read(SW_CALL);
    c.dbg_set = c.dbg != SW_UNSET;
    if (!c.dbg_set) c.dbg = 0;
    if (!c.ab_nochain) c.dbg &= ~(int64_t)(DBG_NO_CHAIN_LDS | DBG_NO_CHAIN_GIANT);
    if (c.no_parfill) c.dbg |= DBG_NO_PARFILL;
    if (c.no_topbt) c.dbg |= DBG_NO_TOPBT;
    if (c.locus_top1) c.dbg |= DBG_LOCUS_TOP1;
    if (c.giant_fanin != 2 && c.giant_fanin != 4) c.giant_fanin = 0;
    return c;
}
// the text a switch is set to (an error message quotes it), "" when it is not
inline const char *shi_call_switch_text(int64_t CallSwitches::*field)
{
    for (const auto &d : SW_CALL) if (d.field == field && getenv(d.name)) return getenv(d.name);
    return "";
}
// the raw values of the context group: contexts built under equal signatures (and equal sh_opts) are interchangeable
inline std::string shi_switches_sig()
{
    std::string sig;
    for (const auto &d : SW_CTX) { const char *e = getenv(d.name); sig += e ? e : "-"; sig += '|'; }
    return sig;
}
