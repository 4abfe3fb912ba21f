// The classify path's switch list on the host (scrubby_amd/csrc/sh_switches.h): defaults, clamps, the dbg folding and the context signature,
// driven by setting one variable at a time.  swh_case(i) returns 0, or the line of the first check that failed.
// With -DSWITCHES_MAIN the file is a program of its own that runs every case (the sanitizer build).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <iterator>
#include <string>
#include <utility>
#include <vector>
#include "../scrubby_amd/csrc/sh_switches.h"

#define CHECK(cond) do { if (!(cond)) return __LINE__; } while (0)

struct CleanEnv {      // none of the list's variables set for the length of a scope; the caller's values come back after it
    std::vector<std::pair<const char *, std::string>> was;
    template <class D> void take(const D &defs) { for (const auto &d : defs) { if (const char *e = getenv(d.name)) was.push_back({d.name, e}); unsetenv(d.name); } }
    CleanEnv() { take(SW_CTX); take(SW_CALL); }
    ~CleanEnv() { for (const auto &w : was) setenv(w.first, w.second.c_str(), 1); }
};
struct With {      // one variable set for the length of a scope
    const char *name;
    With(const char *n, const char *v) : name(n) { setenv(n, v, 1); }
    ~With() { unsetenv(name); }
};

static int case_defaults()
{
    const CtxSwitches x = shi_ctx_switches();
    const CallSwitches c = shi_call_switches();
    CHECK(x.pair_min_anchors == 32 && x.rmq_exact_max == -1 && x.e2_join_min == INT32_MAX && x.coop_min == 12288 && x.coop_run == 3072 && x.rmq_one_lane == 0);
    CHECK(x.ext_reg_cap == 16384 && x.streams == 1 && !x.no_flag_stop && !x.no_pair && !x.no_s1 && !x.no_lemma && !x.coop_check);
    CHECK(x.arena_bytes == SW_UNSET && x.ext_bytes == SW_UNSET && x.stage_bytes == SW_UNSET && x.lext_a == SW_UNSET && x.lext_big_a == SW_UNSET && x.lext_p_bytes == SW_UNSET && x.lext_big_p_bytes == SW_UNSET);
    CHECK(c.giant_fanin == 4 && c.pft_gmin == 32768 && c.top_max == SW_TOPBT_MAX && SW_TOPBT_MAX == 64 && c.side == -1 && c.k2_late == -1 && c.side_pick == -1);
    CHECK(c.dbg == 0 && !c.dbg_set && !c.dbg_exact && c.giant_bins_down == 0 && c.giant_waves == SW_UNSET);
    CHECK(!c.no_locus && !c.no_probe && !c.no_cl_lds && !c.no_coop && !c.giants_plain && !c.no_follow);
    return 0;
}

static int case_values_and_clamps()
{
    { With w("SCRUBBY_HIP_COOP_RUN", "1"); CHECK(shi_ctx_switches().coop_run == 2); }
    { With w("SCRUBBY_HIP_COOP_RUN", "500"); CHECK(shi_ctx_switches().coop_run == 500); }
    { With w("SCRUBBY_HIP_COOP_MIN", "0"); CHECK(shi_ctx_switches().coop_min == 1); }
    { With w("SCRUBBY_HIP_EXT_REGCAP", "3"); CHECK(shi_ctx_switches().ext_reg_cap == 65); }
    { With w("SCRUBBY_HIP_LEXT_A", "3"); CHECK(shi_ctx_switches().lext_a == 64); }
    { With w("SCRUBBY_HIP_LEXT_BIG_A", "3"); CHECK(shi_ctx_switches().lext_big_a == 1024); }
    { With w("SCRUBBY_HIP_TOPBT_MAX", "0"); CHECK(shi_call_switches().top_max == 1); }
    { With w("SCRUBBY_HIP_TOPBT_MAX", "1000"); CHECK(shi_call_switches().top_max == SW_TOPBT_MAX); }
    { With w("SCRUBBY_HIP_TOPBT_MAX", "2"); CHECK(shi_call_switches().top_max == 2); }
    { With w("SCRUBBY_HIP_PFT_GMIN", "-5"); CHECK(shi_call_switches().pft_gmin == 1); }
    { With w("SCRUBBY_HIP_GIANT_WAVES", "0"); CHECK(shi_call_switches().giant_waves == 1); }
    { With w("SCRUBBY_HIP_ARENA_MB", "3"); CHECK(shi_ctx_switches().arena_bytes == 3ll << 20); }
    { With w("SCRUBBY_HIP_LEXT_P_KB", "3"); CHECK(shi_ctx_switches().lext_p_bytes == 3ll << 10); }
    { With w("SCRUBBY_HIP_RMQ_EXACT_MAX", "0"); CHECK(shi_ctx_switches().rmq_exact_max == 0); }
    { With w("SCRUBBY_HIP_STREAMS", "0"); CHECK(shi_ctx_switches().streams == 0); }
    { With w("SCRUBBY_HIP_NO_PAIR", ""); CHECK(shi_ctx_switches().no_pair == 1); }      // present is enough
    { With w("SCRUBBY_HIP_SIDE", "0"); CHECK(shi_call_switches().side == 0); }
    { With w("SCRUBBY_HIP_SIDE_PICK", "2,0"); CHECK(shi_call_switches().side_pick == 2); }
    { With w("SCRUBBY_HIP_SIDE_PICK", "1,2"); CHECK(shi_call_switches().side_pick == (1 | 2 << 8)); }
    { With w("SCRUBBY_HIP_SIDE_PICK", "1,3"); CHECK(shi_call_switches().side_pick == -1); }
    { With w("SCRUBBY_HIP_SIDE_PICK", "1"); CHECK(shi_call_switches().side_pick == -1); }
    return 0;
}

static int case_giant_fanin()
{
    { With w("SCRUBBY_HIP_GIANT_FANIN", "2"); CHECK(shi_call_switches().giant_fanin == 2); }
    { With w("SCRUBBY_HIP_GIANT_FANIN", "4"); CHECK(shi_call_switches().giant_fanin == 4); }
    { With w("SCRUBBY_HIP_GIANT_FANIN", "3"); CHECK(shi_call_switches().giant_fanin == 0 && std::string(shi_call_switch_text(&CallSwitches::giant_fanin)) == "3"); }
    { With w("SCRUBBY_HIP_GIANT_FANIN", "x"); CHECK(shi_call_switches().giant_fanin == 0); }
    CHECK(std::string(shi_call_switch_text(&CallSwitches::giant_fanin)).empty());
    return 0;
}

static int case_signature()
{
    const std::string base = shi_switches_sig();
    for (const auto &d : SW_CTX) {
        { With w(d.name, "7"); CHECK(shi_switches_sig() != base); }
        { With w(d.name, ""); CHECK(shi_switches_sig() != base); }
    }
    for (const auto &d : SW_CALL) { With w(d.name, "7"); CHECK(shi_switches_sig() == base); }
    { With a("SCRUBBY_HIP_LEXT_A", "7"); const std::string s1 = shi_switches_sig(); unsetenv(a.name); With b("SCRUBBY_HIP_LEXT_BIG_A", "7"); CHECK(shi_switches_sig() != s1); }      // which name holds the value counts
    CHECK(shi_switches_sig() == base);
    return 0;
}

static int case_dbg()
{
    { With w("SCRUBBY_HIP_DBG", "0"); const CallSwitches c = shi_call_switches(); CHECK(c.dbg_set == 1 && c.dbg == 0 && !(c.dbg & DBG_STATS)); }
    { With w("SCRUBBY_HIP_DBG", "16"); const CallSwitches c = shi_call_switches(); CHECK(c.dbg_set == 1 && c.dbg == DBG_STATS); }
    { With w("SCRUBBY_HIP_DBG", "19"); const CallSwitches c = shi_call_switches(); CHECK(c.dbg == DBG_STATS); }      // bits 1 and 2 need the second switch
    { With w("SCRUBBY_HIP_DBG", "19"); With v("SCRUBBY_HIP_AB_NOCHAIN", "1"); CHECK(shi_call_switches().dbg == (DBG_STATS | DBG_NO_CHAIN_LDS | DBG_NO_CHAIN_GIANT)); }
    { With w("SCRUBBY_HIP_DBG", "352"); CHECK(shi_call_switches().dbg == (DBG_NO_CLUSTER_DP | DBG_NO_GROUP_PROBE | DBG_NO_LOCAL_CLUSTER)); }
    { With w("SCRUBBY_HIP_NO_PARFILL", "1"); const CallSwitches c = shi_call_switches(); CHECK(c.dbg == DBG_NO_PARFILL && !c.dbg_set); }
    { With w("SCRUBBY_HIP_NO_TOPBT", "1"); CHECK(shi_call_switches().dbg == DBG_NO_TOPBT); }
    { With w("SCRUBBY_HIP_LOCUS_TOP1", "1"); CHECK(shi_call_switches().dbg == DBG_LOCUS_TOP1); }
    { With w("SCRUBBY_HIP_DBG_EXACT", "1"); const CallSwitches c = shi_call_switches(); CHECK(c.dbg_exact == 1 && !c.dbg_set); }
    CHECK(DBG_NO_CHAIN_LDS == 1 && DBG_NO_CHAIN_GIANT == 2 && DBG_STATS == 16 && DBG_NO_CLUSTER_DP == 32 && DBG_NO_GROUP_PROBE == 64 && DBG_NO_PARFILL == 128 &&
          DBG_NO_LOCAL_CLUSTER == 256 && DBG_NO_TOPBT == 512 && DBG_LOCUS_TOP1 == 1024);
    return 0;
}

static int (*const CASES[])() = {case_defaults, case_values_and_clamps, case_giant_fanin, case_signature, case_dbg};
extern "C" int swh_n_cases() { return (int)std::size(CASES); }
extern "C" int swh_case(int i) { const CleanEnv clean; return CASES[i](); }
// the list itself, for the checks of the sources: names of the context group first
extern "C" int swh_n_names(int call_group) { return call_group ? (int)std::size(SW_CALL) : (int)std::size(SW_CTX); }
extern "C" const char *swh_name(int call_group, int i) { return call_group ? SW_CALL[i].name : SW_CTX[i].name; }

#ifdef SWITCHES_MAIN
int main()
{
    int bad = 0;
    for (int i = 0; i < swh_n_cases(); ++i) if (const int rc = swh_case(i)) { printf("case %d: the check in line %d failed\n", i, rc); ++bad; }
    if (!bad) printf("%d cases ok\n", swh_n_cases());
    return bad != 0;
}
#endif
