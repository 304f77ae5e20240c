// Prints tim_amd/csrc/gemm_plan.h's and wgrad_plan.h's answers for the calls it reads from stdin, one per line
// (tests/test_gemm_plan.py, tests/test_wgrad_plan.py):
//   nt <precision> <epi> <M> <N> <K> <splitk> <a_wrap> [KNOB=value ...]    -> the GemmPlan of a tim_gemm_nt call
//   p8 <epi> <M> <N> <K> [KNOB=value ...]                                   -> what timhip_gemm_p8_choice answers
//   group <epi> <n> <M1> <N1> ... <Mn> <Nn> [KNOB=value ...]                -> the GemmGroupPlan of a tim_gemm_nt_group call
//   wgroup <M> <n> <N1> <K1> <ldy1> <ldx1> ... [KNOB=value ...]             -> the contract's answer and the WgradPlan of a
//                                                                              tim_wgrad_group_h16 call (16-byte aligned operands)
//   wtn <M> <N> <K>                                                         -> the WgradPlan of a tim_wgrad_tn_h16 call
// KNOB: a TIMHIP_* variable the plan reads, without the prefix; every other knob keeps TimKnobs' default.  wgroup also takes
// NULL_X=<item> (that item's X pointer is NULL), ODD_DW=<item> (its dW is 4 bytes off a 16-byte boundary) and FORCE_SPLITS=<sk>.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sstream>
#include <string>
#include <vector>

#include "gemm_plan.h"
#include "wgrad_plan.h"

static bool set_knob(TimKnobs& k, const std::string& name, int v) {
  struct { const char* name; int TimKnobs::*field; } const table[] = {
      {"GEMM_PP", &TimKnobs::gemm_pp}, {"GEMM_LD", &TimKnobs::gemm_ld}, {"GEMM_PF", &TimKnobs::gemm_pf},
      {"GEMM_PF_MODE", &TimKnobs::gemm_pf_mode}, {"GEMM_PF_MR", &TimKnobs::gemm_pf_mr}, {"GEMM_LDP", &TimKnobs::gemm_ldp},
      {"GEMM_P8_PH", &TimKnobs::gemm_p8_ph}, {"GEMM_SMALL_W8", &TimKnobs::gemm_small_w8}, {"GEMM_SMALL_NST", &TimKnobs::gemm_small_nst},
      {"GEMM_TMW", &TimKnobs::gemm_tmw}, {"GEMM_PP_MIN_TILES", &TimKnobs::gemm_pp_min}, {"GEMM_P8", &TimKnobs::gemm_p8},
      {"WGRAD_PP", &TimKnobs::wgrad_pp}, {"WGRAD_LD", &TimKnobs::wgrad_ld}, {"WGRAD_PF", &TimKnobs::wgrad_pf},
      {"WGRAD_P8_PH", &TimKnobs::wgrad_p8_ph}, {"WGRAD_P8", &TimKnobs::wgrad_p8}};
  for (const auto& t : table)
    if (name == t.name) { k.*(t.field) = v; return true; }
  return false;
}

static void print_wgrad_plan(const WgradPlan& p) {
  static const char* const family[] = {"split", "pp8w", "ld", "p8"};
  printf("family=%s tn=%d tk=%d tiles=%d splits=%d steps_per_split=%d phases=%d ragged=%d pf_dist=%d grid_x=%u block=%u lds=%u ws=%zu db_off=%zu tile0=",
         family[p.family], p.tn, p.tk, p.tiles, p.splits, p.steps_per_split, p.phases, p.ragged, p.pf_dist, p.grid_x, p.block, p.lds_bytes,
         p.ws_bytes, p.db_off);
  for (int i = 0; i <= WGRAD_MAX_ITEMS; ++i) printf("%s%d", i ? "," : "", p.tile0[i]);
  printf("\n");
}

int main() {
  static const char* const family[] = {"f32", "x3", "h16", "pp8w", "ld", "ldp", "p8"};
  alignas(16) static char operand[32];
  char buf[4096];
  while (fgets(buf, sizeof buf, stdin)) {
    std::istringstream in(buf);
    std::string cmd, tok;
    if (!(in >> cmd)) continue;
    std::vector<int> a;
    TimKnobs kn;
    int null_x = -1, odd_dw = -1, force_splits = 0;
    while (in >> tok) {
      const size_t eq = tok.find('=');
      if (eq == std::string::npos) { a.push_back(atoi(tok.c_str())); continue; }
      const std::string name = tok.substr(0, eq);
      const int v = atoi(tok.c_str() + eq + 1);
      if (name == "NULL_X") null_x = v;
      else if (name == "ODD_DW") odd_dw = v;
      else if (name == "FORCE_SPLITS") force_splits = v;
      else if (!set_knob(kn, name, v)) { fprintf(stderr, "unknown knob %s\n", tok.c_str()); return 2; }
    }
    if (cmd == "nt" && a.size() == 7) {
      const GemmPlan p = gemm_nt_plan(kn, a[0], a[1], a[2], a[3], (a[4] + 63) / 64 * 64, a[5], a[6]);
      printf("family=%s bm=%d bn=%d wm=%d wn=%d nst=%d tm=%d phases=%d tpb=%d pf_dist=%d pf_mode=%d ksteps=%d grid_x=%u grid_z=%u block=%u lds=%u\n",
             family[p.family], p.bm, p.bn, p.wm, p.wn, p.nst, p.tm, p.phases, p.tpb, p.pf_dist, p.pf_mode, p.ksteps, p.grid_x, p.grid_z,
             p.block, p.lds_bytes);
    } else if (cmd == "p8" && a.size() == 4) {
      printf("tm=%d\n", gemm_p8_tm(kn, a[0], a[1], a[2], a[3], 0));
    } else if (cmd == "group" && a.size() >= 2 && a.size() == 2 + 2 * (size_t)a[1]) {
      std::vector<TimGemmItem> items(a[1]);
      for (int i = 0; i < a[1]; ++i) { memset(&items[i], 0, sizeof(TimGemmItem)); items[i].M = a[2 + 2 * i]; items[i].N = a[3 + 2 * i]; }
      const GemmGroupPlan p = gemm_group_plan(kn, a[0], items.data(), a[1]);
      printf("bn=%d wm=%d wn=%d nst=%d tiles=%u block=%u lds=%u\n", p.bn, p.wm, p.wn, p.nst, p.tiles, p.block, p.lds_bytes);
    } else if (cmd == "wgroup" && a.size() >= 2 && a[1] >= 1 && a.size() == 2 + 4 * (size_t)a[1]) {
      std::vector<TimWgradItem> items(a[1]);
      for (int i = 0; i < a[1]; ++i) {
        float* dw = reinterpret_cast<float*>(operand + (i == odd_dw ? 4 : 0));
        items[i] = TimWgradItem{operand, i == null_x ? nullptr : operand, dw, nullptr, a[4 + 4 * i], a[5 + 4 * i], a[2 + 4 * i], a[3 + 4 * i]};
      }
      const int rc = wgrad_group_contract(items.data(), a[1], a[0]);
      printf("contract=%s ", rc == TIMHIP_OK ? "ok" : rc == TIMHIP_EINVAL ? "einval" : rc == TIMHIP_EALIGN ? "ealign" :
                             rc == TIMHIP_EUNSUPPORTED ? "eunsupported" : "other");
      print_wgrad_plan(wgrad_group_plan(kn, items.data(), a[1], a[0], force_splits));
    } else if (cmd == "wtn" && a.size() == 3) {
      print_wgrad_plan(wgrad_tn_plan(a[1], a[2], a[0], force_splits));
    } else {
      fprintf(stderr, "bad line: %s", buf);
      return 2;
    }
  }
  return 0;
}
