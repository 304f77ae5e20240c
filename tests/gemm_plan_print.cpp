// Prints tim_amd/csrc/gemm_plan.h's answers for the calls it reads from stdin, one per line (tests/test_gemm_plan.py):
//   nt <precision> <epi> <M> <N> <K> <splitk> <a_wrap> [KNOB=value ...]    -> the GemmPlan of a tim_gemm_nt call
//   p8 <epi> <M> <N> <K> [KNOB=value ...]                                   -> what timhip_gemm_p8_choice answers
//   group <epi> <n> <M1> <N1> ... <Mn> <Nn> [KNOB=value ...]                -> the GemmGroupPlan of a tim_gemm_nt_group call
// KNOB: a TIMHIP_* variable the plan reads, without the prefix; every other knob keeps TimKnobs' default.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sstream>
#include <string>
#include <vector>

#include "gemm_plan.h"

static bool set_knob(TimKnobs& k, const std::string& name, int v) {
  struct { const char* name; int TimKnobs::*field; } const table[] = {
      {"GEMM_PP", &TimKnobs::gemm_pp}, {"GEMM_LD", &TimKnobs::gemm_ld}, {"GEMM_PF", &TimKnobs::gemm_pf},
      {"GEMM_PF_MODE", &TimKnobs::gemm_pf_mode}, {"GEMM_PF_MR", &TimKnobs::gemm_pf_mr}, {"GEMM_LDP", &TimKnobs::gemm_ldp},
      {"GEMM_P8_PH", &TimKnobs::gemm_p8_ph}, {"GEMM_SMALL_W8", &TimKnobs::gemm_small_w8}, {"GEMM_SMALL_NST", &TimKnobs::gemm_small_nst},
      {"GEMM_TMW", &TimKnobs::gemm_tmw}, {"GEMM_PP_MIN_TILES", &TimKnobs::gemm_pp_min}, {"GEMM_P8", &TimKnobs::gemm_p8}};
  for (const auto& t : table)
    if (name == t.name) { k.*(t.field) = v; return true; }
  return false;
}

int main() {
  static const char* const family[] = {"f32", "x3", "h16", "pp8w", "ld", "ldp", "p8"};
  char buf[4096];
  while (fgets(buf, sizeof buf, stdin)) {
    std::istringstream in(buf);
    std::string cmd, tok;
    if (!(in >> cmd)) continue;
    std::vector<int> a;
    TimKnobs kn;
    while (in >> tok) {
      const size_t eq = tok.find('=');
      if (eq == std::string::npos) { a.push_back(atoi(tok.c_str())); continue; }
      if (!set_knob(kn, tok.substr(0, eq), atoi(tok.c_str() + eq + 1))) { fprintf(stderr, "unknown knob %s\n", tok.c_str()); return 2; }
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
    } else {
      fprintf(stderr, "bad line: %s", buf);
      return 2;
    }
  }
  return 0;
}
