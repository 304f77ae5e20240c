// Which weight-gradient (TN) kernel a group gets, and its launch geometry: the ONE statement of the routing rules (plain C++, no
// HIP, no environment: `g++ -std=c++17 -fsyntax-only` takes it alone, tests/test_wgrad_plan.py pins the routes without a GPU).
// wgrad.hip and wgrad_pp.hip ask for a plan and switch from it to the kernel; they decide nothing themselves.  The sizing calls
// (tim_wgrad_group_ws, tim_wgrad_tn_ws) and timhip_layer_wgrad_pair_wins read the same plan, so "wins", "runs" and "needs this
// much workspace" cannot disagree.  A TUNING=1 build puts its experiment arms IN FRONT of the plan (one #ifdef block per file).
#pragma once

#include <cstdint>
#include "../../include/timhip.h"
#include "tim_knobs.h"

constexpr int WGRAD_MAX_ITEMS = 8;   // products per group (the kernel-argument arrays)
constexpr int WT = 128, WM = 64, WG_LDS = 2 * 2 * WM * WT * 2;   // wgrad.hip: 128 (n) x 128 (k) tile, 64 rows per step, two stages of (dY | X)
constexpr int WP_TN = 128, WP_TK = 256, WP_M = 64, WP_NST = 3;   // wgrad_pp.hip, 8- / 12-wave kernels: 128 (n) x 256 (k), 64 rows per stage, 3-stage ring
constexpr int WP_SUB = WP_M * 256;            // bytes of one [64][128] 16-bit sub-tile (256-byte rows)
constexpr int WP_STAGE = 3 * WP_SUB;          // dY | X[:, 0:128] | X[:, 128:256]
constexpr int W8_T = 256, W8_SUB = WP_M * 256, W8_STAGE = 4 * W8_SUB;   // its eight-phase kernel: 256 x 256, two stages of four sub-tiles

enum WgradFamily {
  WGRAD_SPLIT,   // wgrad.hip     wgrad_group_kernel (+ wgrad_group_reduce_kernel when it splits); wgrad_tn_kernel for one product
  WGRAD_PP8W,    // wgrad_pp.hip  wgrad_pp_kernel: one 8-wave block per CU (the fallback of the loader-wave kernel)
  WGRAD_LD,      // wgrad_pp.hip  wgrad_ld_kernel: 8 MFMA waves + 4 loader waves
  WGRAD_P8       // wgrad_pp.hip  wgrad_p8_kernel: eight-phase schedule, two layers per launch
};

struct WgradPlan {
  int family, tn, tk;                    // WgradFamily; output tile (n x k)
  int tile0[WGRAD_MAX_ITEMS + 1], tiles; // first tile of every item (prefix sums); tile0[WGRAD_MAX_ITEMS] = tiles
  int splits, steps_per_split;           // of the contraction, in 64-row steps; splits: the effective count (no empty splits)
  int phases, ragged;                    // eight-phase kernel: phases per step (2 / 4), M % 64 != 0; else 0
  int pf_dist;                           // WpGroup.pf_dist: L2 prefetch distance of the loader-wave kernel in stages (0: off)
  unsigned grid_x, block, lds_bytes;     // the launch (lds_bytes: dynamic LDS)
  // Workspace [slab: sk x sum N K fp32][bias slab at db_off: sk x sum N fp32], sk the split count the cost model ASKS for.
  // Kept as it always was reported (api.hip's ws_layout and the hosts' arenas hold these numbers): sized by sk although the
  // launch uses `splits` <= sk slabs; the bias slab counts every item's Nout, with a bias or not; and a group is priced as the
  // split kernel would run it whichever family takes it - a tiled family needs none, the launcher asks only when splits > 1.
  size_t ws_bytes, db_off;
};

// The argument contract of a group (include/timhip.h), the same whichever kernel runs it and checked before any launch: a
// group is refused as a whole, no item of it is written.
static inline int wgrad_group_contract(const TimWgradItem* it, int n, int M) {
  if (!it || n < 1 || n > WGRAD_MAX_ITEMS || M <= 0) return TIMHIP_EINVAL;
  for (int i = 0; i < n; ++i) {
    const TimWgradItem& t = it[i];
    if (!t.dY || !t.X || !t.dW || t.Nout <= 0 || t.Kout <= 0) return TIMHIP_EINVAL;
    if ((t.ldy % 8) || (t.ldx % 8) || (((uintptr_t)t.dY | (uintptr_t)t.X | (uintptr_t)t.dW) & 15)) return TIMHIP_EALIGN;
    if (((long long)t.Nout * t.Kout) & 3) return TIMHIP_EUNSUPPORTED;
  }
  return TIMHIP_OK;
}

// Number of splits of the contraction (token) dimension.  Work items = tiles x splits run two per CU (512 slots).
// Cost model in units of one 64-row K-step of one block, fitted to tools/wgrad_splits.py on the C2a shapes:
//   steps per item x (full rounds + a partial round priced at 0.5 + 0.5 x its fill) + slab traffic per split
// e.g. in-proj (192 tiles): 3 splits = 576 items (1.125 rounds) 108 us, 5 splits = 960 items 100 us.
// force_splits: TIMHIP_WGRAD_SPLITS of a TUNING=1 build (read by wgrad.hip), taken when the contraction has that many steps.
static inline int wgrad_splits_for_tiles(int tiles, int M, int force_splits) {
  const int nsteps = (M + WM - 1) / WM;
  if (force_splits >= 1 && force_splits <= nsteps) return force_splits;
  int maxsk = nsteps / 4;
  if (maxsk > 16) maxsk = 16;
  if (maxsk < 1) maxsk = 1;
  int best = 1;
  float best_cost = 0.f;
  for (int sk = 1; sk <= maxsk; ++sk) {
    const float per = (float)((nsteps + sk - 1) / sk);
    const float r = (float)tiles * sk / 512.f;
    const float full = __builtin_floorf(r), frac = r - full;
    const float cost = per * (full + (frac > 0.f ? 0.5f + 0.5f * frac : 0.f)) + 1.5f * (float)tiles / 128.f * sk;
    if (sk == 1 || cost < best_cost) { best = sk; best_cost = cost; }
  }
  return best;
}

// the split kernels' part of a plan: `tiles` 128 x 128 tiles x the effective splits of sk, and the slabs of sk
static inline void wgrad_split_geometry(WgradPlan& p, int tiles, int M, int sk, size_t elems, size_t bias) {
  const int nsteps = (M + WM - 1) / WM;
  p.family = WGRAD_SPLIT; p.tn = p.tk = WT; p.tiles = tiles;
  p.steps_per_split = (nsteps + sk - 1) / sk;
  p.splits = p.steps_per_split > 0 ? (nsteps + p.steps_per_split - 1) / p.steps_per_split : 1;   // no empty splits
  p.grid_x = (unsigned)(tiles * p.splits); p.block = 256; p.lds_bytes = WG_LDS;
  p.db_off = ((size_t)sk * elems * 4 + 255) / 256 * 256;
  p.ws_bytes = p.db_off + ((size_t)sk * bias * 4 + 255) / 256 * 256;
}

// One product (tim_wgrad_tn_h16): always through the slabs and the reduce kernel, also with one split.
static inline WgradPlan wgrad_tn_plan(int Nout, int Kout, int M, int force_splits = 0) {
  WgradPlan p{};
  const int tiles = ((Nout + WT - 1) / WT) * ((Kout + WT - 1) / WT);
  wgrad_split_geometry(p, tiles, M, wgrad_splits_for_tiles(tiles, M, force_splits), (size_t)Nout * Kout, (size_t)Nout);
  return p;
}

// A group of n products that share the contraction length M.  `it` is not NULL; the plan of a group the contract refuses
// (n > WGRAD_MAX_ITEMS among them) is the split family's and only its ws_bytes means anything.
static inline WgradPlan wgrad_group_plan(const TimKnobs& kn, const TimWgradItem* it, int n, int M, int force_splits = 0) {
  long long t128 = 0, tpp = 0, t8 = 0;
  size_t elems = 0, bias = 0;
  // The tiled grids run the whole contraction in every block (no split), one block per CU, and address their operands with
  // 32-bit byte offsets (M * ld * 2 < 2^32): a group beyond that runs on the plain tiles, which have no such limit.
  bool tiled = n >= 1 && n <= WGRAD_MAX_ITEMS && M >= 2048, pp_ok = true, p8_ok = true;
  for (int i = 0; i < n; ++i) {
    const long long N = it[i].Nout, K = it[i].Kout;
    if ((unsigned long long)M * it[i].ldy * 2 >= (1ull << 32) || (unsigned long long)M * it[i].ldx * 2 >= (1ull << 32)) tiled = false;
    if (N < 64 || K < 128) pp_ok = false;
    if (N % W8_T || K % W8_T || N <= 0 || K < 4 * W8_T) p8_ok = false;   // whole tiles; >= 4 k tiles: one bias MFMA per wave
    t128 += ((N + WT - 1) / WT) * ((K + WT - 1) / WT);
    tpp += ((N + WP_TN - 1) / WP_TN) * ((K + WP_TK - 1) / WP_TK);
    t8 += (N / W8_T) * (K / W8_T);
    elems += (size_t)(N * K); bias += (size_t)N;
  }
  // Eight-phase grid (TIMHIP_WGRAD_P8=0: off, A/B switch): whole 256 x 256 tiles (any contraction length: a ragged last stage
  // is an instance of its own) and rounds of 256 tiles filled to 90 % - at C2a that is the eight gradients of TWO encoder layers.
  p8_ok = p8_ok && tiled && kn.wgrad_p8 != 0 && t8 * 100 >= (t8 + 255) / 256 * 256 * 90;
  // Ping-pong grid (TIMHIP_WGRAD_PP=0: off, A/B switch): about a multiple of 256 tiles of 128 x 256 and a long M - an encoder
  // layer of a production batch.
  pp_ok = pp_ok && tiled && kn.wgrad_pp != 0 && tpp >= 192 && tpp * 100 >= (tpp + 255) / 256 * 256 * 75;
  WgradPlan p{};
  const int sk = wgrad_splits_for_tiles((int)t128, M, force_splits);
  wgrad_split_geometry(p, (int)t128, M, sk, elems, bias);
  if (sk == 1) p.ws_bytes = p.db_off = 0;   // dW / db written directly: no slabs, no reduce launch
  if (p8_ok || pp_ok) {
    p.tn = p8_ok ? W8_T : WP_TN; p.tk = p8_ok ? W8_T : WP_TK; p.tiles = (int)(p8_ok ? t8 : tpp);
    p.splits = 1; p.steps_per_split = (M + WM - 1) / WM; p.grid_x = (unsigned)p.tiles;
    // the 12-wave loader form is the default; TIMHIP_WGRAD_LD=0 selects the 8-wave merged-phase kernel (A/B switch)
    p.family = p8_ok ? WGRAD_P8 : (kn.wgrad_ld != 0 ? WGRAD_LD : WGRAD_PP8W);
    p.block = p.family == WGRAD_LD ? 768 : 512; p.lds_bytes = p8_ok ? 2 * W8_STAGE : WP_NST * WP_STAGE;
    // two 32-MFMA phases per step: the default since it was measured (TIMHIP_WGRAD_P8_PH=4: four 16-MFMA phases)
    if (p8_ok) { p.phases = kn.wgrad_p8_ph != 4 ? 2 : 4; p.ragged = (M % WP_M) != 0; }
    else p.pf_dist = kn.wgrad_pf;   // TIMHIP_WGRAD_PF (the 8-wave kernel carries the field and does not read it)
  }
  for (int i = 0; i < WGRAD_MAX_ITEMS; ++i)
    p.tile0[i + 1] = p.tile0[i] + (i < n ? ((it[i].Nout + p.tn - 1) / p.tn) * ((it[i].Kout + p.tk - 1) / p.tk) : 0);
  return p;
}

// The kernel-argument block of a group (WgGroup of wgrad.hip, WpGroup of wgrad_pp.hip: the same leading fields) from its items
// and plan; the slots past n are empty.
template <typename Group>
static inline void wgrad_fill_group(Group& g, const WgradPlan& p, const TimWgradItem* it, int n, int M, int accumulate, const float* out_scale) {
  g.n = n; g.M = M; g.accumulate = accumulate ? 1 : 0; g.out_scale = out_scale;
  const TimWgradItem none{};
  for (int i = 0; i < WGRAD_MAX_ITEMS; ++i) {
    const TimWgradItem& t = i < n ? it[i] : none;
    g.dY[i] = t.dY; g.X[i] = t.X; g.dW[i] = t.dW; g.db[i] = t.db; g.ldy[i] = t.ldy; g.ldx[i] = t.ldx; g.N[i] = t.Nout; g.K[i] = t.Kout;
    g.tile0[i] = p.tile0[i];
  }
  g.tile0[WGRAD_MAX_ITEMS] = p.tile0[WGRAD_MAX_ITEMS];
}
