// Which NT GEMM kernel a call gets, and its launch geometry: the ONE statement of the routing rules (plain C++, no HIP, no
// environment: `g++ -std=c++17 -fsyntax-only` takes it alone, tests/test_gemm_plan.py pins the routes without a GPU).
// gemm.hip and gemm_pp.hip ask for a plan and switch from it to the template instantiation; they decide nothing themselves.
// The plan runs per launch (144 per step): integer arithmetic only - no allocation, no lock, no read of the environment.
// A TUNING=1 build puts its experiment arms IN FRONT of the plan (one #ifdef block per file); a plan never names them.
#pragma once

#include "../../include/timhip.h"
#include "tim_knobs.h"

// tile geometry of the one-block-per-CU kernels (gemm_pp.hip): 256 columns, 128-byte (64-element) LDS rows, three-stage ring
constexpr int PP_BN = 256, PP_ROWB = 128, PP_NST = 3;

enum GemmFamily {
  GEMM_F32,    // gemm.hip      gemm_nt_f32_kernel: exact fp32 MFMA, 128 x 128
  GEMM_X3,     // gemm.hip      gemm_nt_x3_kernel: fp32 operands split into bf16 triples on the fly, 128 x 128
  GEMM_H16,    // gemm.hip      gemm_nt_h16_kernel: two blocks per CU, 64 / 128 / 160 x 128
  GEMM_PP8W,   // gemm_pp.hip   gemm_nt_pp_kernel: one 8-wave block per CU, 160 x 256 (the fallback of the loader-wave kernel)
  GEMM_LD,     // gemm_pp.hip   gemm_nt_ld_kernel: 8 MFMA waves + 4 loader waves, 128 / 160 x 256, one tile per block
  GEMM_LDP,    // gemm_pp.hip   gemm_nt_ldp_kernel: the same block walking 2 to 4 column tiles
  GEMM_P8      // gemm_pp.hip   gemm_nt_p8_kernel: eight-phase schedule, 256 / 320 x 256
};

struct GemmPlan {
  int family;             // GemmFamily
  int bm, bn;             // output tile
  int wm, wn;             // MFMA waves along M and N (the loader-wave kernels add four loader waves: block 768)
  int nst;                // LDS stages
  int tm;                 // 16-row MFMA tiles per wave: TMW 4 / 5 of the pp / loader-wave kernels, TM 8 / 10 of the eight-phase kernel; else 0
  int phases;             // eight-phase kernel: phases per contraction step, 2 or 4; else 0
  int tpb;                // column tiles a block walks
  int pf_dist, pf_mode;   // loader-wave kernels: L2 prefetch distance in stages (0: off) and mode
  int ksteps;             // gemm.hip kernels: contraction steps per split
  unsigned grid_x, grid_z, block, lds_bytes;   // the launch (lds_bytes: dynamic LDS)
};

static inline bool gemm_h16(int precision) { return precision == TIMHIP_PREC_BF16 || precision == TIMHIP_PREC_F16; }
static inline long long gemm_cdiv(long long a, long long b) { return (a + b - 1) / b; }

// ---- gemm.hip: two blocks per CU -----------------------------------------------------------------------------------------------
// Tile height.  Two tiles are built: 128 x 128 (2 x 2 waves of 64 x 64) and 160 x 128 (1 x 4 waves of 160 x 32).
// The taller tile stages 71 instead of 64 FLOP per LDS-DMA byte (the kernel is staging-bound) and quantises the
// encoder's M = 64 windows x 155 tokens = 9920 = 62 x 160 rows exactly: N = 1024 -> 496 tiles = ONE round of the
// 512 block slots (2 per CU) instead of 624 = 1.2 rounds.  Measured on M = 9920 (tools/gemm_tune.py, variant 14):
// +8...+35 % on every shape of the layer.  Cost model: rounds of 512 slots x tile height; the tall tile also wins ties.
static inline bool gemm_tall_tile_wins(int M, int N, int splitk) {
  if (M <= 128) return false;
  const long long tn = gemm_cdiv(N, 128);
  const long long t128 = gemm_cdiv(M, 128) * tn * splitk, t160 = gemm_cdiv(M, 160) * tn * splitk;
  const long long c128 = gemm_cdiv(t128, 512) * 128, c160 = gemm_cdiv(t160, 512) * 160;
  if (c160 != c128) return c160 < c128;
  return gemm_cdiv(M, 160) * 160 <= gemm_cdiv(M, 128) * 128 + 32;
}

// LDS stages of the small-problem (64 x 128) instances: TIMHIP_GEMM_SMALL_NST = 2 / 3 / 4 forces; 0 (default) = by the block
// count - as many stages as leave every block of the launch resident at once (24 KiB per stage, 160 KiB per CU)
static inline int gemm_small_nst(const TimKnobs& kn, long long blocks) {
  const int k = kn.gemm_small_nst;
  if (k >= 2 && k <= 4) return k;
  if (k == 1) return 2;
  return blocks <= 256 ? 4 : (blocks <= 512 ? 3 : 2);
}

// a gemm_nt_h16_kernel instance as a plan: BM x BN tile on WM x WN waves, NST stages of BKT contraction elements
static inline GemmPlan gemm_h16_tile(int bm, int bn, int wm, int wn, int nst, int M, int N, int Kp, int splitk, int bkt = 64) {
  GemmPlan p{};
  p.family = GEMM_H16; p.bm = bm; p.bn = bn; p.wm = wm; p.wn = wn; p.nst = nst; p.tpb = 1;
  p.ksteps = (int)gemm_cdiv(Kp / 64, splitk);
  p.grid_x = (unsigned)(gemm_cdiv(M, bm) * gemm_cdiv(N, bn)); p.grid_z = (unsigned)splitk; p.block = (unsigned)(wm * wn * 64);
  p.lds_bytes = (unsigned)(nst * (bm + bn) * bkt * 2);
  return p;
}

static inline GemmPlan gemm_h16_plan(const TimKnobs& kn, int M, int N, int Kp, int splitk) {
  // small problems (front end, heads: a few hundred to a few thousand rows): when 128-row tiles would fill at most
  // half of the 512 block slots, 64 x 128 tiles (1 x 4 waves of 64 x 32, 48 KB of LDS: three blocks per CU) double
  // the number of blocks - these launches are occupancy-bound, not staging-bound
  const long long t128 = gemm_cdiv(M, 128) * gemm_cdiv(N, 128) * splitk;
  if (t128 <= 256 && M > 64) {
    // (a block of such a launch is a CHAIN of K / 64 stage latencies: with two LDS stages one load is in flight while the
    //  previous stage is multiplied - 0.1 us of MFMAs - so a step lasts a memory latency; deeper rings divide that.
    //  TIMHIP_GEMM_SMALL_NST = 2 / 3 / 4 stages of 24 KiB: 3 / 2 / 1 blocks per CU)
    const int nst = gemm_small_nst(kn, gemm_cdiv(M, 64) * gemm_cdiv(N, 128) * splitk);
    // With the latency chain shortened, a step costs a wave its six LDS-DMA issue stalls and eight MFMAs: the launches of at
    // most 256 blocks (one per CU: three SIMD slots of four idle) run the tile on EIGHT waves, 2 x 4 of 32 x 32 - half of both
    // per wave: C2a at 8 windows per GPU 1.843 -> 1.790 ms, C1 0.832 -> 0.826 (profiles/r06_aa_small_gemm_w8_ab.txt; the
    // two-blocks-per-CU launches gain nothing from it: r06_ab).  TIMHIP_GEMM_SMALL_W8=0: four waves.
    return gemm_h16_tile(64, 128, nst >= 4 && kn.gemm_small_w8 != 0 ? 2 : 1, 4, nst, M, N, Kp, splitk);
  }
  if (gemm_tall_tile_wins(M, N, splitk)) return gemm_h16_tile(160, 128, 1, 4, 2, M, N, Kp, splitk);
  return gemm_h16_tile(128, 128, 2, 2, 2, M, N, Kp, splitk);
}

// ---- gemm_pp.hip: one block per CU ---------------------------------------------------------------------------------------------
// Is this problem one for the ping-pong kernels?  It needs enough 160 x 256 tiles to fill the 256 CUs about evenly: the
// encoder-layer GEMMs of a production batch (M = B * S in the thousands, N a multiple of 256 from 1024 up).
static inline bool gemm_pp_wins(const TimKnobs& kn, int M, int N, int splitk) {
  if (splitk != 1 || N < 512 || M < 1280) return false;
  const long long tiles = gemm_cdiv(M, 160) * gemm_cdiv(N, PP_BN);
  const long long rounds = gemm_cdiv(tiles, 256);
  if (tiles < 256) return tiles >= kn.gemm_pp_min;   // (TIMHIP_GEMM_PP_MIN_TILES: half-batch chains run 124-tile launches side by side)
  return tiles * 100 >= rounds * 256 * 75;   // the last round at least three quarters full on average
}

// The epilogues each family of gemm_pp.hip is instantiated for; a call with any other epilogue stays in gemm.hip.
constexpr bool gemm_pp_carries(int epi) {
  return epi == TIMHIP_EPI_STORE_T || epi == TIMHIP_EPI_RELU_T || epi == TIMHIP_EPI_STORE_F32 || epi == TIMHIP_EPI_DROP_RES_F32 ||
         epi == TIMHIP_EPI_ADD_F32 || epi == TIMHIP_EPI_GELU_DROP_G2 || epi == TIMHIP_EPI_GELU_T || epi == TIMHIP_EPI_MULAUX_T;
}
constexpr bool gemm_p8_carries(int epi) {
  return epi == TIMHIP_EPI_STORE_T || epi == TIMHIP_EPI_GELU_DROP_G2 || epi == TIMHIP_EPI_GELU_T || epi == TIMHIP_EPI_MULAUX_T;
}

// The eight-phase kernel's row tile for a launch (8, 10 or 0 = not taken; also what timhip_gemm_p8_choice answers).
// Which shapes: the ones that run MORE than one round of 160 x 256 tiles, when one of the two big tiles fills its rounds to at
// least 85 % (useful tile area / (rounds x 256 CUs)).  C2a, M = 9920: N = 3072 -> 256 rows (0.91), N = 2048 -> 320 rows (0.97),
// N = 1024 stays on the one-round 160-row kernel.  TIMHIP_GEMM_P8 = 0: off; 1 (default): by shape, the 16-bit store and the GELU
// epilogue; 2: by shape, also the multiply-by-saved-factor epilogue (linear2's input gradient: measured 40.2 against 46.8 us
// with a plain store but 53.3 against 52.6 with its epilogue - 80 MB of aux rows and results leave through 8 waves instead of
// 12 - profiles/r06_b_p8_ab.txt); 8 / 10: that tile for every legal shape and all three epilogues (tests)
static inline int gemm_p8_tm(const TimKnobs& kn, int epi, int M, int N, int Kp, int a_wrap) {
  const int k = kn.gemm_p8;
  if (k == 0 || a_wrap != 0 || Kp % 64 || Kp < 128 || N % PP_BN || M < 1) return 0;
  if (!gemm_p8_carries(epi)) return 0;
  if (k == 8 || k == 10) return k;
  if (epi == TIMHIP_EPI_MULAUX_T && k != 2) return 0;
  if (gemm_cdiv(M, 160) * (N / PP_BN) <= 256) return 0;
  auto fill = [&](int bm) {
    const long long tiles = gemm_cdiv(M, bm) * (N / PP_BN), rounds = gemm_cdiv(tiles, 256);
    return (double)M * N / ((double)bm * PP_BN) / (double)(rounds * 256);
  };
  const double f8 = fill(256), f10 = fill(320);
  if (f10 >= f8 && f10 >= 0.85) return 10;
  if (f8 >= 0.85) return 8;
  return 0;
}

// Tiles per block of the loader-wave kernel.  Two to four full rounds of tiles run as ONE round of blocks that walk that many
// column tiles each (gemm_nt_ldp_kernel) - the tiles of an XCD stay in step, so the prefetch shares apply to them.  In the
// step 5.343 -> 5.314 ms (four interleaved runs per arm, every run of the walk below every run of the one-tile kernel).
// The history of that number is in DESIGN.md section 5d: a first A/B had said -2.6 % against a one-tile instance that
// spilled; against the restored spill-free one-tile kernel the walk first LOST 1.3 % - it spilled 9-21 registers itself,
// the epilogue's loop-invariant lane arithmetic having been hoisted in front of the tile loop and held across the main
// loop; with the lane id laundered once per tile (8 / 5 / 1 spills on the three epilogues that use it) it wins 0.5 %.
static inline int gemm_pp_walk(int tiles, int tiles_n, int Kp) {
  if (tiles <= 256) return 1;
  const int want = (tiles + 255) / 256;
  return (want <= 4 && tiles_n % want == 0 && tiles % want == 0 && Kp >= 128) ? want : 1;
}

// Which row-panel height: 160 (the default: 98 FLOP per staged byte) or 128 (85)?  What a launch costs is (rounds of co-resident
// blocks) x (tiles a block walks) x (bytes a tile stages per step); M = 7984 (detection, B = 16 x 499 tokens) and M = 8000
// (Perception Test) give 50 panels of 160 rows - 200 tiles per 1024 columns on 256 CUs - but 63 panels of 128: 252.
// (Kept as it was: the cost prices the walk even when TIMHIP_GEMM_LDP=0 turns the walk off, and for the 8-wave kernel that
//  never walks - with those knobs the row tile is chosen for a launch that then runs one tile per block.)
static inline int gemm_pp_cost(int M, int N, int Kp, int bm) {
  const int tiles_n = (N + PP_BN - 1) / PP_BN, tiles = ((M + bm - 1) / bm) * tiles_n;
  const int tpb = gemm_pp_walk(tiles, tiles_n, Kp);
  const int blocks = tiles / tpb, rounds = (blocks + 255) / 256;
  return rounds * tpb * (bm + PP_BN);
}
static inline int gemm_pp_tmw(const TimKnobs& kn, int M, int N, int Kp) {
  const int force = kn.gemm_tmw;   // (A/B knob)
  if (force == 4 || force == 5) return force;
  return gemm_pp_cost(M, N, Kp, 128) * 100 < gemm_pp_cost(M, N, Kp, 160) * 97 ? 4 : 5;
}

static inline GemmPlan gemm_pp_plan(const TimKnobs& kn, int epi, int M, int N, int Kp, int a_wrap) {
  GemmPlan p{};
  p.bn = PP_BN; p.wm = 2; p.wn = 4; p.tpb = 1; p.grid_z = 1; p.block = 512;
  if (const int tm8 = gemm_p8_tm(kn, epi, M, N, Kp, a_wrap)) {
    p.family = GEMM_P8; p.tm = tm8; p.bm = 32 * tm8; p.nst = 2;
    p.phases = kn.gemm_p8_ph != 4 ? 2 : 4;   // two phases per step: the default (in-projection forward 60.0 -> 56.8 us, linear1 forward 54.5 -> 51.9: profiles/r06_af_*)
    p.grid_x = (unsigned)(gemm_cdiv(M, p.bm) * gemm_cdiv(N, PP_BN));
    p.lds_bytes = (unsigned)(p.nst * (p.bm + PP_BN) * PP_ROWB);
    return p;
  }
  // Default: the loader-wave kernel with the L2 prefetch (round 3: in the step 5.66 ms with the 8-wave kernel, 5.60-5.65 with
  // loader waves, 5.41-5.44 with loader waves + prefetch 4 stages ahead, NT GEMMs 763 -> 816 TFLOP/s; prefetch distance 2 / 3 / 5
  // / 6 / 8: +1.0 / +0.5 / +0.2 / +0.7 / +0.8 % of the step; every tile prefetching ALL its lines: 5.83-5.89 ms, the
  // prefetch loads then take the vector-memory path's time themselves).  TIMHIP_GEMM_LD=0: the 8-wave kernel (fallback).
  const bool loaders = kn.gemm_ld != 0 && a_wrap == 0;
  p.tm = loaders ? gemm_pp_tmw(kn, M, N, Kp) : 5;   // the 128-row tile exists for the loader-wave kernels only
  p.bm = 32 * p.tm; p.nst = PP_NST;
  p.lds_bytes = (unsigned)(PP_NST * (p.bm + PP_BN) * PP_ROWB);
  const int tiles_n = (N + PP_BN - 1) / PP_BN, tiles = ((M + p.bm - 1) / p.bm) * tiles_n;
  if (!loaders) {
    p.family = GEMM_PP8W; p.grid_x = (unsigned)tiles;
    return p;
  }
  if (kn.gemm_ldp != 0) p.tpb = gemm_pp_walk(tiles, tiles_n, Kp);   // (TIMHIP_GEMM_LDP=0: one tile per block)
  p.family = p.tpb > 1 ? GEMM_LDP : GEMM_LD;
  p.grid_x = (unsigned)(tiles / p.tpb); p.block = 768;
  // multi-round shapes run one tile per block (more than 256 tiles; TIMHIP_GEMM_PF_MR): no prefetch - their tiles drift apart
  // after the first round and a share covers a twelfth of a panel; in the step distance 0 / 2 / 4 / 6 / 8 / 12 for them:
  // 5.29 / 5.32 / 5.32 / 5.34 / 5.34 / 5.34 ms
  p.pf_dist = (tiles > 256 && p.tpb == 1) ? kn.gemm_pf_mr : kn.gemm_pf;
  p.pf_mode = kn.gemm_pf_mode;
  return p;
}

// ---- the entry point ----------------------------------------------------------------------------------------------------------
// Kp: K rounded up to 64; a_wrap: EpiDev.a_wrap (A repeats after that many 64-deep steps; 0: it does not).  The caller has
// checked the arguments (prepare_gemm): a valid precision, splitk >= 1.
static inline GemmPlan gemm_nt_plan(const TimKnobs& kn, int precision, int epi, int M, int N, int Kp, int splitk, int a_wrap) {
  if (!gemm_h16(precision)) {   // their 128 x 128 kernels: static LDS, 2 x 2 waves, 64- (x3) and 16-deep (fp32) steps
    GemmPlan p{};
    p.family = precision == TIMHIP_PREC_BF16X3 ? GEMM_X3 : GEMM_F32;
    p.bm = p.bn = 128; p.wm = p.wn = 2; p.nst = 1; p.tpb = 1;
    p.ksteps = (int)gemm_cdiv(Kp / (p.family == GEMM_X3 ? 64 : 16), splitk);
    p.grid_x = (unsigned)(gemm_cdiv(M, 128) * gemm_cdiv(N, 128)); p.grid_z = (unsigned)splitk; p.block = 256;
    return p;
  }
  // production-batch layer shapes: the one-block-per-CU kernels (TIMHIP_GEMM_PP=0 turns them off: A/B switch)
  if (kn.gemm_pp != 0 && gemm_pp_wins(kn, M, N, splitk) && gemm_pp_carries(epi)) return gemm_pp_plan(kn, epi, M, N, Kp, a_wrap);
  return gemm_h16_plan(kn, M, N, Kp, splitk);
}

// ---- the grouped launch (tim_gemm_nt_group): n independent 16-bit problems as one grid of 64-row tiles -----------------------------
struct GemmGroupPlan {
  int bn, wm, wn, nst;                  // 64 x bn tiles on wm x wn waves, nst stages
  unsigned tiles, block, lds_bytes;     // tiles = the grid
};
static inline GemmGroupPlan gemm_group_plan(const TimKnobs& kn, int epi, const TimGemmItem* items, int n) {
  auto count = [&](int bn) {
    long long t = 0;
    for (int i = 0; i < n; ++i) t += gemm_cdiv(items[i].M, 64) * gemm_cdiv(items[i].N, bn);
    return t;
  };
  GemmGroupPlan p{};
  p.block = 256;
  const long long t128 = count(128);
  if (t128 <= 512 && epi == TIMHIP_EPI_ADD_F32) {
    // still under-filled with 64 x 128 tiles (the heads' input gradients: one long-K item dominates): 64 x 64 tiles double
    // the blocks again
    p.bn = 64; p.wm = 2; p.wn = 2; p.nst = 2; p.tiles = (unsigned)count(64);
  } else {
    p.bn = 128; p.wm = 1; p.wn = 4; p.nst = gemm_small_nst(kn, t128); p.tiles = (unsigned)t128;
  }
  p.lds_bytes = (unsigned)(p.nst * (64 + p.bn) * 64 * 2);
  return p;
}
