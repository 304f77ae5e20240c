// A/B knobs of the launchers (plain C++: no HIP types, so host-only code such as gemm_plan.h and wgrad_plan.h can take them;
// what a TIMHIP_GEMM_* / TIMHIP_WGRAD_* routing knob does to a launch is stated there).
#pragma once

// Read from the environment ONCE (first launch) instead of per launch - the step issues 144 launches and the host is within
// 36 % of being the bottleneck.  timhip_reload_env() (test hook, include/timhip.h) re-reads them; the knobs marked (T) select
// kernels that exist only in a TUNING=1 build of the library and are ignored otherwise.  The initialisers are the defaults an
// unset variable gives (api.hip: read_knobs).
struct TimKnobs {
  int gemm_pp = 1;        // TIMHIP_GEMM_PP      0: no one-block-per-CU NT kernels at all (the two-blocks-per-CU kernels of gemm.hip)
  int gemm_ld = 1;        // TIMHIP_GEMM_LD      0: the 8-wave ping-pong kernel instead of loader waves + L2 prefetch
  int gemm_pf = 4;        // TIMHIP_GEMM_PF      L2 prefetch distance in stages (default 4, 0: off)
  int gemm_pf_mode = 1;   // TIMHIP_GEMM_PF_MODE 1: a tile touches its share of the XCD's lines, 2: all its lines
  int gemm_pf_mr = 0;     // TIMHIP_GEMM_PF_MR   prefetch distance of multi-round shapes run one tile per block (default 0)
  int gemm_ldp = 1;       // TIMHIP_GEMM_LDP     0: one tile per block where the default walks 2-4
  int gemm_ld1 = 0;       // TIMHIP_GEMM_LD1 (T) 1: one barrier per contraction step
  int gemm_pt = 0;        // TIMHIP_GEMM_PT  (T) 1: 8-wave persistent-tile kernel
  int gemm_dg = 0;        // TIMHIP_GEMM_DG  (T) 1: dual-group persistent kernel;  gemm_dg_offset: TIMHIP_GEMM_DG_OFFSET
  int gemm_dg_offset = 9;
  int fuse_ln = 0;        // TIMHIP_FUSE_LN  (T) 1: residual + LayerNorm inside the out-projection / linear2 epilogue
  int fuse_ln_spin = 100000;   // TIMHIP_FUSE_LN_SPIN
  int wgrad_pp = 1;       // TIMHIP_WGRAD_PP     0: no one-block-per-CU weight-gradient grid
  int wgrad_ld = 1;       // TIMHIP_WGRAD_LD     0: its 8-wave merged-phase form
  int wgrad_pf = 4;       // TIMHIP_WGRAD_PF     its L2 prefetch distance (default 4)
  int wgrad_p8_ph = 2;    // TIMHIP_WGRAD_P8_PH  phases per contraction step of the eight-phase weight-gradient kernel: 2 (32 MFMAs each, default) or 4 (16 each, as first written)
  int wgrad_p8 = 1;       // TIMHIP_WGRAD_P8     0: no eight-phase 256 x 256 weight-gradient grid (two layers per launch)
  int attn_waves = 0;     // TIMHIP_ATTN_WAVES   waves per attention block (0: by shape)
  int attn_fused = 1;     // TIMHIP_ATTN_FUSED   0: two-kernel attention backward
  int ln_rpb = 0;         // TIMHIP_LN_RPB       rows per LayerNorm-backward block (0: by shape)
  int gemm_p8_ph = 2;     // TIMHIP_GEMM_P8_PH   phases per contraction step of the eight-phase NT kernel: 2 (4 TM MFMAs each, default) or 4 (2 TM each, as first written)
  int gemm_small_w8 = 1;  // TIMHIP_GEMM_SMALL_W8   0: four waves instead of eight (2 x 4 of 32 x 32) on the small-problem GEMM's 64 x 128 tile where four stages are taken
  int gemm_small_nst = 0; // TIMHIP_GEMM_SMALL_NST  LDS stages of the small-problem GEMM instances (0: by the block count; 1 / 2: two, as before round 6)
  int ln_fwd_rpb = 0;     // TIMHIP_LN_FWD_RPB   rows per block of the 8-columns-per-lane LayerNorm forward (0: by the row count)
  int ln_rpb_small = 0;   // TIMHIP_LN_RPB_SMALL rows per block of the LayerNorm-backward launches that end in atomics (0: as TIMHIP_LN_RPB)
  int gemm_tmw = 0;       // TIMHIP_GEMM_TMW     5 / 4: force the 160- / 128-row tile of the loader-wave NT kernels (0: by shape)
  int attn_ks = 1;        // TIMHIP_ATTN_KS      0: fused attention backward with the one-wave-per-row-block phase 1 (default 1: key-split)
  int gemm_pp_min = 192;  // TIMHIP_GEMM_PP_MIN_TILES  fewest 160 x 256 tiles the one-block-per-CU NT kernels are used for (default 192)
  int attn_split_min = 4; // TIMHIP_ATTN_SPLIT_MIN  attention forward, B * H < 128: fewest row blocks per workgroup when a (window, head) is split (default 4)
  int epi_pair = 1;       // TIMHIP_EPI_PAIR     dropout + residual NT epilogue: lane pairs share the Philox calls of their keep factors (default 1)
  int ln_pair = 1;        // TIMHIP_LN_PAIR      LayerNorm backward: lane pairs share the Philox calls of their dropout keep factors (default 1)
  int gemm_p8 = 1;        // TIMHIP_GEMM_P8      eight-phase 256 / 320 x 256 tiles for the multi-round NT shapes: 0 off, 1 by shape (default), 2 + the mulaux epilogue, 8 / 10 forced
  int attn_bwd_co = 1;    // TIMHIP_ATTN_BWD_CO  0: the key-split fused attention backward as ONE 8-wave block per CU with a phase 2 at the end (default 1: two co-resident 4-wave blocks per CU, dK / dV accumulated per row sweep)
  int epi_g2_pk = 1;      // TIMHIP_EPI_G2_PK    0: the eight-phase NT kernel's gelu + gelu' epilogue one quad at a time through epi_oct (default 1: whole wave tiles with keep-bits or p = 0 take the branch-free pair form, gemm_pp.hip: pp_epilogue_g2pk - the same bits)
  int epi_wt = 1;         // TIMHIP_EPI_WT       0: the 160-row loader-wave NT kernel's DROP_RES_F32 epilogue one quad at a time through epi_quad (default 1: whole wave tiles take the straight-line form whose stores stream, gemm_pp.hip: pp_epilogue_wt_res - the same bits)
};
const TimKnobs& tim_knobs();
