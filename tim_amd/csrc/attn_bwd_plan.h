// LDS plan of the co-resident fused attention backward (attention_bwd2.hip: attn_bwd_co).  Plain C++ - no HIP types - so that the
// launcher and a host-only program (tests/attn_bwd_plan_print.cpp) share one statement of what the block holds.
#pragma once
#include <stddef.h>

// The block of attn_bwd_co: head width 128, 97 .. 128 feature keys (four 32-key blocks), S <= 160 (five 32-row sweeps).
//   K tile   [kv_rows][128] 16-bit   key rows 0 .. F - 1 are data, rows F .. kv_rows - 1 are written as zeros by the staging
//   V tile   the same
//   sweep    2 x [32 rows][128] 16-bit: Q | dO of the sweep, then - the same bytes - its dS | P~
// kv_rows = 128 whatever F is: the fragment reads of key block 3 (rows 96 + lane) and the transposing reads of the dQ units
// (rows 96 + 16 aa + 4 g + p / 4 + 8 hh <= 127) touch every row of the last key block, so all of them exist and the ones past F
// hold exact zeros.  The per-row scalars of a sweep (delta, self term, lse) have no bytes of their own: they pass through
// the sweep space between the last fragment read of Q / dO and the first store of dS / P~, in the 16 bytes the reading lane is
// about to overwrite itself.  2 x 32 KiB + 16 KiB = 80 KiB: two blocks per CU.
struct AttnBwdCoPlan {
  bool fits;         // the co-resident form serves this shape
  int kv_rows;       // rows of the K and of the V tile
  int sweeps;        // 32-row sweeps
  size_t k_off, v_off, ds_off, pt_off;   // byte offsets of the four regions
  size_t lds_bytes;  // dynamic LDS of the launch
};

constexpr size_t ATTN_BWD_CO_LDS_MAX = 80 * 1024;   // half of a CU's 160 KiB

inline AttnBwdCoPlan attn_bwd_co_plan(int S, int F, int Dh) {
  AttnBwdCoPlan p{};
  p.kv_rows = 128;
  p.sweeps = (S + 31) / 32;
  p.k_off = 0;
  p.v_off = p.k_off + (size_t)p.kv_rows * 128 * 2;
  p.ds_off = p.v_off + (size_t)p.kv_rows * 128 * 2;
  p.pt_off = p.ds_off + (size_t)32 * 128 * 2;
  p.lds_bytes = p.pt_off + (size_t)32 * 128 * 2;
  p.fits = Dh == 128 && S >= 1 && S <= 160 && F >= 97 && F <= 128 && F <= S && p.lds_bytes <= ATTN_BWD_CO_LDS_MAX;
  return p;
}
