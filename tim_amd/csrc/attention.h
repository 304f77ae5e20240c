// What the four attention units (attention.hip, attention_mfma.hip, attention_bwd2.hip, attention_f32.hip) share: the kernel
// argument block, the dropout keep factors, the table of shapes the matrix-core kernels are built for, the launch geometry
// helpers, and the entry points the units call across each other.  Included by those four units only.
#pragma once
#include <type_traits>

#include "common.h"

namespace {

// (field order: what the MFMA forward's block had, then the two fields only one family reads - its kernels, the hot ones, keep the
//  offsets they had; a kernel loads the fields it reads and nothing else, so the unused ones cost kernarg bytes, not registers)
struct AttnArgs {
  int S, F, E, H, LP;  // LP = round_up(F + 1, 8): row pitch of the probability dropout stream
  float scale;
  uint32_t thr; float dscale; TimSeed seed; uint32_t site;
  int rsplit, rper;    // the 32-row blocks of a (window, head) are spread over rsplit workgroups of rper row blocks each (1: one workgroup)
  int s0;              // forward: first token row computed and stored (0: all).  Row blocks keep their 32-row alignment - the grid
                       // starts at block s0 / 32 - and rows land compactly in o, S - s0 per window (timhip_attention_fwd_rows)
  const unsigned long long* kbits;   // keep-bits drawn ahead of the layer (tim_attn_keep_bits; round 6), or nullptr
  int Dh;              // head width (the fp32-arithmetic kernels of attention.hip; a template parameter everywhere else)
  int abl;             // tuning builds only (TimDesc.reserved >> 8): 1 no scratch stores, 2 no dqkv stores, 4 operand rows alias row 0
};

AttnArgs make_attn_args(const TimDesc& d) {
  AttnArgs a;
  a.S = d.S; a.F = d.F; a.E = d.E; a.H = d.H; a.Dh = d.E / d.H; a.LP = round_up(d.F + 1, 8);
  a.scale = 1.f / sqrtf((float)a.Dh);
  a.thr = d.p_drop > 0.f ? drop_threshold(d.p_drop) : 0u;
  a.dscale = d.p_drop > 0.f ? 1.f / (1.f - d.p_drop) : 1.f;
  a.seed = d.seed; a.site = layer_site(d.layer, SITE_L_ATTN);
  a.rsplit = 1; a.rper = (d.S + 31) / 32;
  a.s0 = 0;
  a.kbits = nullptr;
  a.abl = (d.reserved >> 8) & 0xff;
  return a;
}

// keep factors of the four keys key .. key + 3 (rowbase + key a multiple of 4) / of one key of the row whose dropout stream
// starts at element rowbase
__device__ __forceinline__ void keep4(const AttnArgs& a, uint64_t rowbase, int key, float& k0, float& k1, float& k2,
                                      float& k3) {
  drop_mask4(a.seed, a.site, (rowbase + (uint64_t)key) >> 2, a.thr, a.dscale, k0, k1, k2, k3);
}
__device__ __forceinline__ float keep1(const AttnArgs& a, uint64_t rowbase, int key) {
  float k[4];
  drop_mask4(a.seed, a.site, (rowbase + (uint64_t)key) >> 2, a.thr, a.dscale, k[0], k[1], k[2], k[3]);
  const int c = (int)((rowbase + (uint64_t)key) & 3);
  return c == 0 ? k[0] : (c == 1 ? k[1] : (c == 2 ? k[2] : k[3]));
}

// keep factors of one lane pair's 16 keys kb .. kb+15 (kb a multiple of 16, rowbase of 8): lane g owns keys kb + 8t + 4g .. +3
// for t = 0, 1.  Counter t covers keys kb + 8t .. +7: lane g draws counter t = g and passes its partner (lane ^ 32) the half
// that lane owns - one Philox call and two exchanges per lane instead of two calls (common.h: 16-bit draws)
__device__ __forceinline__ void keep_pair(const AttnArgs& a, uint64_t rowbase, int kb, int g, float (&k0)[4], float (&k1)[4]) {
  const Philox4 r = philox4x32_7(a.seed, a.site, ((rowbase + (uint64_t)kb) >> 3) + (uint64_t)g);
  // v_permlane32_swap (x, z) and (y, w): lane g = 0 ends with (own x, partner's x), lane g = 1 with (partner's z, own z) - the
  // words of counter 0 first and of counter 1 second in both lanes, no select
  const auto xz = __builtin_amdgcn_permlane32_swap(r.x, r.z, false, false);
  const auto yw = __builtin_amdgcn_permlane32_swap(r.y, r.w, false, false);
  drop_mask4_words(xz[0], yw[0], a.thr, a.dscale, k0[0], k0[1], k0[2], k0[3]);
  drop_mask4_words(xz[1], yw[1], a.thr, a.dscale, k1[0], k1[1], k1[2], k1[3]);
}

// The (head width, 32-key blocks) pairs the matrix-core kernels are instantiated for - the 16-bit forward, the 16-bit rows + keys
// backward and the f32 forward / backward all take their shapes from here.  Calls f with the pair as two
// std::integral_constant values; TIMHIP_EUNSUPPORTED for every other pair (the caller falls through to attention.hip).
template <typename Fn>
inline int attn_for_shape(int Dh, int NJB, Fn&& f) {
  using std::integral_constant;
  if (Dh == 128) {
    switch (NJB) {
      case 1: return f(integral_constant<int, 128>{}, integral_constant<int, 1>{});
      case 2: return f(integral_constant<int, 128>{}, integral_constant<int, 2>{});
      case 3: return f(integral_constant<int, 128>{}, integral_constant<int, 3>{});
      case 4: return f(integral_constant<int, 128>{}, integral_constant<int, 4>{});
      case 5: return f(integral_constant<int, 128>{}, integral_constant<int, 5>{});
      default: break;
    }
  } else if (Dh == 64) {
    switch (NJB) {
      case 1: return f(integral_constant<int, 64>{}, integral_constant<int, 1>{});
      case 2: return f(integral_constant<int, 64>{}, integral_constant<int, 2>{});
      case 4: return f(integral_constant<int, 64>{}, integral_constant<int, 4>{});
      default: break;
    }
  } else if (Dh == 32) {
    switch (NJB) {
      case 1: return f(integral_constant<int, 32>{}, integral_constant<int, 1>{});
      case 2: return f(integral_constant<int, 32>{}, integral_constant<int, 2>{});
      default: break;
    }
  }
  return TIMHIP_EUNSUPPORTED;
}

// Row split of a (window, head): enough workgroups for two per CU (512) when B * H alone does not provide them, each with at
// least `waves_min` row blocks (one per wave).  C4 training (B = 16, H = 8, S = 499: 16 row blocks): 4 parts of 4 row blocks.
inline void attn_row_split(const TimDesc& d, int s0, int waves_min, int& rsplit, int& rper) {
  const int nrb = (d.S + 31) / 32 - s0 / 32, bh = d.B * d.H;
  int want = bh >= 512 ? 1 : (512 + bh - 1) / bh;
  const int most = nrb / (waves_min < 1 ? 1 : waves_min);
  if (want > most) want = most;
  if (want < 1) want = 1;
  rper = (nrb + want - 1) / want;
  rsplit = (nrb + rper - 1) / rper;
}

// waves of a block whose waves walk the 32-row blocks of S rows: one per row block, at most `cap`.  `knob`: TIMHIP_ATTN_WAVES
// (1 .. 8) overrides the count - fewer waves than row blocks, a wave then walks several; the f32 kernels do not take it
inline int attn_waves(int S, int cap, bool knob) {
  int n = (S + 31) / 32;
  n = n < 1 ? 1 : (n > cap ? cap : n);
  if (knob) {
    const int w = tim_knobs().attn_waves;
    if (w >= 1 && w <= 8) n = w;
  }
  return n;
}

}  // namespace

// attention_mfma.hip / attention_bwd2.hip: 16-bit operands.  All of these return TIMHIP_EUNSUPPORTED for what they have no kernel
// for; tim_attention_fwd / _bwd (attention.hip) then use the fp32-arithmetic kernels
int tim_attention_fwd_mfma(const TimDesc& d, const void* qkv, void* o, float* lse, hipStream_t s, const unsigned long long* kbits, int s0);
int tim_attention_bwd2_mfma(const TimDesc& d, const void* qkv, const void* o, const float* lse, const void* d_o,
                            void* dqkv, void* ws, size_t ws_bytes, hipStream_t s, const unsigned long long* kbits);
size_t tim_attention_bwd2_ws(const TimDesc& d);
// attention_f32.hip: exact-fp32 MFMA kernels for the fp32 / bf16x3 modes
int tim_attention_fwd_f32(const TimDesc& d, const void* qkv, void* o, float* lse, hipStream_t s, int s0);
int tim_attention_bwd_f32(const TimDesc& d, const void* qkv, const void* o, const float* lse, const void* d_o, void* dqkv,
                          void* ws, size_t ws_bytes, hipStream_t s);
size_t tim_attention_f32_bwd_ws(const TimDesc& d);
