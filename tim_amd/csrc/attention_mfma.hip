// MFMA (bf16 / fp16 operands: template parameter HT) structured attention for the TIM encoder: the forward, and the
// keep-bits of its dropout drawn ahead of a layer (the backward: attention_bwd2.hip).
//
// Math: see attention.hip (token i attends to the F feature tokens + itself; reference
// tim.py:161-166 mask over nn.MultiheadAttention, transformers.py:102).
//
// One workgroup (4 waves) per (window, head).  The F feature keys/values of the head
// (F <= 192, padded to NJB*32) live in LDS for the whole kernel; query rows are processed
// in blocks of 32 with the MFMA issued "swapped" (D = K_frag x Q_frag = S^T) so that a
// LANE OWNS ONE QUERY ROW: the softmax reduction is over that lane's registers plus one
// cross-half shuffle, the probabilities feed the P.V MFMA straight from registers (the MFMA
// contraction order is a free permutation, so P's accumulator registers 8a..8a+7 ARE a valid
// B operand), and V^T fragments come from LDS through ds_read_b64_tr_b16.
//
// LDS image of a [rows][DH] bf16 tile: row stride DH*2 bytes, 16-byte chunk index XOR g(row)
// with g chosen so that BOTH access patterns are bank-conflict free:
//   ds_read_b128 fragment reads (16 different rows, same chunk)   -> rows map to 16 distinct slots
//   ds_read_b64_tr_b16 reads (4 rows x 64 B)                      -> 16 distinct slots
#include <stdlib.h>

#include "attention.h"
#include "mfma_tiles.h"

namespace {

// ---------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------
// KB (round 6): the dropout keep-bits of the layer were drawn ahead of it (a.kbits, two 64-bit words per row: tim_attn_keep_bits) -
// a lane reads the word of its (row, key half g) with its q row and turns bits into factors (v_bfe_i32 + v_and per element)
// instead of eight Philox calls per row block.  Same bits, same results.
template <typename HT, int DH, int NJB, bool KB = false>
__global__ __launch_bounds__(512) void attn_fwd_mfma(const HT* __restrict__ qkv, HT* __restrict__ o,
                                                     float* __restrict__ lse, AttnArgs a) {
  attn_fwd_mfma_body<HT, DH, NJB, KB, false>(qkv, o, lse, a, AttnQuerySrc{});
}

// One wave per 32-row block of queries, but at most FOUR per block: the kernel needs 212 VGPRs (two waves per SIMD = eight wave
// slots per CU) and 64-80 KiB of LDS, so two 4-wave blocks are co-resident on a CU where a 5-wave block (S = 155) runs alone -
// one block's K / V staging and operand loads then overlap the other's arithmetic (C2a forward 33.3 -> 26.9 us; 3 waves 28.8,
// 8 waves 32.8); a wave walks rows rb, rb + 4, ...
constexpr int FWD_WAVES_MAX = 4;

template <typename HT, int DH, int NJB>
int launch_fwd(const TimDesc& d, const void* qkv, void* o, float* lse, hipStream_t s, const unsigned long long* kbits, int s0) {
  const size_t lds = (size_t)2 * NJB * 32 * DH * 2;
  AttnArgs a = make_attn_args(d);
  a.s0 = s0;
  // (few windows - B * H < 128, e.g. C2a at 8 windows per GPU - leave most CUs without a block: split down to TIMHIP_ATTN_SPLIT_MIN
  //  row blocks per workgroup there; default 4 = one per wave of a full block)
  attn_row_split(d, s0, d.B * d.H < 128 ? tim_knobs().attn_split_min : 4, a.rsplit, a.rper);
  const int waves = attn_waves(32 * a.rper, FWD_WAVES_MAX, true);
  if constexpr (DH == 128 && NJB == 4) {   // (the keep-bit form exists for the geometry tim_attn_keep_bits serves: C2a / C3 / C4)
    if (kbits && a.thr != 0u) {
      a.kbits = kbits;
      (void)hipFuncSetAttribute((const void*)attn_fwd_mfma<HT, DH, NJB, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      hipLaunchKernelGGL((attn_fwd_mfma<HT, DH, NJB, true>), dim3(d.B * d.H * a.rsplit), dim3(64 * waves), lds, s, (const HT*)qkv, (HT*)o,
                         lse, a);
      return hipGetLastError() == hipSuccess ? TIMHIP_OK : TIMHIP_ELAUNCH;
    }
  }
  (void)hipFuncSetAttribute((const void*)attn_fwd_mfma<HT, DH, NJB>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL((attn_fwd_mfma<HT, DH, NJB>), dim3(d.B * d.H * a.rsplit), dim3(64 * waves), lds, s, (const HT*)qkv, (HT*)o, lse,
                     a);
  return hipGetLastError() == hipSuccess ? TIMHIP_OK : TIMHIP_ELAUNCH;
}

// keep-bits of the attention dropout, one thread per (window, head, token row): the 8 elements of Philox counter c are the keys
// 8 c .. 8 c + 7; the MFMA kernels' lane (row, g) owns keys 8 c + 4 g + t - so the low nibble of a counter's keep-bits goes
// to word g = 0 and the high nibble to word g = 1, both at bit 4 c
struct KeepBitsArgs { unsigned long long* out[8]; TimSeed seed; uint32_t site[8]; uint32_t thr; int rows, nc, lp8; };
__global__ __launch_bounds__(256) void attn_keep_bits_kernel(KeepBitsArgs k) {
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row >= k.rows) return;
  const uint64_t c0 = (uint64_t)row * (uint64_t)k.lp8;
  const uint32_t site = k.site[blockIdx.y];
  // (unrolled over the 16 possible counters: a thread's draws are independent, and a runtime-bounded loop ran their 7-round
  //  dependency chains one after the other - 16 us for 6.2 M calls where the vector pipes need 6; the two 32-bit halves of a word
  //  are built separately: no 64-bit shifts)
  const uint64_t seed = k.seed;
  uint32_t lo0 = 0u, hi0 = 0u, lo1 = 0u, hi1 = 0u;
#pragma unroll
  for (int c = 0; c < 16; ++c) {
    if (c < k.nc) {
      const uint32_t bits = drop_bits8(seed, site, c0 + (uint64_t)c, k.thr);
      if (c < 8) { lo0 |= (bits & 15u) << (4 * c); lo1 |= (bits >> 4) << (4 * c); }
      else { hi0 |= (bits & 15u) << (4 * (c - 8)); hi1 |= (bits >> 4) << (4 * (c - 8)); }
    }
  }
  const unsigned long long w0 = ((unsigned long long)hi0 << 32) | lo0, w1 = ((unsigned long long)hi1 << 32) | lo1;
  typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
  u64x2 v; v[0] = w0; v[1] = w1;
  *reinterpret_cast<u64x2*>(k.out[blockIdx.y] + 2 * (size_t)row) = v;
}

}  // namespace

// returns TIMHIP_EUNSUPPORTED when the (head_dim, F) combination has no MFMA instantiation;
// the caller then uses the fp32-arithmetic kernels of attention.hip
int tim_attention_fwd_mfma(const TimDesc& d, const void* qkv, void* o, float* lse, hipStream_t s, const unsigned long long* kbits, int s0) {
  if (!h16_storage(d.precision) || (d.E % 8) != 0) return TIMHIP_EUNSUPPORTED;
  return attn_for_shape(d.E / d.H, (d.F + 31) / 32, [&](auto dh, auto njb) {
    DISPATCH_H16(d.precision, return (launch_fwd<HT, decltype(dh)::value, decltype(njb)::value>(d, qkv, o, lse, s, kbits, s0)));
  });
}

int tim_attn_keep_bits(const TimDesc& d, int first_layer, int n, unsigned long long* const* out, hipStream_t s) {
  if (n < 1 || n > 8 || !out) return TIMHIP_EINVAL;
  KeepBitsArgs k;
  for (int i = 0; i < 8; ++i) { k.out[i] = i < n ? out[i] : nullptr; k.site[i] = layer_site(first_layer + (i < n ? i : 0), SITE_L_ATTN); }
  k.seed = d.seed; k.thr = drop_threshold(d.p_drop);
  k.rows = d.B * d.H * d.S;
  k.lp8 = round_up(d.F + 1, 8) / 8;
  k.nc = k.lp8 < 16 ? k.lp8 : 16;   // keys 0 .. 127 (the self key of a 128-key window is drawn by the kernels themselves)
  hipLaunchKernelGGL(attn_keep_bits_kernel, dim3((k.rows + 255) / 256, n), dim3(256), 0, s, k);
  return hipGetLastError() == hipSuccess ? TIMHIP_OK : TIMHIP_ELAUNCH;
}
