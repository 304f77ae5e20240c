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
  constexpr int FP = NJB * 32, NKK = DH / 16, NDB = DH / 32;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* sK = smem;
  char* sV = smem + FP * DH * 2;
  // (window, head) = blockIdx.x / rsplit; a long sequence (detection: S = 499, B * H = 128) spreads its row blocks over rsplit
  // workgroups that each stage the K / V tile themselves (51 KB from L2) - 128 workgroups would leave half of the 256 CUs idle
  const int bh = blockIdx.x / a.rsplit, part = blockIdx.x - bh * a.rsplit;
  const int b = bh / a.H, h = bh % a.H;
  const int S = a.S, F = a.F, E = a.E;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const size_t ld = (size_t)3 * E;
  const HT* base = qkv + (size_t)b * S * ld + (size_t)h * DH;
  const int li = lane & 31, g = lane >> 5;
  const int rb0 = a.s0 >> 5;
  const int nrb = min((S + 31) >> 5, rb0 + (part + 1) * a.rper);
  const int nwaves = blockDim.x >> 6;
  // (five key blocks - F > 128 - hold 80 score registers per lane: no room for operands in flight, the requests stay where
  //  they are consumed)
  constexpr bool PRE = NJB <= 4;
  // Operand prefetch (round 4).  The block used to run a chain of dependent memory latencies - K tile, V tile, then per row
  // block its q / self-k rows, its self-v rows at the store - with two workgroups per CU to hide them: 31.5 us for 82 MB.  Now
  // every load is issued as early as its registers allow: the first row block's q / self-k rows BEFORE the K / V staging
  // loads (one latency for all three), K and V staged as a pair, the self-v rows and the NEXT row block's q / self-k rows
  // right after the S^T products (under the softmax and the P V products).
  auto load_rows = [&](int rbx, vec8<HT> (&qf)[NKK], vec8<HT> (&kself)[NKK]) {
    const int rowx = min(rbx * 32 + li, S - 1);
    const HT* qx = base + (size_t)rowx * ld;
#pragma unroll
    for (int kk = 0; kk < NKK; ++kk) qf[kk] = *reinterpret_cast<const vec8<HT>*>(qx + kk * 16 + g * 8);
    if (!PRE || rowx >= F) {   // (feature tokens have no self term; without operand prefetch the plain unconditional form)
#pragma unroll
      for (int kk = 0; kk < NKK; ++kk) kself[kk] = *reinterpret_cast<const vec8<HT>*>(qx + E + kk * 16 + g * 8);
    }
  };
  // one 32-row block of queries; qf / kself: its q rows and (query tokens) own-key rows, already requested
  auto row_block = [&](int rb, vec8<HT> (&qf)[NKK], vec8<HT> (&kself)[NKK]) {
    const int row = rb * 32 + li;
    const bool valid = row < S && row >= a.s0;   // (rows of the first block below s0: computed like the padding rows, not stored)
    const int rowc = row < S ? row : S - 1;
    const bool isq = rowc >= F;
    const HT* qp = base + (size_t)rowc * ld;
    unsigned long long kw = 0ull;   // KB: this lane's keep-bits, bit 4 c + t = key 8 c + 4 g + t (requested ahead of the products)
    if constexpr (KB) kw = a.kbits[((((size_t)b * a.H + h) * S + rowc) << 1) + g];

    // S^T = K Q^T : lane owns query row `row`, registers hold keys 32jb + (r&3) + 8(r>>2) + 4g
    f32x16_t sc[NJB];
#pragma unroll
    for (int jb = 0; jb < NJB; ++jb) {
#pragma unroll
      for (int r = 0; r < 16; ++r) sc[jb][r] = 0.f;
#pragma unroll
      for (int kk = 0; kk < NKK; ++kk) {
        const vec8<HT> kf = *reinterpret_cast<const vec8<HT>*>(sK + tile_off<DH>(jb * 32 + li, kk * 2 + g));
        sc[jb] = mfma16<HT>(kf, qf[kk], sc[jb]);
      }
      __builtin_amdgcn_sched_barrier(0);  // keep the K-fragment reads of later key blocks from being hoisted
    }
    // self score of query tokens (raw, unscaled like sc)
    float sself = -INFINITY;
    {
      float t = 0.f;
      if (isq) {
#pragma unroll
        for (int kk = 0; kk < NKK; ++kk) t += dot8(qf[kk], kself[kk]);
      }
      const float other = __shfl_xor(t, 32, 64);
      if (isq) sself = t + other;
    }
    // only the last key block can hold padded keys
    {
      constexpr int jb = NJB - 1;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = jb * 32 + (r & 3) + 8 * (r >> 2) + 4 * g;
        if (key >= F) sc[jb][r] = -INFINITY;
      }
    }
    float mx = sself;
#pragma unroll
    for (int jb = 0; jb < NJB; ++jb)
#pragma unroll
      for (int r = 0; r < 16; ++r) mx = fmaxf(mx, sc[jb][r]);
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    // p = exp(scale*(s - mx)) = exp2(c*s - c*mx)
    const float c2 = a.scale * 1.4426950408889634f;
    const float mc = mx * c2;
    float sum = 0.f;
#pragma unroll
    for (int jb = 0; jb < NJB; ++jb)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float p = __builtin_amdgcn_exp2f(fmaf(sc[jb][r], c2, -mc));
        sc[jb][r] = p;
        sum += p;
      }
    sum += __shfl_xor(sum, 32, 64);
    const float pself_un = isq ? __builtin_amdgcn_exp2f(fmaf(sself, c2, -mc)) : 0.f;
    sum += pself_un;
    const float inv = 1.f / sum;
    if (valid && g == 0 && lse) lse[((size_t)b * a.H + h) * S + row] = mx * a.scale + __logf(sum);
    const uint64_t rowbase = (((uint64_t)b * a.H + h) * S + rowc) * (uint64_t)a.LP;
#pragma unroll
    for (int jb = 0; jb < NJB; ++jb)
#pragma unroll
      for (int qp = 0; qp < 2; ++qp) {
        float ka[4] = {1.f, 1.f, 1.f, 1.f}, kb[4] = {1.f, 1.f, 1.f, 1.f};
        if constexpr (KB) {
          const int w32 = (int)(uint32_t)(kw >> (32 * (jb >> 1)));   // keys of key blocks 2 (jb >> 1), + 1: one dword
          const int ds = __float_as_int(a.dscale);
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            ka[t] = __int_as_float(__builtin_amdgcn_sbfe(w32, 16 * (jb & 1) + 8 * qp + t, 1) & ds);
            kb[t] = __int_as_float(__builtin_amdgcn_sbfe(w32, 16 * (jb & 1) + 8 * qp + 4 + t, 1) & ds);
          }
        } else if (a.thr != 0u) keep_pair(a, rowbase, jb * 32 + 16 * qp, g, ka, kb);   // (both lanes of a pair take this branch)
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          sc[jb][8 * qp + t] *= inv * ka[t];
          sc[jb][8 * qp + 4 + t] *= inv * kb[t];
        }
      }
    float pself = pself_un * inv;
    if (isq && a.thr != 0u) pself *= keep1(a, rowbase, F);

    // O^T = V^T P^T.  P is packed to bf16 first (frees the fp32 score registers); the head dim is
    // processed in halves so only NDB/2 accumulator tiles are live at a time.
    vec8<HT> pf[NJB][2];
#pragma unroll
    for (int jb = 0; jb < NJB; ++jb) {
      pf[jb][0] = pack8<HT>(sc[jb], 0);
      pf[jb][1] = pack8<HT>(sc[jb], 1);
    }
    // the self-v rows of this block (used at the store) go out now - the score registers are free - under the P V products
    vec8<HT> vself[NKK];
    if (PRE && isq) {
#pragma unroll
      for (int kk = 0; kk < NKK; ++kk) vself[kk] = *reinterpret_cast<const vec8<HT>*>(qp + 2 * E + kk * 16 + g * 8);
    }
    constexpr int NH = NDB >= 2 ? 2 : 1, DBH = NDB / NH;
    HT* op = o + ((size_t)b * (S - a.s0) + (valid ? row - a.s0 : 0)) * E + (size_t)h * DH;
#pragma unroll
    for (int hh = 0; hh < NH; ++hh) {
      f32x16_t oa[DBH];
#pragma unroll
      for (int d2 = 0; d2 < DBH; ++d2)
#pragma unroll
        for (int r = 0; r < 16; ++r) oa[d2][r] = 0.f;
#pragma unroll
      for (int jb = 0; jb < NJB; ++jb)
#pragma unroll
        for (int aa = 0; aa < 2; ++aa)
#pragma unroll
          for (int d2 = 0; d2 < DBH; ++d2) {
            const vec8<HT> vf = tr_frag<DH, HT>(sV, jb * 32 + 16 * aa, hh * DBH + d2, lane);
            oa[d2] = mfma16<HT>(vf, pf[jb][aa], oa[d2]);
            if (d2 == DBH - 1 && aa == 1) __builtin_amdgcn_sched_barrier(0);
          }
      // lanes l and l ^ 32 trade quads so that each stores 8 contiguous head-dim columns (16 bytes) per pair of quads;
      // the exchange is executed by every lane (shuffles), the store only by valid rows
#pragma unroll
      for (int d2 = 0; d2 < DBH; ++d2)
#pragma unroll
        for (int p2 = 0; p2 < 2; ++p2) {
          float v[8];
          pair_exchange(v, oa[d2][8 * p2], oa[d2][8 * p2 + 1], oa[d2][8 * p2 + 2], oa[d2][8 * p2 + 3], oa[d2][8 * p2 + 4],
                        oa[d2][8 * p2 + 5], oa[d2][8 * p2 + 6], oa[d2][8 * p2 + 7], g);
          const int dh = 32 * (hh * DBH + d2) + 16 * p2 + 8 * g;
          if (valid) {
            if (isq) {
              // columns dh .. dh + 7 = 16 (dh / 16) + 8 g: the chunk requested above (PRE), or read here
              const vec8<HT> sv = PRE ? vself[2 * (hh * DBH + d2) + p2] : *reinterpret_cast<const vec8<HT>*>(qp + 2 * E + dh);
#pragma unroll
              for (int u = 0; u < 8; ++u) v[u] = fmaf(pself, (float)sv[u], v[u]);
            }
            store8_h<HT>(op + dh, v);
          }
        }
    }
  };

  // The wave's first row block is peeled out of the loop: its operands were requested before the K / V staging, and keeping
  // them in registers of their own (not loop-carried) is what lets the compiler fit the kernel without spills.
  int rb = rb0 + part * a.rper + wave;
  if constexpr (!PRE) {   // the plain loop: operands requested where they are consumed
    stage_tile<DH>(sK, base + E, ld, FP, F, tid, blockDim.x);
    stage_tile<DH>(sV, base + 2 * E, ld, FP, F, tid, blockDim.x);
    __syncthreads();
    for (; rb < nrb; rb += nwaves) {
      vec8<HT> q1[NKK], k1[NKK];
      load_rows(rb, q1, k1);
      row_block(rb, q1, k1);
    }
    return;
  }
  {
    vec8<HT> q0[NKK], k0[NKK];
    if (PRE && rb < nrb) load_rows(rb, q0, k0);
    if constexpr (PRE) {
      stage_tile_pair<DH>(sK, base + E, sV, base + 2 * E, ld, FP, F, tid, blockDim.x);
    } else {
      stage_tile<DH>(sK, base + E, ld, FP, F, tid, blockDim.x);
      stage_tile<DH>(sV, base + 2 * E, ld, FP, F, tid, blockDim.x);
    }
    __syncthreads();
    if (!PRE && rb < nrb) load_rows(rb, q0, k0);
    if (rb < nrb) row_block(rb, q0, k0);
  }
  for (rb += nwaves; rb < nrb; rb += nwaves) {
    vec8<HT> q1[NKK], k1[NKK];
    load_rows(rb, q1, k1);
    row_block(rb, q1, k1);
  }
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
