// What the five attention units (attention.hip, attention_mfma.hip, attention_query.hip, attention_bwd2.hip, attention_f32.hip) share: the kernel
// argument block, the dropout keep factors, the table of shapes the matrix-core kernels are built for, the launch geometry
// helpers, the forward bodies the full and the query kernels both instantiate, and the entry points the units call across each
// other.  Included by those five units only.
#pragma once
#include <type_traits>

#include "common.h"
#include "mfma_tiles.h"

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

// ---- the forward bodies two units instantiate ------------------------------------------------------------------------------------
// attention_mfma.hip / attention.hip run them over the rows of a full qkv (QRY = false: keys and values are the first F rows of the
// window the rows belong to); attention_query.hip runs them over compact query rows against keys and values kept elsewhere
// (QRY = true: every row is a query row, `qs` says where the window's K | V rows live).  One softmax, one row_block: a row's
// arithmetic does not depend on which of the two forms computes it, so the query form's outputs are the full form's bits.
struct AttnQuerySrc {
  const void* kv;      // K columns of row 0 of window 0; V lies E elements behind K in the same row
  const int* widx;     // window of group g (device, G entries), or nullptr: group g reads window g
  int ldkv, wrows, W;  // row pitch (elements), rows from one window to the next, number of windows
};

// QRY: the window this block's group reads, or -1 - then the block stores quiet NaNs into the rows [r0, r1) of its head's columns and
// reads nothing (one comparison per block: a bad index never becomes an address)
template <typename T>
__device__ __forceinline__ int attn_query_window(const AttnQuerySrc& qs, int g, T* __restrict__ o_rows, int r0, int r1, int E, int Dh) {
  const int w = qs.widx ? qs.widx[g] : g;
  if ((unsigned)w < (unsigned)qs.W) return w;
  for (int idx = threadIdx.x; idx < (r1 - r0) * Dh; idx += blockDim.x)
    o_rows[(size_t)(r0 + idx / Dh) * E + idx % Dh] = (T)__builtin_nanf("");
  return -1;
}

// The 16-bit matrix-core forward (attention_mfma.hip describes the block: K / V of the head in LDS, 32-row blocks, a lane owns a row)
template <typename HT, int DH, int NJB, bool KB, bool QRY>
__device__ __forceinline__ void attn_fwd_mfma_body(const HT* __restrict__ qkv, HT* __restrict__ o, float* __restrict__ lse,
                                                   const AttnArgs& a, const AttnQuerySrc& qs) {
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
  // where the head's keys live (values: E elements behind them) - the window's own first F rows, or the group's window of the cache
  const HT* kp = base + E;
  const HT* vp = base + 2 * E;
  size_t ldk = ld;
  if constexpr (QRY) {
    const int w = attn_query_window(qs, b, o + (size_t)b * S * E + (size_t)h * DH, min(part * a.rper * 32, S), min(nrb * 32, S), E, DH);
    if (w < 0) return;
    kp = static_cast<const HT*>(qs.kv) + (size_t)w * qs.wrows * qs.ldkv + (size_t)h * DH;
    vp = kp + E;
    ldk = (size_t)qs.ldkv;
  }
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
    if (!PRE || QRY || rowx >= F) {   // (feature tokens have no self term; without operand prefetch the plain unconditional form)
#pragma unroll
      for (int kk = 0; kk < NKK; ++kk) kself[kk] = *reinterpret_cast<const vec8<HT>*>(qx + E + kk * 16 + g * 8);
    }
  };
  // one 32-row block of queries; qf / kself: its q rows and (query tokens) own-key rows, already requested
  auto row_block = [&](int rb, vec8<HT> (&qf)[NKK], vec8<HT> (&kself)[NKK]) {
    const int row = rb * 32 + li;
    const bool valid = row < S && row >= a.s0;   // (rows of the first block below s0: computed like the padding rows, not stored)
    const int rowc = row < S ? row : S - 1;
    const bool isq = QRY || rowc >= F;
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
    stage_tile<DH>(sK, kp, ldk, FP, F, tid, blockDim.x);
    stage_tile<DH>(sV, vp, ldk, FP, F, tid, blockDim.x);
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
      stage_tile_pair<DH>(sK, kp, sV, vp, ldk, FP, F, tid, blockDim.x);
    } else {
      stage_tile<DH>(sK, kp, ldk, FP, F, tid, blockDim.x);
      stage_tile<DH>(sV, vp, ldk, FP, F, tid, blockDim.x);
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

__device__ __forceinline__ float attn_keep(const AttnArgs& a, int b, int h, int row, int j) {
  if (a.thr == 0u) return 1.f;
  const uint64_t base = (((uint64_t)b * a.H + h) * a.S + row) * (uint64_t)a.LP + (uint64_t)j;
  return drop_mask1(a.seed, a.site, base, a.thr, a.dscale);
}

constexpr int KPL = 3;  // keys per lane: F <= 192

// The fp32-arithmetic forward (operand storage T = fp32, bf16 or fp16; attention.hip): one wave per token row, four rows in flight
template <typename T, bool QRY>
__device__ __forceinline__ void attn_fwd_simple_body(const T* __restrict__ qkv, T* __restrict__ o, float* __restrict__ lse,
                                                     const AttnArgs& a, const AttnQuerySrc& qs) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int b = blockIdx.x / a.H, h = blockIdx.x % a.H;
  const int Dh = a.Dh, F = a.F, S = a.S, E = a.E;
  const int KS = Dh + (sizeof(T) == 2 ? 2 : 1);
  T* sK = reinterpret_cast<T*>(smem);
  T* sV = sK + (size_t)F * KS;
  float* sQ = reinterpret_cast<float*>(smem + align_up((size_t)2 * F * KS * sizeof(T), 16));
  float* sP = sQ + 4 * Dh;
  const int PP = F + 4;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t ld = (size_t)3 * E;
  const T* base = qkv + (size_t)b * S * ld + (size_t)h * Dh;
  const T* kp = base + E;   // the head's keys (values: E elements behind them), as in attn_fwd_mfma_body
  size_t ldk = ld;
  if constexpr (QRY) {
    const int w = attn_query_window(qs, b, o + (size_t)b * S * E + (size_t)h * Dh, 0, S, E, Dh);
    if (w < 0) return;
    kp = static_cast<const T*>(qs.kv) + (size_t)w * qs.wrows * qs.ldkv + (size_t)h * Dh;
    ldk = (size_t)qs.ldkv;
  }
  for (int idx = tid; idx < F * Dh; idx += 256) {
    const int j = idx / Dh, c = idx % Dh;
    sK[j * KS + c] = kp[(size_t)j * ldk + c];
    sV[j * KS + c] = kp[(size_t)j * ldk + E + c];
  }
  __syncthreads();
  for (int r0 = a.s0; r0 < S; r0 += 4) {
    const int row = r0 + wave;
    const bool active = row < S;
    const T* qp = base + (size_t)(active ? row : 0) * ld;
    for (int c = lane; c < Dh; c += 64) sQ[wave * Dh + c] = OpT<T>::to_f(qp[c]) * a.scale;
    __syncthreads();
    float sc[KPL];
    float mx = -INFINITY;
#pragma unroll
    for (int kk = 0; kk < KPL; ++kk) {
      const int j = lane + 64 * kk;
      float s = -INFINITY;
      if (j < F) {
        s = 0.f;
        for (int c = 0; c < Dh; ++c) s = fmaf(sQ[wave * Dh + c], OpT<T>::to_f(sK[j * KS + c]), s);
      }
      sc[kk] = s;
      mx = fmaxf(mx, s);
    }
    const bool isq = QRY || row >= F;
    float sself = -INFINITY;
    if (isq && active) {
      float t = 0.f;
      for (int c = lane; c < Dh; c += 64) t = fmaf(sQ[wave * Dh + c], OpT<T>::to_f(qp[E + c]), t);
      sself = wave_sum(t);
    }
    mx = fmaxf(wave_max(mx), sself);
    float sum = 0.f;
#pragma unroll
    for (int kk = 0; kk < KPL; ++kk) {
      sc[kk] = (lane + 64 * kk < F) ? __expf(sc[kk] - mx) : 0.f;
      sum += sc[kk];
    }
    const float pself_un = isq ? __expf(sself - mx) : 0.f;
    sum = wave_sum(sum) + pself_un;
    const float inv = 1.f / sum;
    if (active && lane == 0 && lse) lse[((size_t)b * a.H + h) * S + row] = mx + __logf(sum);
#pragma unroll
    for (int kk = 0; kk < KPL; ++kk) {
      const int j = lane + 64 * kk;
      if (j < F) sP[wave * PP + j] = sc[kk] * inv * (active ? attn_keep(a, b, h, row, j) : 0.f);
    }
    const float pself = (isq && active) ? pself_un * inv * attn_keep(a, b, h, row, F) : 0.f;
    __syncthreads();
    if (active) {
      for (int c = lane; c < Dh; c += 64) {
        float acc = 0.f;
        for (int j = 0; j < F; ++j) acc = fmaf(sP[wave * PP + j], OpT<T>::to_f(sV[j * KS + c]), acc);
        if (isq) acc = fmaf(pself, OpT<T>::to_f(qp[2 * E + c]), acc);
        o[((size_t)b * (S - a.s0) + (row - a.s0)) * E + (size_t)h * Dh + c] = OpT<T>::from_f(acc);
      }
    }
    __syncthreads();
  }
}

// dynamic LDS of the fp32-arithmetic kernels: K and V of the head, nrowbuf row buffers and the probabilities of four rows
size_t simple_lds(const TimDesc& d, int nrowbuf) {
  const int Dh = d.E / d.H;
  const size_t ts = opsize(d.precision);
  const int KS = Dh + (ts == 2 ? 2 : 1);
  return align_up((size_t)2 * d.F * KS * ts, 16) + (size_t)nrowbuf * 4 * Dh * 4 + (size_t)4 * (d.F + 4) * 4;
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
