// Query attention maps: the head-averaged softmax weights of one encoder layer (timhip_attention_weights) - what the
// reference's TransformerEncoder.forward returns beside its output (transformers.py:45-48,102: nn.MultiheadAttention's
// need_weights result, averaged over heads) and the fused attention kernels never store.
//
// TIM's mask (tim.py:161-166) lets token s attend to the F feature tokens and to itself, so a row of the reference's dense
// [S, S] map has F + 1 non-zeros at most.  The map is stored that way: for the token rows s0 <= s < S of every window
//
//   w[b, s - s0, j] = 1/H * sum over heads h (ascending) of softmax_j( scale * q[b,h,s] . k[b,h,key(j)] ),   0 <= j <= F
//   key(j) = j for j < F;  column F = the token's own key for query rows (s >= F), exact 0.0f for feature rows (their own key
//   is one of the F)
//
// fp32, row pitch ld >= F + 1.  per_head: [B, H, S - s0, ld], one map per head, no mean.
//
// Where things are rounded (the unit is compiled with contraction off; every fused multiply-add below is written as one):
//   score   raw q . k in fp32 - on the matrix cores for the 16-bit kernels (products of 16-bit operands are exact in fp32), an
//           fmaf chain in ascending head-dim order in the generic kernel;
//   max     over the row's F (+ 1) raw scores;   p = exp2(fma(score, c, -(max * c))),  c = scale * log2(e)
//   sum     fp32, in the order the kernel's lanes hold the keys;   weight = p * (1 / sum)
//   mean    acc += weight for h = 0 .. H - 1 in registers, then acc * (1 / H)
// The softmax is computed here, with max and sum over the row's scores: there is no lse to take (the evaluation forward
// stores none).
//
// One workgroup owns a block of token rows of one window and walks the heads in ascending order; a head's keys go through
// LDS once per (row block, head).  A row's arithmetic is that of its lane (16-bit kernels: attention_mfma.hip's ownership, a
// lane pair owns a query row) or of its wave (generic kernel) and of nothing else: not of B, not of s0, not of the way rows
// are spread over workgroups.  No atomics; the same window gives the same bits alone or inside any batch, on every run.
//
// timhip_attention_query_weights: the same two bodies with QRY = true - every row is a query row of one of G groups (compact
// [G Q, 3E] rows: q | own k | own v) and the F keys are those of window widx[g] of a K | V cache (AttnQuerySrc, attention.h).  QRY
// changes where a workgroup finds its rows and its keys and, on ordinary rows, nothing about what a lane does with them, so on
// equal q and K values the rows are timhip_attention_weights' query rows bit for bit; the one exception are rows with
// |max c| >= 2^30 (map_p_wide below), where that entry's exponent line is not finite.  A widx[g] outside [0, W) never becomes an address: the
// workgroups of that group store quiet NaNs into columns 0 .. F of their rows and return.
#pragma clang fp contract(off)
#include <stdint.h>

#include "attention.h"
#include "mfma_tiles.h"

namespace {

struct MapArgs {
  int S, F, E, H, Dh;
  float scale, inv_h;
  int s0, ld;
  int nblk;   // workgroups per window
  int nwr;    // 16-bit kernels: row-owning waves (32-row blocks) of a workgroup
};

constexpr float LOG2E = 1.4426950408889634f;

// p of one raw score: exp2(fma(score, c, -(max c))).  At the row's largest score the exponent is not 0 but the rounding error of
// max c, at most 2^-24 |max c|: a common factor of the row that the normalisation cancels - while it stays an exponent exp2 can
// take.  QRY only: a row with |max c| >= 2^30 (wide; raw scores near the largest finite value of bf16 / fp32) takes
// exp2((score - max) c) instead, exact 0 at the maximum and never positive; every other row keeps the line above and its bits
// (timhip_attention_weights has that line alone and is not finite on such rows)
// (the full form's lines stay as they were written, QRY = false compiles to the instructions it had)
__device__ __forceinline__ float map_p_wide(float score, float mx, float c2, float mc, bool wide) {
  return __builtin_amdgcn_exp2f(wide ? (score - mx) * c2 : fmaf(score, c2, -mc));
}
constexpr float WIDE_MC = 1073741824.f;   // 2^30

// the last kernel argument: where the keys live when they are not the rows' own window (QRY), nothing otherwise
struct NoSrc {};
template <bool QRY> using MapSrc = std::conditional_t<QRY, AttnQuerySrc, NoSrc>;

// ---------------------------------------------------------------------------------------------------------------------
// 16-bit operands, shapes of attn_for_shape: S^T = K Q^T on the matrix cores, a lane pair (lane, lane ^ 32) owns a row -
// lane half g holds keys 32 jb + (r & 3) + 8 (r >> 2) + 4 g in register r of key block jb (attention_mfma.hip)
// ---------------------------------------------------------------------------------------------------------------------
template <int NJB>
__device__ __forceinline__ void store_row(float* __restrict__ wr, const f32x16_t (&v)[NJB], float vself, float mul, int F, int g,
                                          bool isq) {
#pragma unroll
  for (int jb = 0; jb < NJB; ++jb)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = jb * 32 + (r & 3) + 8 * (r >> 2) + 4 * g;
      if (jb < NJB - 1 || key < F) wr[key] = v[jb][r] * mul;   // (only the last key block can hold padded keys)
    }
  if (g == 0) wr[F] = isq ? vself * mul : 0.f;
}

// QRY: the window group g reads, or -1 - then the workgroup stores quiet NaNs into columns 0 .. F of its rows [r0, r1) (PH: of every
// head's map) and reads nothing (attn_query_window's rule, attention.h: one comparison per workgroup, block-uniform)
template <bool PH>
__device__ __forceinline__ int map_query_window(const AttnQuerySrc& qs, int g, float* __restrict__ w, const MapArgs& a, int r0, int r1) {
  const int win = qs.widx ? qs.widx[g] : g;
  if ((unsigned)win < (unsigned)qs.W) return win;
  const int nc = a.F + 1, nh = PH ? a.H : 1;
  const size_t nrow = (size_t)(a.S - a.s0);
  for (int h = 0; h < nh; ++h) {
    float* wh = w + ((size_t)g * nh + h) * nrow * a.ld;
    for (int idx = threadIdx.x; idx < (r1 - r0) * nc; idx += blockDim.x)
      wh[(size_t)(r0 + idx / nc) * a.ld + idx % nc] = __builtin_nanf("");
  }
  return -1;
}

// The workgroup is always four waves: `nwr` of them (1 .. 4) own a 32-row block each, all four stage the keys.  The K tile of
// head h + 1 is requested - into registers - before the products of head h start and written to the other LDS buffer behind
// them: one barrier and no exposed memory latency per head (a first version staged each head where it was consumed, by the
// row-owning waves alone: 45 us at C2a / 64 windows, a chain of eight times four memory latencies).
template <typename HT, int DH, int NJB, bool PH, bool QRY = false>
__global__ __launch_bounds__(256) void attn_w_mfma(const HT* __restrict__ qkv, float* __restrict__ w, MapArgs a, MapSrc<QRY> qs) {
  constexpr int FP = NJB * 32, NKK = DH / 16, NC = DH / 8;
  constexpr int TILE = FP * DH * 2;                  // bytes of one head's K tile (tile_off image)
  constexpr int NCH = (FP * NC + 255) / 256;         // 16-byte chunks of a tile per thread
  extern __shared__ __attribute__((aligned(16))) char smem[];   // two K tiles
  const int b = blockIdx.x / a.nblk, part = blockIdx.x - b * a.nblk;
  const int S = a.S, F = a.F, E = a.E;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, g = lane >> 5;
  const size_t ldq = (size_t)3 * E;
  const HT* wbase = qkv + (size_t)b * S * ldq;
  // row blocks keep their 32-row alignment (the grid starts at block s0 / 32), one per row-owning wave
  const int rb = (a.s0 >> 5) + part * a.nwr + wave;
  const bool owner = wave < a.nwr && rb * 32 < S;    // (wave-uniform; the other waves only stage)
  const int row = rb * 32 + li;
  const bool valid = owner && row < S && row >= a.s0;   // (rows below s0 / past S - 1: computed like the padding rows, not stored)
  const int rowc = row < S ? row : S - 1;
  const bool isq = QRY || rowc >= F;
  const size_t nrow = (size_t)(S - a.s0);
  const float c2 = a.scale * LOG2E;
  // QRY: the heads' keys are not the window's own first F rows but those of the group's window of the cache
  const HT* kwin = nullptr;
  if constexpr (QRY) {
    const int rpb = 32 * a.nwr;   // (s0 = 0: the workgroup's rows by compact index)
    const int win = map_query_window<PH>(qs, b, w, a, min(part * rpb, S), min((part + 1) * rpb, S));
    if (win < 0) return;
    kwin = static_cast<const HT*>(qs.kv) + (size_t)win * qs.wrows * qs.ldkv;
  }

  // this thread's chunks of head h's K tile: requested / written (rows >= F are zero)
  auto tile_load = [&](int h, vec8<HT> (&v)[NCH]) {
    const HT* src = wbase + (size_t)h * DH + E;
    size_t ldk = ldq;
    if constexpr (QRY) {
      src = kwin + (size_t)h * DH;
      ldk = (size_t)qs.ldkv;
    }
#pragma unroll
    for (int u = 0; u < NCH; ++u) {
      const int idx = tid + u * 256, r = idx / NC, c = idx % NC;
      if (idx < FP * NC && r < F) {
        v[u] = *reinterpret_cast<const vec8<HT>*>(src + (size_t)r * ldk + c * 8);
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[u][e] = (HT)0.f;
      }
    }
  };
  auto tile_store = [&](char* tile, const vec8<HT> (&v)[NCH]) {
#pragma unroll
    for (int u = 0; u < NCH; ++u) {
      const int idx = tid + u * 256;
      if (idx < FP * NC) *reinterpret_cast<vec8<HT>*>(tile + tile_off<DH>(idx / NC, idx % NC)) = v[u];
    }
  };
  auto rows_load = [&](int h, vec8<HT> (&qf)[NKK], vec8<HT> (&kself)[NKK]) {
    const HT* qx = wbase + (size_t)h * DH + (size_t)rowc * ldq;
#pragma unroll
    for (int kk = 0; kk < NKK; ++kk) qf[kk] = *reinterpret_cast<const vec8<HT>*>(qx + kk * 16 + g * 8);
#pragma unroll
    for (int kk = 0; kk < NKK; ++kk) kself[kk] = *reinterpret_cast<const vec8<HT>*>(qx + E + kk * 16 + g * 8);
  };

  f32x16_t acc[NJB];
  float acc_self = 0.f;
#pragma unroll
  for (int jb = 0; jb < NJB; ++jb)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[jb][r] = 0.f;

  vec8<HT> qf[NKK], kself[NKK];
  {
    vec8<HT> t0[NCH];
    if (owner) rows_load(0, qf, kself);
    tile_load(0, t0);
    tile_store(smem, t0);
  }
  for (int h = 0; h < a.H; ++h) {
    const char* sK = smem + (h & 1) * TILE;
    __syncthreads();   // head h's keys are in sK; every wave is done with the other buffer (head h - 1)
    const bool more = h + 1 < a.H;
    vec8<HT> tn[NCH];
    if (more) tile_load(h + 1, tn);
    if (owner) {
      // self score of query tokens (raw)
      float sself = -INFINITY;
      {
        float t = 0.f;
#pragma unroll
        for (int kk = 0; kk < NKK; ++kk) t += dot8(qf[kk], kself[kk]);
        const float other = __shfl_xor(t, 32, 64);
        if (isq) sself = t + other;
      }
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
      }
      if (more) rows_load(h + 1, qf, kself);   // (the next head's rows, under the softmax)
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
      const float mc = mx * c2;
      [[maybe_unused]] const bool wide = QRY && !(fabsf(mc) < WIDE_MC);
      float sum = 0.f;
#pragma unroll
      for (int jb = 0; jb < NJB; ++jb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          float p;
          if constexpr (QRY) p = map_p_wide(sc[jb][r], mx, c2, mc, wide);
          else p = __builtin_amdgcn_exp2f(fmaf(sc[jb][r], c2, -mc));
          sc[jb][r] = p;
          sum += p;
        }
      sum += __shfl_xor(sum, 32, 64);
      float pself;
      if constexpr (QRY) pself = map_p_wide(sself, mx, c2, mc, wide);
      else pself = isq ? __builtin_amdgcn_exp2f(fmaf(sself, c2, -mc)) : 0.f;
      sum += pself;
      const float inv = 1.f / sum;
      if constexpr (PH) {
        if (valid) store_row<NJB>(w + (((size_t)b * a.H + h) * nrow + (size_t)(row - a.s0)) * a.ld, sc, pself, inv, F, g, isq);
      } else {
#pragma unroll
        for (int jb = 0; jb < NJB; ++jb)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[jb][r] += sc[jb][r] * inv;
        acc_self += pself * inv;
      }
    }
    if (more) tile_store(smem + ((h + 1) & 1) * TILE, tn);
  }
  if constexpr (!PH) {
    if (valid) store_row<NJB>(w + ((size_t)b * nrow + (size_t)(row - a.s0)) * a.ld, acc, acc_self, a.inv_h, F, g, isq);
  }
}

// row blocks per workgroup: four, unless that leaves fewer than one workgroup per CU - then two, then one (a narrower block
// stages the keys more often, from L2; an idle CU stages nothing)
int mfma_row_waves(int B, int nrb) {
  for (int wv = 4; wv > 1; wv >>= 1)
    if (nrb >= wv && (long long)B * ((nrb + wv - 1) / wv) >= 256) return wv;
  return 1;
}

// qs != nullptr: the query form (s0 = 0; d.B groups of d.S compact rows against d.F cached keys)
template <typename HT, int DH, int NJB>
int launch_mfma(const TimDesc& d, const void* qkv, int s0, int per_head, float* w, int ld, hipStream_t s,
                const AttnQuerySrc* qs = nullptr) {
  const size_t lds = (size_t)2 * NJB * 32 * DH * 2;
  const int nrb = (d.S + 31) / 32 - s0 / 32;
  const int nwr = mfma_row_waves(d.B, nrb);
  MapArgs a{d.S, d.F, d.E, d.H, DH, 1.f / sqrtf((float)DH), 1.f / (float)d.H, s0, ld, (nrb + nwr - 1) / nwr, nwr};
  const dim3 grid((unsigned)d.B * (unsigned)a.nblk), block(256);
  if (qs) {
    if (per_head) {
      (void)hipFuncSetAttribute((const void*)attn_w_mfma<HT, DH, NJB, true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      hipLaunchKernelGGL((attn_w_mfma<HT, DH, NJB, true, true>), grid, block, lds, s, (const HT*)qkv, w, a, *qs);
    } else {
      (void)hipFuncSetAttribute((const void*)attn_w_mfma<HT, DH, NJB, false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      hipLaunchKernelGGL((attn_w_mfma<HT, DH, NJB, false, true>), grid, block, lds, s, (const HT*)qkv, w, a, *qs);
    }
  } else if (per_head) {
    (void)hipFuncSetAttribute((const void*)attn_w_mfma<HT, DH, NJB, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL((attn_w_mfma<HT, DH, NJB, true>), grid, block, lds, s, (const HT*)qkv, w, a, NoSrc{});
  } else {
    (void)hipFuncSetAttribute((const void*)attn_w_mfma<HT, DH, NJB, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL((attn_w_mfma<HT, DH, NJB, false>), grid, block, lds, s, (const HT*)qkv, w, a, NoSrc{});
  }
  return hipGetLastError() == hipSuccess ? TIMHIP_OK : TIMHIP_ELAUNCH;
}

// ---------------------------------------------------------------------------------------------------------------------
// every other shape, the fp32-storage modes and TIMHIP_DESC_ATTN_FP32: fp32 arithmetic, a wave owns a row, lane l the keys
// l, l + 64, l + 128 (F <= 192)
// ---------------------------------------------------------------------------------------------------------------------
constexpr int GKPL = 3;    // keys per lane
constexpr int GROWS = 8;   // rows per wave: a workgroup of four waves owns 32 consecutive rows

template <typename T, bool PH, bool QRY = false>
__global__ __launch_bounds__(256) void attn_w_generic(const T* __restrict__ qkv, float* __restrict__ w, MapArgs a, MapSrc<QRY> qs) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int b = blockIdx.x / a.nblk, part = blockIdx.x - b * a.nblk;
  const int Dh = a.Dh, F = a.F, S = a.S, E = a.E;
  const int KS = Dh + (sizeof(T) == 2 ? 2 : 1);
  T* sK = reinterpret_cast<T*>(smem);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const size_t ldq = (size_t)3 * E;
  const int row0 = a.s0 + (part * 4 + wave) * GROWS;
  const size_t nrow = (size_t)(S - a.s0);
  const float c2 = a.scale * LOG2E;
  const T* kwin = nullptr;   // QRY: row 0 of the group's window in the cache
  if constexpr (QRY) {
    const int rpb = 4 * GROWS;
    const int win = map_query_window<PH>(qs, b, w, a, min(part * rpb, S - a.s0), min((part + 1) * rpb, S - a.s0));
    if (win < 0) return;
    kwin = static_cast<const T*>(qs.kv) + (size_t)win * qs.wrows * qs.ldkv;
  }
  float acc[GROWS][GKPL], accs[GROWS];
#pragma unroll
  for (int r = 0; r < GROWS; ++r) {
    accs[r] = 0.f;
#pragma unroll
    for (int kk = 0; kk < GKPL; ++kk) acc[r][kk] = 0.f;
  }
  for (int h = 0; h < a.H; ++h) {
    const T* base = qkv + (size_t)b * S * ldq + (size_t)h * Dh;
    if (h) __syncthreads();   // every wave has read the previous head's keys
    for (int idx = tid; idx < F * Dh; idx += 256) {
      const int j = idx / Dh, c = idx % Dh;
      if constexpr (QRY) sK[j * KS + c] = kwin[(size_t)j * qs.ldkv + (size_t)h * Dh + c];
      else sK[j * KS + c] = base[(size_t)j * ldq + E + c];
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < GROWS; ++r) {
      const int row = row0 + r;   // (wave-uniform: the q row is read through uniform addresses)
      if (row >= S) continue;
      const T* qp = base + (size_t)row * ldq;
      const bool isq = QRY || row >= F;
      float sc[GKPL];
      float mx = -INFINITY;
#pragma unroll
      for (int kk = 0; kk < GKPL; ++kk) {
        const int j = lane + 64 * kk;
        float sv = -INFINITY;
        if (j < F) {
          sv = 0.f;
          for (int c = 0; c < Dh; ++c) sv = fmaf(OpT<T>::to_f(qp[c]), OpT<T>::to_f(sK[j * KS + c]), sv);
        }
        sc[kk] = sv;
        mx = fmaxf(mx, sv);
      }
      float sself = -INFINITY;
      if (isq) {
        float t = 0.f;
        for (int c = lane; c < Dh; c += 64) t = fmaf(OpT<T>::to_f(qp[c]), OpT<T>::to_f(qp[E + c]), t);
        sself = wave_sum(t);
      }
      mx = fmaxf(wave_max(mx), sself);
      const float mc = mx * c2;
      [[maybe_unused]] const bool wide = QRY && !(fabsf(mc) < WIDE_MC);
      float sum = 0.f;
#pragma unroll
      for (int kk = 0; kk < GKPL; ++kk) {
        if constexpr (QRY) sc[kk] = (lane + 64 * kk < F) ? map_p_wide(sc[kk], mx, c2, mc, wide) : 0.f;
        else sc[kk] = (lane + 64 * kk < F) ? __builtin_amdgcn_exp2f(fmaf(sc[kk], c2, -mc)) : 0.f;
        sum += sc[kk];
      }
      float pself;
      if constexpr (QRY) pself = map_p_wide(sself, mx, c2, mc, wide);
      else pself = isq ? __builtin_amdgcn_exp2f(fmaf(sself, c2, -mc)) : 0.f;
      sum = wave_sum(sum) + pself;
      const float inv = 1.f / sum;
      if constexpr (PH) {
        float* wr = w + (((size_t)b * a.H + h) * nrow + (size_t)(row - a.s0)) * a.ld;
#pragma unroll
        for (int kk = 0; kk < GKPL; ++kk)
          if (lane + 64 * kk < F) wr[lane + 64 * kk] = sc[kk] * inv;
        if (lane == 0) wr[F] = pself * inv;
      } else {
#pragma unroll
        for (int kk = 0; kk < GKPL; ++kk) acc[r][kk] += sc[kk] * inv;
        accs[r] += pself * inv;
      }
    }
  }
  if constexpr (!PH) {
#pragma unroll
    for (int r = 0; r < GROWS; ++r) {
      const int row = row0 + r;
      if (row >= S) continue;
      float* wr = w + ((size_t)b * nrow + (size_t)(row - a.s0)) * a.ld;
#pragma unroll
      for (int kk = 0; kk < GKPL; ++kk)
        if (lane + 64 * kk < F) wr[lane + 64 * kk] = acc[r][kk] * a.inv_h;
      if (lane == 0) wr[F] = accs[r] * a.inv_h;
    }
  }
}

template <typename T>
int launch_generic(const TimDesc& d, const void* qkv, int s0, int per_head, float* w, int ld, hipStream_t s,
                   const AttnQuerySrc* qs = nullptr) {
  const int Dh = d.E / d.H;
  const size_t lds = align_up((size_t)d.F * (Dh + (sizeof(T) == 2 ? 2 : 1)) * sizeof(T), 16);
  if (lds > 160 * 1024) return TIMHIP_EUNSUPPORTED;   // (the forward's own limit: a head's keys do not fit the LDS)
  const int rpb = 4 * GROWS;
  MapArgs a{d.S, d.F, d.E, d.H, Dh, 1.f / sqrtf((float)Dh), 1.f / (float)d.H, s0, ld, (d.S - s0 + rpb - 1) / rpb, 0};
  const dim3 grid((unsigned)d.B * (unsigned)a.nblk), block(256);
  if (qs) {
    if (per_head) {
      (void)hipFuncSetAttribute((const void*)attn_w_generic<T, true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      hipLaunchKernelGGL((attn_w_generic<T, true, true>), grid, block, lds, s, (const T*)qkv, w, a, *qs);
    } else {
      (void)hipFuncSetAttribute((const void*)attn_w_generic<T, false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      hipLaunchKernelGGL((attn_w_generic<T, false, true>), grid, block, lds, s, (const T*)qkv, w, a, *qs);
    }
  } else if (per_head) {
    (void)hipFuncSetAttribute((const void*)attn_w_generic<T, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL((attn_w_generic<T, true>), grid, block, lds, s, (const T*)qkv, w, a, NoSrc{});
  } else {
    (void)hipFuncSetAttribute((const void*)attn_w_generic<T, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL((attn_w_generic<T, false>), grid, block, lds, s, (const T*)qkv, w, a, NoSrc{});
  }
  return hipGetLastError() == hipSuccess ? TIMHIP_OK : TIMHIP_ELAUNCH;
}

}  // namespace

// Every refusal comes before any launch.
int tim_attention_weights(const TimDesc& d, const void* qkv, int s0, int per_head, float* w, int ld, hipStream_t s) {
  if (!qkv || !w) return TIMHIP_EINVAL;
  if (d.B <= 0 || d.S <= 0 || d.F <= 0 || d.F > d.S || d.H <= 0 || d.E <= 0 || d.E % d.H || !valid_precision(d.precision))
    return TIMHIP_EINVAL;
  if (d.p_drop != 0.f) return TIMHIP_EINVAL;   // the reference's weights under dropout are a mask, not a map
  if (s0 < 0 || s0 >= d.S || ld < d.F + 1) return TIMHIP_EINVAL;
  if (((uintptr_t)w & 3) != 0 || ((uintptr_t)qkv & (opsize(d.precision) - 1)) != 0) return TIMHIP_EALIGN;
  if (d.F > 64 * GKPL) return TIMHIP_EUNSUPPORTED;
  // the shapes (and the switch) that send the forward to its matrix-core kernels send this one to its own; 16-byte operand rows
  if (h16_storage(d.precision) && !(d.reserved & TIMHIP_DESC_ATTN_FP32) && (d.E % 8) == 0 && ((uintptr_t)qkv & 15) == 0) {
    const int rc = attn_for_shape(d.E / d.H, (d.F + 31) / 32, [&](auto dh, auto njb) {
      DISPATCH_H16(d.precision, return (launch_mfma<HT, decltype(dh)::value, decltype(njb)::value>(d, qkv, s0, per_head, w, ld, s)));
    });
    if (rc != TIMHIP_EUNSUPPORTED) return rc;
  }
  DISPATCH_T(d.precision, return launch_generic<T>(d, qkv, s0, per_head, w, ld, s));
  return TIMHIP_EINVAL;
}

// d: B = G groups, S = Q rows per group, F = cached keys per window (no relation to S).  Every refusal comes before any launch.
int tim_attention_query_weights(const TimDesc& d, const void* qkv_q, const void* kv, int ldkv, int wrows, int W, const int* widx,
                                int per_head, float* w, int ld, hipStream_t s) {
  if (!qkv_q || !kv || !w) return TIMHIP_EINVAL;
  if (d.B <= 0 || d.S <= 0 || d.F <= 0 || d.H <= 0 || d.E <= 0 || d.E % d.H || !valid_precision(d.precision)) return TIMHIP_EINVAL;
  if (d.p_drop != 0.f || W <= 0 || (!widx && d.B != W)) return TIMHIP_EINVAL;
  if (ld < d.F + 1 || ldkv < 2 * d.E || wrows < d.F) return TIMHIP_EINVAL;
  if (d.F > 64 * GKPL) return TIMHIP_EUNSUPPORTED;
  const size_t ts = opsize(d.precision);
  if (((uintptr_t)w & 3) != 0 || (((uintptr_t)qkv_q | (uintptr_t)kv) & (ts - 1)) != 0) return TIMHIP_EALIGN;
  const AttnQuerySrc qs{kv, widx, ldkv, wrows, W};
  // (the matrix-core body reads 16-byte chunks: the forward's own condition, tim_attention_query_fwd)
  const bool al16 = (d.E % 8) == 0 && (ldkv % 8) == 0 && (((uintptr_t)qkv_q | (uintptr_t)kv) & 15) == 0;
  if (h16_storage(d.precision) && !(d.reserved & TIMHIP_DESC_ATTN_FP32) && al16) {
    const int rc = attn_for_shape(d.E / d.H, (d.F + 31) / 32, [&](auto dh, auto njb) {
      DISPATCH_H16(d.precision, return (launch_mfma<HT, decltype(dh)::value, decltype(njb)::value>(d, qkv_q, 0, per_head, w, ld, s, &qs)));
    });
    if (rc != TIMHIP_EUNSUPPORTED) return rc;
  }
  DISPATCH_T(d.precision, return launch_generic<T>(d, qkv_q, 0, per_head, w, ld, s, &qs));
  return TIMHIP_EINVAL;
}

extern "C" int timhip_attention_query_weights(const TimDesc* d, const void* qkv_q, const void* kv, int ldkv, int wrows, int W,
                                              const int* widx, int per_head, float* w, int ld, void* stream) {
  if (!d) return TIMHIP_EINVAL;
  return tim_attention_query_weights(*d, qkv_q, kv, ldkv, wrows, W, widx, per_head, w, ld, (hipStream_t)stream);
}

extern "C" int timhip_attention_weights(const TimDesc* d, const void* qkv, int s0, int per_head, float* w, int ld, void* stream) {
  if (!d) return TIMHIP_EINVAL;
  return tim_attention_weights(*d, qkv, s0, per_head, w, ld, (hipStream_t)stream);
}
