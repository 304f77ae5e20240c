// Audio-guided visual attention pooling (AVGA) of the AVE recipe on the device (gfx950): timhip_avga_fwd / timhip_avga_bwd.
//
// One workgroup (4 waves) owns one pooled row r: its S <= 64 cells X[r] : [S, Cv] and the row's audio term g[r] : [S].
//   hv   = relu(X W_video^T + b_video)     [64, H]   never leaves the CU: walked in chunks of 128 hidden columns
//   c    = hv W_v^T                        [64, 64]  one 32 x 32 accumulator tile per wave, summed over the chunks
//   z[s] = sum_j w_h[j] tanh(c[s, j] + g[s]),  alpha = softmax over the S real cells,  out = alpha X
// Both products of a chunk are computed TRANSPOSED (hv^T = W_video X^T, c^T = W_v hv^T): the cell index then lies on the lane
// and the hidden / map index in the accumulator registers, so the bias, the per-cell g[s], the w_h dot and the relu mask are
// per-register work with no cross-lane traffic, and four consecutive hidden columns of a cell pack into one 8-byte LDS store.
// 16-bit precisions: the row's cells are staged once into LDS in the operand dtype (64 x Cv: 128 KiB at Cv = 1024), the weights
// stream from L2 in fragment shape; TIMHIP_PREC_FP32 runs the same schedule on the exact f32 MFMA (32x32x2) with the cells read
// from global memory (a 64 x 1024 fp32 image does not fit).  The weighted sums over the cells (out, and d_alpha of the
// backward) read the fp32 cells, not the staged copies: alpha of a saturated softmax selects one cell exactly.
// Padded cell rows s >= S carry relu(b_video) through hv; they are masked out of the softmax and every gradient (alpha = 0 there).
//
// Backward (parameter gradients only): pass 1 recomputes c and alpha as the forward does, then d_z, d_c = d_z w_h (1 - tanh^2)
// go to an LDS tile; pass 2 walks the hidden chunks again, recomputes hv, forms d_pre = (d_c W_v) * (hv > 0) and the row's
// share of dW_v = d_c^T hv (16-bit: the mask from a split product, av_hidden<SPLIT>).  dW_v and dw_h are reduced over the rows with float atomics; d_pre and an operand-dtype copy of
// the cells are the two [R * S, Cv] intermediates the weight-gradient kernel turns into dW_video / db_video.
#include <type_traits>

#include "mfma_tiles.h"

namespace {

constexpr int AV_THREADS = 256;
constexpr int AV_HC = 128;   // hidden columns per chunk: one 32-column block per wave

struct AvgaArgs {
  const float* X; long long pitch;
  const float* g; int ldg;
  const void* Wvid; int ldwvid;
  const float* bvid;
  const void* Wv; int ldwv;
  const float* wh;
  float* out; int ldo;
  float* alpha; int lda;
  int R, S, Cv;
  // backward
  const float* dout; int lddo;
  const void* WvT; int ldwvt;
  const void* WvidLo; int ldwlo;   // 16-bit: the lo block of the split copy of W_video (W - hi, operand dtype)
  void* XT; void* dpre; void* dgT;
  float* dWv; float* dwh;
  const float* gs;
};

template <typename T> using frag_t = std::conditional_t<sizeof(T) == 2, vec8<T>, float>;

template <typename T>
__device__ __forceinline__ f32x16_t av_mma(frag_t<T> a, frag_t<T> b, f32x16_t c) {
  if constexpr (sizeof(T) == 2) return mfma16<T>(a, b, c);
  else return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ f32x16_t zero16() {
  f32x16_t v;
#pragma unroll
  for (int i = 0; i < 16; ++i) v[i] = 0.f;
  return v;
}

// operand fragment of the lane's row (`row` points at element 0 of row lane & 31) for the contraction step at k0:
// 16-bit: the 8 values k0 + 8 g .. + 7, fp32: the value k0 + g  (g = lane >> 5)
template <typename T>
__device__ __forceinline__ frag_t<T> gfrag(const T* row, int k0, int g, bool ok) {
  if constexpr (sizeof(T) == 2) {
    vec8<T> v;
    if (ok) {
      v = *reinterpret_cast<const vec8<T>*>(row + k0 + 8 * g);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = (T)0.f;
    }
    return v;
  } else {
    return ok ? row[k0 + g] : 0.f;
  }
}

// LDS tiles [64][DH]: 16-bit = the swizzled image of mfma_tiles.h (row and transposing fragment reads both conflict free),
// fp32 = rows padded to DH + 1 words
template <typename T, int DH>
__device__ __forceinline__ frag_t<T> lfrag(const char* tile, int row, int k0, int g) {
  if constexpr (sizeof(T) == 2) return *reinterpret_cast<const vec8<T>*>(tile + tile_off<DH>(row, (k0 >> 3) + g));
  else return reinterpret_cast<const float*>(tile)[row * (DH + 1) + k0 + g];
}
// four consecutive columns c0 .. c0 + 3 (c0 a multiple of 4) of one row
template <typename T, int DH>
__device__ __forceinline__ void lstore4(char* tile, int row, int c0, float v0, float v1, float v2, float v3) {
  if constexpr (sizeof(T) == 2) {
    store4<T>(reinterpret_cast<T*>(tile + tile_off<DH>(row, c0 >> 3) + (c0 & 7) * 2), v0, v1, v2, v3);
  } else {
    float* p = reinterpret_cast<float*>(tile) + row * (DH + 1) + c0;
    p[0] = v0; p[1] = v1; p[2] = v2; p[3] = v3;
  }
}
// fragment of a product that contracts over the tile's ROW index: lane (i = lane & 31 -> column 32 cb + i); both operands of
// such a product come from this function, so the order of the rows inside a step is theirs to share
template <typename T, int DH>
__device__ __forceinline__ frag_t<T> tfrag(const char* tile, int kb, int cb, int lane) {
  if constexpr (sizeof(T) == 2) return tr_frag<DH, T>(tile, kb, cb, lane);
  else return reinterpret_cast<const float*>(tile)[(kb + (lane >> 5)) * (DH + 1) + 32 * cb + (lane & 31)];
}

// staged cells (16-bit): [64][Cv], 16-byte chunk c of row `row` XORed so that the 32 rows of a fragment read spread over the banks
// (NC = Cv / 8 chunks per row is a multiple of 8: a 3-bit XOR never leaves the row; 4 bits only where NC is a multiple of 16)
__device__ __forceinline__ int x_off(int row, int c, int NC) {
  const int x = (NC & 15) == 0 ? (row & 15) : ((row >> 1) & 7);
  return row * (NC << 4) + ((c ^ x) << 4);
}

template <typename T, bool BWD>
struct AvLds {
  static constexpr bool h16 = sizeof(T) == 2;
  static constexpr int HV_BYTES = h16 ? 64 * AV_HC * 2 : 64 * (AV_HC + 1) * 4;
  static constexpr int DC_BYTES = !BWD ? 0 : (h16 ? 64 * 64 * 2 : 64 * 65 * 4);
  static constexpr int SM_BYTES = 640 * 4;   // z parts [4][64], alpha [64], d_alpha [64], d_g parts [4][64]
  // the backward keeps a second image of the cells, X - hi (the lo half of the relu mask's split product), where it fits
  static constexpr bool lo_image(int Cv) { return BWD && h16 && Cv <= 512; }
  static constexpr size_t x_bytes(int Cv) { return h16 ? (size_t)64 * Cv * 2 * (lo_image(Cv) ? 2 : 1) : 0; }
  static constexpr size_t total(int Cv) { return x_bytes(Cv) + HV_BYTES + DC_BYTES + SM_BYTES; }
};

// lo half of 8 consecutive fp32 cells: T(x - T(x)), what the staged copy dropped
template <typename T>
__device__ __forceinline__ vec8<T> lo8(const float* p, bool ok) {
  vec8<T> v;
  if (ok) {
    const float4 a = reinterpret_cast<const float4*>(p)[0], b = reinterpret_cast<const float4*>(p)[1];
    const float x[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (T)(x[e] - (float)(T)x[e]);
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (T)0.f;
  }
  return v;
}

// hv^T block of one wave: rows hrow0 .. hrow0 + 31 of W_video against all 64 cell rows (acc0: cells 0 .. 31, acc1: 32 .. 63)
// SPLIT (16-bit backward): cor0 / cor1 additionally get X_lo W_hi^T + X_hi W_lo^T, the two terms that bring the pre-activation
// to about twice the operand's mantissa - the relu MASK of the backward is taken from acc + cor (rounding X and W alone moves
// pre-activations across zero; every flipped mask bit adds or drops a full-size term of dW_video), hv itself stays acc
template <typename T, bool SPLIT = false>
__device__ __forceinline__ void av_hidden(const AvgaArgs& a, const char* Xs, const float* Xr, int hrow0, int lane, f32x16_t& acc0,
                                          f32x16_t& acc1, f32x16_t* cor0 = nullptr, f32x16_t* cor1 = nullptr) {
  constexpr bool h16 = sizeof(T) == 2;
  constexpr int KS = h16 ? 16 : 2;
  const int l31 = lane & 31, g = lane >> 5, Cv = a.Cv;
  const T* wrow = reinterpret_cast<const T*>(a.Wvid) + (size_t)(hrow0 + l31) * a.ldwvid;
  acc0 = zero16(); acc1 = zero16();
  if constexpr (SPLIT) { *cor0 = zero16(); *cor1 = zero16(); }
  if constexpr (h16) {
    const int NC = Cv >> 3;
    for (int kk = 0; kk < Cv; kk += 4 * KS) {   // Cv is a multiple of 64: whole groups of four steps
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int k0 = kk + u * KS;
        const frag_t<T> wa = gfrag<T>(wrow, k0, g, true);
        const frag_t<T> b0 = *reinterpret_cast<const vec8<T>*>(Xs + x_off(l31, (k0 >> 3) + g, NC));
        const frag_t<T> b1 = *reinterpret_cast<const vec8<T>*>(Xs + x_off(32 + l31, (k0 >> 3) + g, NC));
        acc0 = av_mma<T>(wa, b0, acc0);
        acc1 = av_mma<T>(wa, b1, acc1);
        if constexpr (SPLIT) {
          const T* wlrow = reinterpret_cast<const T*>(a.WvidLo) + (size_t)(hrow0 + l31) * a.ldwlo;
          const frag_t<T> wl = gfrag<T>(wlrow, k0, g, true);
          frag_t<T> l0, l1;
          if (AvLds<T, true>::lo_image(Cv)) {
            const char* Xl = Xs + (size_t)64 * Cv * 2;
            l0 = *reinterpret_cast<const vec8<T>*>(Xl + x_off(l31, (k0 >> 3) + g, NC));
            l1 = *reinterpret_cast<const vec8<T>*>(Xl + x_off(32 + l31, (k0 >> 3) + g, NC));
          } else {
            l0 = lo8<T>(Xr + (size_t)l31 * Cv + k0 + 8 * g, l31 < a.S);
            l1 = lo8<T>(Xr + (size_t)(32 + l31) * Cv + k0 + 8 * g, 32 + l31 < a.S);
          }
          *cor0 = av_mma<T>(wl, b0, *cor0); *cor0 = av_mma<T>(wa, l0, *cor0);
          *cor1 = av_mma<T>(wl, b1, *cor1); *cor1 = av_mma<T>(wa, l1, *cor1);
        }
      }
    }
  } else {
    const float* x0 = Xr + (size_t)l31 * Cv;
    const float* x1 = Xr + (size_t)(32 + l31) * Cv;
    const bool ok0 = l31 < a.S, ok1 = 32 + l31 < a.S;
    for (int kk = 0; kk < Cv; kk += 8 * KS) {
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int k0 = kk + u * KS;
        const float wa = gfrag<float>(reinterpret_cast<const float*>(wrow), k0, g, true);
        acc0 = av_mma<float>(wa, gfrag<float>(x0, k0, g, ok0), acc0);
        acc1 = av_mma<float>(wa, gfrag<float>(x1, k0, g, ok1), acc1);
      }
    }
  }
}

// bias + relu of the wave's hv^T block into the chunk tile; returns the (hv > 0) bits (bit 16 sb + reg)
template <typename T>
__device__ __forceinline__ uint32_t av_hidden_store(const AvgaArgs& a, char* hvs, int hc, int w, int lane, const f32x16_t& acc0,
                                                    const f32x16_t& acc1, const f32x16_t* cor0 = nullptr,
                                                    const f32x16_t* cor1 = nullptr) {
  const int l31 = lane & 31, g = lane >> 5;
  uint32_t pos = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int h0 = w * 32 + 8 * q + 4 * g;   // column inside the chunk
    const float4 b4 = *reinterpret_cast<const float4*>(a.bvid + hc * AV_HC + h0);
    const float bb[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
    for (int sb = 0; sb < 2; ++sb) {
      float v[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float pre = (sb ? acc1[4 * q + i] : acc0[4 * q + i]) + bb[i];
        v[i] = fmaxf(pre, 0.f);
        const float mpre = cor0 != nullptr ? pre + (sb ? (*cor1)[4 * q + i] : (*cor0)[4 * q + i]) : pre;
        if (mpre > 0.f) pos |= 1u << (16 * sb + 4 * q + i);
      }
      lstore4<T, AV_HC>(hvs, sb * 32 + l31, h0, v[0], v[1], v[2], v[3]);
    }
  }
  return pos;
}

template <typename T, bool BWD>
__global__ __launch_bounds__(AV_THREADS) void avga_kernel(const AvgaArgs a) {
  extern __shared__ __attribute__((aligned(16))) char av_lds[];
  using Lay = AvLds<T, BWD>;
  constexpr bool h16 = sizeof(T) == 2;
  constexpr int KS = h16 ? 16 : 2;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l31 = lane & 31, g = lane >> 5;
  const int wj = w & 1, ws = w >> 1;   // the wave's 32 x 32 tile of c^T: map rows 32 wj .., cells 32 ws ..
  const int r = blockIdx.x, S = a.S, Cv = a.Cv, H = Cv;
  char* Xs = av_lds;
  char* hvs = Xs + Lay::x_bytes(Cv);
  char* dcs = hvs + Lay::HV_BYTES;
  float* sm = reinterpret_cast<float*>(dcs + Lay::DC_BYTES);
  float* zpart = sm; float* alpha_s = sm + 256; float* dal_s = sm + 320; float* dgp = sm + 384;
  const float* Xr = a.X + (size_t)r * a.pitch;
  (void)dal_s; (void)dgp;

  // ---- the row's cells: fp32 -> operand dtype, once (16-bit: into LDS; backward: also the [R * S, Cv] copy) ----
  if constexpr (h16) {
    const int NC = Cv >> 3, nreal = S * NC;
    constexpr int UN = 4;
    for (int i0 = tid; i0 < nreal; i0 += AV_THREADS * UN) {
      float4 lo[UN], hi[UN];
#pragma unroll
      for (int u = 0; u < UN; ++u) {
        const int idx = i0 + u * AV_THREADS;
        if (idx < nreal) {
          const float4* p = reinterpret_cast<const float4*>(Xr + (size_t)idx * 8);
          lo[u] = p[0]; hi[u] = p[1];
        }
      }
#pragma unroll
      for (int u = 0; u < UN; ++u) {
        const int idx = i0 + u * AV_THREADS;
        if (idx < nreal) {
          vec8<T> v;
          v[0] = (T)lo[u].x; v[1] = (T)lo[u].y; v[2] = (T)lo[u].z; v[3] = (T)lo[u].w;
          v[4] = (T)hi[u].x; v[5] = (T)hi[u].y; v[6] = (T)hi[u].z; v[7] = (T)hi[u].w;
          const int row = idx / NC, c = idx - row * NC;
          *reinterpret_cast<vec8<T>*>(Xs + x_off(row, c, NC)) = v;
          if constexpr (BWD) {
            *reinterpret_cast<vec8<T>*>(reinterpret_cast<T*>(a.XT) + ((size_t)r * S * Cv + (size_t)idx * 8)) = v;
            if (Lay::lo_image(Cv)) {
              const float x[8] = {lo[u].x, lo[u].y, lo[u].z, lo[u].w, hi[u].x, hi[u].y, hi[u].z, hi[u].w};
              vec8<T> l;
#pragma unroll
              for (int e = 0; e < 8; ++e) l[e] = (T)(x[e] - (float)v[e]);
              *reinterpret_cast<vec8<T>*>(Xs + (size_t)64 * Cv * 2 + x_off(row, c, NC)) = l;
            }
          }
        }
      }
    }
    vec8<T> zv;
#pragma unroll
    for (int e = 0; e < 8; ++e) zv[e] = (T)0.f;
    for (int idx = nreal + tid; idx < 64 * NC; idx += AV_THREADS) {
      const int row = idx / NC, c = idx - row * NC;
      *reinterpret_cast<vec8<T>*>(Xs + x_off(row, c, NC)) = zv;
      if (Lay::lo_image(Cv)) *reinterpret_cast<vec8<T>*>(Xs + (size_t)64 * Cv * 2 + x_off(row, c, NC)) = zv;
    }
  } else if constexpr (BWD) {
    float4* dst = reinterpret_cast<float4*>(reinterpret_cast<float*>(a.XT) + (size_t)r * S * Cv);
    for (int i = tid; i < S * (Cv >> 2); i += AV_THREADS) dst[i] = reinterpret_cast<const float4*>(Xr)[i];
  }

  // w_h of the 16 map rows this lane holds in its c^T registers (0 past the map)
  float whr[16];
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    const int j = wj * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * g;
    whr[reg] = j < S ? a.wh[j] : 0.f;
  }
  lds_barrier();

  // ---- pass 1: c^T over the hidden chunks ----
  const int nchunks = (H + AV_HC - 1) / AV_HC;
  f32x16_t accc = zero16();
  const int jrow = wj * 32 + l31;   // W_v row of this lane's A fragment
  const T* vrow = reinterpret_cast<const T*>(a.Wv) + (size_t)jrow * a.ldwv;
  for (int hc = 0; hc < nchunks; ++hc) {
    const int nhb = min(4, (H - hc * AV_HC) / 32);   // 32-column blocks of this chunk (H is a multiple of 64: 4 or 2)
    f32x16_t acc0, acc1;
    if (w < nhb) av_hidden<T>(a, Xs, Xr, hc * AV_HC + w * 32, lane, acc0, acc1);
    lds_barrier();   // the previous chunk's reads of the tile are done
    if (w < nhb) av_hidden_store<T>(a, hvs, hc, w, lane, acc0, acc1);
    lds_barrier();
    const int kw = nhb * 32;
    for (int kk = 0; kk < kw; kk += 4 * KS) {   // kw is 64 or 128
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int k0 = kk + u * KS;
        accc = av_mma<T>(gfrag<T>(vrow + hc * AV_HC, k0, g, jrow < S), lfrag<T, AV_HC>(hvs, ws * 32 + l31, k0, g), accc);
      }
    }
  }

  // ---- z, softmax over the real cells ----
  const int s_own = ws * 32 + l31;
  const float g_s = s_own < S ? a.g[(size_t)r * a.ldg + s_own] : 0.f;
  float th[16];
  float zp = 0.f;
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    th[reg] = tanhf(accc[reg] + g_s);
    zp = fmaf(whr[reg], th[reg], zp);
  }
  zpart[(wj * 2 + g) * 64 + s_own] = zp;
  lds_barrier();
  {
    const float z = (zpart[lane] + zpart[64 + lane]) + (zpart[128 + lane] + zpart[192 + lane]);
    const bool real = lane < S;
    const float zmax = wave_max(real ? z : -INFINITY);
    const float e = real ? expf(z - zmax) : 0.f;
    const float al = e / wave_sum(e);
    if (w == 0) {
      alpha_s[lane] = al;
      if (a.alpha != nullptr && real) a.alpha[(size_t)r * a.lda + lane] = al;
    }
  }
  lds_barrier();
  const int nc4 = Cv >> 2;

  if constexpr (!BWD) {
    // ---- out = alpha X from the fp32 cells: column quads x groups of cells, partial sums through LDS in a fixed order ----
    float4* red = reinterpret_cast<float4*>(hvs);
    const int nparts = nc4 >= AV_THREADS ? 1 : AV_THREADS / nc4;
    const int c4 = tid % nc4, part = tid / nc4;
    if (part < nparts) {
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int s = part; s < S; s += nparts) {
        const float al = alpha_s[s];
        const float4 x = reinterpret_cast<const float4*>(Xr + (size_t)s * Cv)[c4];
        acc.x = fmaf(al, x.x, acc.x); acc.y = fmaf(al, x.y, acc.y); acc.z = fmaf(al, x.z, acc.z); acc.w = fmaf(al, x.w, acc.w);
      }
      red[part * nc4 + c4] = acc;
    }
    lds_barrier();
    if (tid < nc4) {
      float4 acc = red[tid];
      for (int p = 1; p < nparts; ++p) {
        const float4 v = red[p * nc4 + tid];
        acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
      }
      reinterpret_cast<float4*>(a.out + (size_t)r * a.ldo)[tid] = acc;
    }
  } else {
    // ---- d_alpha[s] = d_out . X[s] (fp32 cells, one wave per cell), d_z, d_c ----
    const float* dor = a.dout + (size_t)r * a.lddo;
    for (int s = w; s < S; s += 4) {
      float p = 0.f;
      for (int c4 = lane; c4 < nc4; c4 += 64) {
        const float4 x = reinterpret_cast<const float4*>(Xr + (size_t)s * Cv)[c4];
        const float4 d = reinterpret_cast<const float4*>(dor)[c4];
        p = fmaf(x.x, d.x, p); p = fmaf(x.y, d.y, p); p = fmaf(x.z, d.z, p); p = fmaf(x.w, d.w, p);
      }
      p = wave_sum(p);
      if (lane == 0) dal_s[s] = p;
    }
    if (tid >= S && tid < 64) dal_s[tid] = 0.f;
    lds_barrier();
    const float adot = wave_sum(lane < S ? alpha_s[lane] * dal_s[lane] : 0.f);
    const float dz = s_own < S ? alpha_s[s_own] * (dal_s[s_own] - adot) : 0.f;
    const float gsc = a.gs != nullptr ? a.gs[0] : 1.f, ginv = a.gs != nullptr ? a.gs[1] : 1.f;
    float chk = 0.f;
    float dgl = 0.f;
    float dcv[16];
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      dcv[reg] = dz * whr[reg] * (1.f - th[reg] * th[reg]);
      dgl += dcv[reg];
    }
    dgp[(wj * 2 + g) * 64 + s_own] = dgl;
    // dw_h[j] += sum over the cells (the 32 lanes of a half wave) of d_z tanh
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      float v = dz * th[reg];
      v += __shfl_xor(v, 1); v += __shfl_xor(v, 2); v += __shfl_xor(v, 4); v += __shfl_xor(v, 8); v += __shfl_xor(v, 16);
      const int j = wj * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * g;
      if (l31 == 0 && j < S) {
        nf_note(chk, v);
        unsafeAtomicAdd(a.dwh + j, v);
      }
    }
    // d_c as the operand of pass 2 (fp16: under the gradient scale)
#pragma unroll
    for (int q = 0; q < 4; ++q)
      lstore4<T, 64>(dcs, s_own, wj * 32 + 8 * q + 4 * g, gsc * dcv[4 * q], gsc * dcv[4 * q + 1], gsc * dcv[4 * q + 2],
                     gsc * dcv[4 * q + 3]);
    lds_barrier();
    if (tid < 64) {
      const float dg = (dgp[tid] + dgp[64 + tid]) + (dgp[128 + tid] + dgp[192 + tid]);
      reinterpret_cast<T*>(a.dgT)[(size_t)r * 64 + tid] = OpT<T>::from_f(gsc * dg);
    }

    // ---- pass 2: per chunk hv again, d_pre = (d_c W_v) * (hv > 0), dW_v += d_c^T hv ----
    T* dpre = reinterpret_cast<T*>(a.dpre) + (size_t)r * S * Cv;
    for (int hc = 0; hc < nchunks; ++hc) {
      const int nhb = min(4, (H - hc * AV_HC) / 32);
      f32x16_t acc0, acc1, cor0, cor1;
      uint32_t pos = 0;
      if (w < nhb) av_hidden<T, h16>(a, Xs, Xr, hc * AV_HC + w * 32, lane, acc0, acc1, &cor0, &cor1);
      lds_barrier();
      if (w < nhb) pos = av_hidden_store<T>(a, hvs, hc, w, lane, acc0, acc1, h16 ? &cor0 : nullptr, h16 ? &cor1 : nullptr);
      lds_barrier();
      if (w < nhb) {
        const int hcol0 = hc * AV_HC + w * 32;
        // d_hv^T block: rows = hidden columns of the wave's block (W_v^T rows), columns = cells
        const T* trow = reinterpret_cast<const T*>(a.WvT) + (size_t)(hcol0 + l31) * a.ldwvt;
        f32x16_t d0 = zero16(), d1 = zero16();
#pragma unroll 2
        for (int j0 = 0; j0 < 64; j0 += KS) {
          const frag_t<T> ta = gfrag<T>(trow, j0, g, true);
          d0 = av_mma<T>(ta, lfrag<T, 64>(dcs, l31, j0, g), d0);
          d1 = av_mma<T>(ta, lfrag<T, 64>(dcs, 32 + l31, j0, g), d1);
        }
#pragma unroll
        for (int sb = 0; sb < 2; ++sb) {
          const int s = sb * 32 + l31;
          if (s < S) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              float v[4];
#pragma unroll
              for (int i = 0; i < 4; ++i)
                v[i] = (pos >> (16 * sb + 4 * q + i)) & 1u ? (sb ? d1[4 * q + i] : d0[4 * q + i]) : 0.f;
              store4<T>(dpre + (size_t)s * Cv + hcol0 + 8 * q + 4 * g, v[0], v[1], v[2], v[3]);
            }
          }
        }
        // the row's share of dW_v[j, hcol0 + lane & 31]: contraction over the 64 cell rows of both tiles (padded cells: d_c = 0)
        for (int jb = 0; jb < (S > 32 ? 2 : 1); ++jb) {
          f32x16_t dw = zero16();
#pragma unroll 2
          for (int kb = 0; kb < 64; kb += KS)
            dw = av_mma<T>(tfrag<T, 64>(dcs, kb, jb, lane), tfrag<T, AV_HC>(hvs, kb, w, lane), dw);
#pragma unroll
          for (int reg = 0; reg < 16; ++reg) {
            const int j = jb * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * g;
            if (j < S) {
              const float v = dw[reg] * ginv;
              nf_note(chk, v);
              unsafeAtomicAdd(a.dWv + (size_t)j * H + hcol0 + l31, v);
            }
          }
        }
      }
    }
    nf_commit(a.gs != nullptr ? a.gs + 1 : nullptr, chk);
  }
}

// zero fill of an accumulated-into gradient as a kernel of the same stream (a captured step replays it like any other launch)
__global__ void avga_zero_kernel(float* p, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = 0.f;
}
int av_zero(float* p, size_t n, hipStream_t s) {
  const size_t blocks = (n + 255) / 256;
  hipLaunchKernelGGL(avga_zero_kernel, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, s, p, n);
  TIM_CHECK_LAUNCH();
  return TIMHIP_OK;
}

// the audio rows fp32 [R, lda >= Ca] (any row stride, 4-byte alignment) as the operand [R, Kap] (zero padded) and, when `split`
// is given, as the split operand [hi | lo | hi] of 3 Kap columns (what timhip_split3_many writes in mode 0)
template <typename T>
__global__ void avga_audio_kernel(const float* a, long long lda, int R, int Ca, int Kap, T* plain, T* split) {
  const long long n = (long long)R * Kap;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const long long r = i / Kap;
    const int k = (int)(i - r * Kap);
    const float x = k < Ca ? a[r * lda + k] : 0.f;
    const T hi = OpT<T>::from_f(x);
    plain[i] = hi;
    if (split != nullptr) {
      T* q = split + r * 3 * Kap + k;
      q[0] = hi; q[Kap] = OpT<T>::from_f(x - OpT<T>::to_f(hi)); q[2 * Kap] = hi;
    }
  }
}
int av_audio(int precision, const TimAvga* p, void* plain, void* split, hipStream_t s) {
  const int Kap = round_up(p->Ca, 64);
  const long long n = (long long)p->R * Kap;
  const unsigned blocks = (unsigned)((n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048);
  DISPATCH_T(precision, hipLaunchKernelGGL(avga_audio_kernel<T>, dim3(blocks), dim3(256), 0, s, p->audio, (long long)p->ld_audio, p->R,
                                           p->Ca, Kap, (T*)plain, (T*)split));
  TIM_CHECK_LAUNCH();
  return TIMHIP_OK;
}

template <typename T, bool BWD>
int av_launch(const AvgaArgs& a, hipStream_t s) {
  static PerDeviceOnce once;
  if (once.first() &&
      hipFuncSetAttribute(reinterpret_cast<const void*>(&avga_kernel<T, BWD>), hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)(AvLds<T, BWD>::total(512) > AvLds<T, BWD>::total(1024) ? AvLds<T, BWD>::total(512) : AvLds<T, BWD>::total(1024))) != hipSuccess)
    return TIMHIP_ELAUNCH;
  const size_t shmem = AvLds<T, BWD>::total(a.Cv);
  hipLaunchKernelGGL((avga_kernel<T, BWD>), dim3(a.R), dim3(AV_THREADS), shmem, s, a);
  TIM_CHECK_LAUNCH();
  return TIMHIP_OK;
}

// workspace: the audio side's [R]-row operands, the row's audio term g, and (backward) the two [R * S, Cv] operands of dW_video
struct AvgaWs { Field aT, haT, g, xT, dpre, dgT, dpaT, a3, haM, wg; size_t total; };

AvgaWs avga_ws(int prec, int R, int S, int Cv, int Ca, int backward) {
  const size_t ts = opsize(prec), H = Cv;
  Arena ar;
  AvgaWs w{};
  w.aT = ar.take((size_t)R * round_up(Ca, 64) * ts);
  w.haT = ar.take((size_t)R * H * ts);
  w.g = ar.take((size_t)R * 64 * 4);
  if (backward) {
    w.xT = ar.take((size_t)R * S * Cv * ts);
    w.dpre = ar.take((size_t)R * S * Cv * ts);
    w.dgT = ar.take((size_t)R * 64 * ts);
    w.dpaT = ar.take((size_t)R * H * ts);
    if (h16_storage(prec)) {   // the audio side's relu mask from a split product: a as [hi | lo | hi], ha again at ~2x the mantissa
      w.a3 = ar.take((size_t)R * 3 * round_up(Ca, 64) * ts);
      w.haM = ar.take((size_t)R * H * ts);
    }
    size_t wg = timhip_wgrad_workspace_bytes(prec, (int)H, Cv, R * S);
    const size_t wg2 = timhip_wgrad_workspace_bytes(prec, S, (int)H, R), wg3 = timhip_wgrad_workspace_bytes(prec, (int)H, Ca, R);
    wg = wg > wg2 ? wg : wg2;
    wg = wg > wg3 ? wg : wg3;
    w.wg = ar.take(wg > 256 ? wg : 256);
  }
  w.total = ar.total();
  return w;
}

int avga_check(int precision, const TimAvga* p, int backward) {
  if (!p || !p->video || !p->audio || !p->w_video || !p->w_audio || !p->w_v || !p->w_g || !p->b_video || !p->b_audio || !p->w_h)
    return TIMHIP_EINVAL;
  if (backward && (!p->w_v_t || !p->w_g_t)) return TIMHIP_EINVAL;
  if (p->R < 1 || p->S < 1 || p->Cv < 1 || p->Ca < 1 || p->H < 1) return TIMHIP_EINVAL;
  if (precision != TIMHIP_PREC_BF16 && precision != TIMHIP_PREC_F16 && precision != TIMHIP_PREC_FP32) return TIMHIP_EUNSUPPORTED;
  if (p->S > 64 || p->S != p->map_size || p->H != p->Cv || p->Cv % 64 || p->Cv > 1024) return TIMHIP_EUNSUPPORTED;
  if ((unsigned long long)p->R * p->S * p->Cv >= (1ull << 31)) return TIMHIP_EUNSUPPORTED;   // 32-bit offsets into the [R * S, Cv] operands
  if (p->pitch < (long long)p->S * p->Cv || p->ld_audio < p->Ca) return TIMHIP_EINVAL;
  const int Kv = p->Cv, Ka = round_up(p->Ca, 64);
  if (p->pitch % 4 || p->ld_w_video % 64 || p->ld_w_video < Kv || p->ld_w_audio % 64 || p->ld_w_audio < Ka ||
      p->ld_w_v % 64 || p->ld_w_v < Kv || p->ld_w_g % 64 || p->ld_w_g < Kv)
    return TIMHIP_EALIGN;
  if (backward && (p->ld_w_v_t % 64 || p->ld_w_v_t < 64 || p->ld_w_g_t % 64 || p->ld_w_g_t < 64)) return TIMHIP_EALIGN;
  if (backward && h16_storage(precision)) {   // the split copies [hi | hi | lo] of W_video and W_audio
    if (!p->w_video_s || !p->w_audio_s) return TIMHIP_EINVAL;
    if (p->ld_w_video_s != 3 * Kv || p->ld_w_audio_s != 3 * Ka ||   // three blocks of ru(K) columns, nothing between them
        (((uintptr_t)p->w_video_s | (uintptr_t)p->w_audio_s) & 15))
      return TIMHIP_EALIGN;
  }
  if ((uintptr_t)p->audio & 3) return TIMHIP_EALIGN;
  uintptr_t bits = (uintptr_t)p->video | (uintptr_t)p->w_video | (uintptr_t)p->w_audio | (uintptr_t)p->w_v |
                   (uintptr_t)p->w_g | (uintptr_t)p->b_video | (uintptr_t)p->b_audio;
  if (backward) bits |= (uintptr_t)p->w_v_t | (uintptr_t)p->w_g_t;
  if (bits & 15) return TIMHIP_EALIGN;
  return TIMHIP_OK;
}

// ha = relu(a W_audio^T + b_audio) and g = ha W_g^T: [R]-row products in front of the fused kernel
int avga_audio_side(int precision, const TimAvga* p, const AvgaWs& W, char* ws, bool backward, hipStream_t s) {
  const int R = p->R, H = p->H, Kap = round_up(p->Ca, 64);
  int rc = av_audio(precision, p, W.aT.at(ws), backward && h16_storage(precision) ? W.a3.at(ws) : nullptr, s);
  if (rc) return rc;
  TimEpi e{};
  e.out0 = W.haT.at(ws); e.ld0 = H; e.bias = p->b_audio;
  if ((rc = tim_gemm_nt(precision, TIMHIP_EPI_RELU_T, W.aT.at(ws), Kap, p->w_audio, p->ld_w_audio, R, H, p->Ca, e, 1, s))) return rc;
  TimEpi e2{};
  e2.out0 = W.g.at(ws); e2.ld0 = 64;
  return tim_gemm_nt(precision, TIMHIP_EPI_STORE_F32, W.haT.at(ws), H, p->w_g, p->ld_w_g, R, p->S, H, e2, 1, s);
}

AvgaArgs avga_args(const TimAvga* p, const AvgaWs& W, char* ws) {
  AvgaArgs a{};
  a.X = p->video; a.pitch = p->pitch;
  a.g = (const float*)W.g.at(ws); a.ldg = 64;
  a.Wvid = p->w_video; a.ldwvid = p->ld_w_video; a.bvid = p->b_video;
  a.Wv = p->w_v; a.ldwv = p->ld_w_v; a.wh = p->w_h;
  a.R = p->R; a.S = p->S; a.Cv = p->Cv;
  return a;
}

}  // namespace

extern "C" {

size_t timhip_avga_workspace_bytes(int precision, int R, int S, int Cv, int Ca, int backward) {
  if ((unsigned long long)(R < 1 ? 1 : R) * (S < 1 ? 1 : S) * (Cv < 1 ? 1 : Cv) >= (1ull << 31)) return 0;
  if (!valid_precision(precision) || precision == TIMHIP_PREC_BF16X3 || R < 1 || S < 1 || S > 64 || Cv < 64 || Cv > 1024 || Cv % 64 || Ca < 1) return 0;
  return avga_ws(precision, R, S, Cv, Ca, backward).total;
}

int timhip_avga_fwd(int precision, const TimAvga* p, float* out, int ldo, float* alpha, int ld_alpha, void* workspace,
                    size_t workspace_bytes, void* stream) {
  if (!out || !workspace) return TIMHIP_EINVAL;
  int rc = avga_check(precision, p, 0);
  if (rc) return rc;
  if (ldo < p->Cv || (alpha && ld_alpha < p->S)) return TIMHIP_EINVAL;
  if (ldo % 4 || (((uintptr_t)out | (uintptr_t)workspace) & 15)) return TIMHIP_EALIGN;
  const AvgaWs W = avga_ws(precision, p->R, p->S, p->Cv, p->Ca, 0);
  if (workspace_bytes < W.total) return TIMHIP_EWORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  if ((rc = avga_audio_side(precision, p, W, ws, false, s))) return rc;
  AvgaArgs a = avga_args(p, W, ws);
  a.out = out; a.ldo = ldo; a.alpha = alpha; a.lda = ld_alpha;
  DISPATCH_T(precision, rc = av_launch<T, false>(a, s));
  return rc;
}

int timhip_avga_bwd(int precision, const TimAvga* p, const float* d_out, int ldd, const TimAvgaGrads* gr, const float* grad_scale,
                    void* workspace, size_t workspace_bytes, void* stream) {
  if (!d_out || !workspace || !gr || !gr->w_video || !gr->b_video || !gr->w_audio || !gr->b_audio || !gr->w_v || !gr->w_g || !gr->w_h)
    return TIMHIP_EINVAL;
  int rc = avga_check(precision, p, 1);
  if (rc) return rc;
  if (ldd < p->Cv) return TIMHIP_EINVAL;
  if (ldd % 4 || (((uintptr_t)d_out | (uintptr_t)workspace) & 15)) return TIMHIP_EALIGN;
  if (grad_scale && precision != TIMHIP_PREC_F16) return TIMHIP_EINVAL;
  const int R = p->R, S = p->S, Cv = p->Cv, H = p->H, Ca = p->Ca, Kap = round_up(Ca, 64);
  const AvgaWs W = avga_ws(precision, R, S, Cv, Ca, 1);
  if (workspace_bytes < W.total) return TIMHIP_EWORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  if ((rc = avga_audio_side(precision, p, W, ws, true, s))) return rc;
  // reduced with atomics by the fused kernel
  if ((rc = av_zero(gr->w_v, (size_t)S * H, s)) || (rc = av_zero(gr->w_h, (size_t)S, s))) return rc;
  AvgaArgs a = avga_args(p, W, ws);
  a.dout = d_out; a.lddo = ldd;
  a.WvT = p->w_v_t; a.ldwvt = p->ld_w_v_t;
  if (h16_storage(precision)) {   // lo block: the third of [hi | hi | lo], each Cv = ld / 3 wide (avga_check)
    a.WvidLo = (const char*)p->w_video_s + (size_t)2 * Cv * 2;
    a.ldwlo = p->ld_w_video_s;
  }
  a.XT = W.xT.at(ws); a.dpre = W.dpre.at(ws); a.dgT = W.dgT.at(ws);
  a.dWv = gr->w_v; a.dwh = gr->w_h; a.gs = grad_scale;
  DISPATCH_T(precision, rc = av_launch<T, true>(a, s));
  if (rc) return rc;
  const float* gs_out = grad_scale ? grad_scale + 1 : nullptr;
  // d(pre-activation of affine_audio) = (d_g W_g) * (ha > 0)
  const void* ha_mask = W.haT.at(ws);
  if (h16_storage(precision)) {   // ha once more from split operands, for its sign only (see av_hidden<SPLIT>)
    TimEpi em{};
    em.out0 = W.haM.at(ws); em.ld0 = H; em.bias = p->b_audio; em.reserved = 3;
    if ((rc = tim_gemm_nt(precision, TIMHIP_EPI_RELU_T, W.a3.at(ws), 3 * Kap, p->w_audio_s, p->ld_w_audio_s, R, H, 3 * Kap, em, 1, s))) return rc;
    ha_mask = W.haM.at(ws);
  }
  TimEpi e{};
  e.out0 = W.dpaT.at(ws); e.ld0 = H; e.aux = ha_mask; e.ldaux = H;
  if ((rc = tim_gemm_nt(precision, TIMHIP_EPI_DRELU_T, W.dgT.at(ws), 64, p->w_g_t, p->ld_w_g_t, R, H, S, e, 1, s))) return rc;
  struct Prod { const void* dY; int ldy, Nout; const void* X; int ldx, Kout, M; float* dW; float* db; };
  const Prod prods[3] = {{W.dpre.at(ws), Cv, H, W.xT.at(ws), Cv, Cv, R * S, gr->w_video, gr->b_video},
                         {W.dgT.at(ws), 64, S, W.haT.at(ws), H, H, R, gr->w_g, nullptr},
                         {W.dpaT.at(ws), H, H, W.aT.at(ws), Kap, Ca, R, gr->w_audio, gr->b_audio}};
  for (const Prod& q : prods) {
    if (h16_storage(precision)) {
      rc = tim_wgrad_tn_h16(precision, q.dY, q.ldy, q.Nout, q.X, q.ldx, q.Kout, q.M, q.dW, q.db, W.wg.at(ws), W.wg.bytes, s, 0, gs_out);
    } else {   // the fp32 route accumulates
      if ((rc = av_zero(q.dW, (size_t)q.Nout * q.Kout, s))) return rc;
      if (q.db && (rc = av_zero(q.db, (size_t)q.Nout, s))) return rc;
      rc = timhip_wgrad(precision, q.dY, q.ldy, q.Nout, q.X, q.ldx, q.Kout, q.M, q.dW, q.db, W.wg.at(ws), W.wg.bytes, nullptr, s);
    }
    if (rc) return rc;
  }
  return TIMHIP_OK;
}

}  // extern "C"
