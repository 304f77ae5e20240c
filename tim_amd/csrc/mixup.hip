// Mixup of the inputs on the device (utils/mixup.py:4-22; include/timhip.h has the contract):
//   * mixup_draw_kernel: lam ~ Beta(alpha, alpha) and a permutation with its inverse, from philox4x32_7 keyed by the seed and
//     numbered by a device counter the kernel advances itself - a captured step redraws on every replay
//   * mixup_apply_kernel: dst[b] = lam * src[b] + (1 - lam) * src[index[b]] for up to four tensors in one byte-bound pass
//     (the eager form is a gather pass and a lerp pass per tensor); with the inverse permutation it is its own backward
#include "common.h"

namespace {

constexpr int MIX_JOHNK_TRIALS = 64;     // alpha < 1: blocks 0..63
constexpr int MIX_MT_TRIALS = 32;        // alpha >= 1: blocks 0..31 (first variate), 32..63 (second)
constexpr uint64_t MIX_PERM_BLOCK0 = 256;  // the permutation's words start here
constexpr int MIX_DRAW_BITS = 24;        // Philox counter = (draw number << 24) | block

__device__ __forceinline__ double mix_uniform(uint32_t r) { return ((double)r + 0.5) * (1.0 / 4294967296.0); }

// Gamma(alpha) for alpha >= 1 (Marsaglia & Tsang 2000); the trials read blocks block0 .. block0 + MIX_MT_TRIALS - 1
__device__ double mix_gamma(uint64_t seed, uint64_t base, int block0, double alpha) {
  const double d = alpha - 1.0 / 3.0, c = 1.0 / sqrt(9.0 * d);
  for (int t = 0; t < MIX_MT_TRIALS; ++t) {
    const Philox4 r = philox4x32_7(seed, SITE_MIXUP, base | (uint64_t)(block0 + t));
    const double x = sqrt(-2.0 * log(mix_uniform(r.x))) * cos(6.283185307179586476925 * mix_uniform(r.y));
    const double w = 1.0 + c * x, v = w * w * w;
    if (v <= 0.0) continue;
    if (log(mix_uniform(r.z)) < 0.5 * x * x + d - d * v + d * log(v)) return d * v;
  }
  return d;   // (probability < 1e-39, include/timhip.h)
}

__device__ float mix_beta(uint64_t seed, uint64_t base, float alpha_f) {
  if (!(alpha_f > 0.f)) return 1.f;
  const double alpha = (double)alpha_f;
  if (alpha_f < 1.f) {   // Johnk
    const double e = 1.0 / alpha;
    for (int t = 0; t < MIX_JOHNK_TRIALS; ++t) {
      const Philox4 r = philox4x32_7(seed, SITE_MIXUP, base | (uint64_t)t);
      const double X = pow(mix_uniform(r.x), e), Y = pow(mix_uniform(r.y), e);
      if (X + Y <= 1.0) return (float)(X / (X + Y));   // (X + Y > 0: alpha >= TIMHIP_MIXUP_ALPHA_MIN keeps u^(1/alpha) >= 2^-660)
    }
    return 0.5f;   // (probability <= 2^-64)
  }
  const double g1 = mix_gamma(seed, base, 0, alpha), g2 = mix_gamma(seed, base, MIX_MT_TRIALS, alpha);
  return (float)(g1 / (g1 + g2));
}

// one thread per set, ONE block: every thread reads the counter, the barrier, then thread 0 stores its new value.  (The
// swaps run in the output array: a build that kept them in LDS changed the time of a draw + mix + targets call by under 1 us.)
__global__ __launch_bounds__(256) void mixup_draw_kernel(uint64_t seed, unsigned long long* __restrict__ counter, float alpha,
                                                         int B, int n, float* __restrict__ lam, int* __restrict__ perm,
                                                         int* __restrict__ inv) {
  const unsigned long long c0 = *counter;
  __syncthreads();
  if (threadIdx.x == 0) *counter = c0 + (unsigned long long)n;
  for (int s = threadIdx.x; s < n; s += blockDim.x) {
    const uint64_t base = ((uint64_t)c0 + (uint64_t)s) << MIX_DRAW_BITS;
    lam[s] = mix_beta(seed, base, alpha);
    int* p = perm + (size_t)s * B;
    int* q = inv + (size_t)s * B;
    for (int i = 0; i < B; ++i) p[i] = i;
    Philox4 r = {0, 0, 0, 0};
    int have = -1;   // the block whose words r holds
    for (int i = B - 1; i >= 1; --i) {
      if ((i >> 2) != have) { have = i >> 2; r = philox4x32_7(seed, SITE_MIXUP, base | (MIX_PERM_BLOCK0 + (uint64_t)have)); }
      const int k = i & 3;
      const uint32_t w = k == 0 ? r.x : (k == 1 ? r.y : (k == 2 ? r.z : r.w));
      const int j = (int)(((uint64_t)w * (uint64_t)(i + 1)) >> 32);
      const int a = p[i], b = p[j];
      p[i] = b; p[j] = a;
    }
    for (int i = 0; i < B; ++i) q[p[i]] = i;
  }
}

// ---- apply ----------------------------------------------------------------------------------------------------------
struct MixApplyArgs {
  const void* src[TIMHIP_MIXUP_MAX_TENSORS];
  void* dst[TIMHIP_MIXUP_MAX_TENSORS];
  long long elems[TIMHIP_MIXUP_MAX_TENSORS];    // elements of one item
  long long chunks[TIMHIP_MIXUP_MAX_TENSORS];   // 16-byte chunks of one item, the last one possibly short
  long long first[TIMHIP_MIXUP_MAX_TENSORS + 1];  // flat work index of tensor t's first chunk; first[nt] = all of them
  int dtype[TIMHIP_MIXUP_MAX_TENSORS];
  int nt, B;
};

// (products and sum rounded separately: the stated error bound, and the bits of lam * x + (1 - lam) * y in any fp32 restatement)
__device__ __forceinline__ float mix1(float la, float lb, float x, float y) { return __fadd_rn(__fmul_rn(la, x), __fmul_rn(lb, y)); }

template <typename T>
__device__ __forceinline__ void mix_chunk(const T* __restrict__ src, T* __restrict__ dst, long long elems, long long b, long long ib,
                                          long long chunk, float la, float lb) {
  constexpr int V = 16 / (int)sizeof(T);
  const long long e0 = chunk * V;
  const T* x = src + b * elems + e0;
  const T* y = src + ib * elems + e0;
  T* o = dst + b * elems + e0;
  const bool full = e0 + V <= elems;
  if (full && ((((uintptr_t)x) | ((uintptr_t)y) | ((uintptr_t)o)) & 15) == 0) {
    typedef T vecT __attribute__((ext_vector_type(V)));
    const vecT vx = *reinterpret_cast<const vecT*>(x), vy = *reinterpret_cast<const vecT*>(y);
    vecT vo;
#pragma unroll
    for (int k = 0; k < V; ++k) vo[k] = OpT<T>::from_f(mix1(la, lb, OpT<T>::to_f(vx[k]), OpT<T>::to_f(vy[k])));
    *reinterpret_cast<vecT*>(o) = vo;
  } else {   // the tail of an item, or an item off 16-byte alignment
    const int m = full ? V : (int)(elems - e0);
    for (int k = 0; k < m; ++k) o[k] = OpT<T>::from_f(mix1(la, lb, OpT<T>::to_f(x[k]), OpT<T>::to_f(y[k])));
  }
}

// flat work index over (tensor, item, chunk), grid-stride
__global__ __launch_bounds__(256) void mixup_apply_kernel(const MixApplyArgs a, const float* __restrict__ lam,
                                                          const int* __restrict__ index) {
  const float la = lam[0], lb = 1.f - la;
  const long long total = a.first[a.nt], stride = (long long)gridDim.x * blockDim.x;
  for (long long w = (long long)blockIdx.x * blockDim.x + threadIdx.x; w < total; w += stride) {
    int t = 0;
#pragma unroll
    for (int k = 1; k < TIMHIP_MIXUP_MAX_TENSORS; ++k) t += (k < a.nt && w >= a.first[k]) ? 1 : 0;
    const long long r = w - a.first[t], cpi = a.chunks[t];
    long long b, chunk;
    if (((unsigned long long)(r | cpi) >> 32) == 0) {   // (a 32-bit divide wherever it is enough: every product shape)
      b = (long long)((uint32_t)r / (uint32_t)cpi);
      chunk = (long long)((uint32_t)r - (uint32_t)b * (uint32_t)cpi);
    } else {
      b = r / cpi;
      chunk = r - b * cpi;
    }
    const long long ib = (long long)index[b];
    if (a.dtype[t] == TIMHIP_PREC_FP32)
      mix_chunk<float>((const float*)a.src[t], (float*)a.dst[t], a.elems[t], b, ib, chunk, la, lb);
    else if (a.dtype[t] == TIMHIP_PREC_F16)
      mix_chunk<f16_t>((const f16_t*)a.src[t], (f16_t*)a.dst[t], a.elems[t], b, ib, chunk, la, lb);
    else
      mix_chunk<bf16_t>((const bf16_t*)a.src[t], (bf16_t*)a.dst[t], a.elems[t], b, ib, chunk, la, lb);
  }
}

}  // namespace

extern "C" {

int timhip_mixup_draw(uint64_t seed, uint64_t* counter, float alpha, int B, int n, float* lam, int32_t* perm, int32_t* inv,
                      void* stream) {
  if (!counter || !lam || !perm || !inv || B < 1 || B > (1 << 20) || n < 1 || n > 65536) return TIMHIP_EINVAL;
  if (alpha != alpha) return TIMHIP_EINVAL;
  if (alpha > 0.f && (alpha < TIMHIP_MIXUP_ALPHA_MIN || alpha > TIMHIP_MIXUP_ALPHA_MAX)) return TIMHIP_EINVAL;
  hipLaunchKernelGGL(mixup_draw_kernel, dim3(1), dim3(n < 256 ? 64 : 256), 0, (hipStream_t)stream, seed,
                     (unsigned long long*)counter, alpha, B, n, lam, (int*)perm, (int*)inv);
  TIM_CHECK_LAUNCH();
  return TIMHIP_OK;
}

int timhip_mixup_apply(int nt, const void* const* src, void* const* dst, const int64_t* elems, const int32_t* dtype, int B,
                       const float* lam, const int32_t* index, void* stream) {
  if (nt < 1 || nt > TIMHIP_MIXUP_MAX_TENSORS || !src || !dst || !elems || !dtype || B < 1 || !lam || !index) return TIMHIP_EINVAL;
  MixApplyArgs a;
  a.nt = nt;
  a.B = B;
  long long total = 0;
  for (int t = 0; t < TIMHIP_MIXUP_MAX_TENSORS; ++t) {
    a.first[t] = total;
    if (t >= nt) { a.src[t] = nullptr; a.dst[t] = nullptr; a.elems[t] = 0; a.chunks[t] = 1; a.dtype[t] = TIMHIP_PREC_FP32; continue; }
    if (!src[t] || !dst[t] || elems[t] < 1) return TIMHIP_EINVAL;
    if (dtype[t] != TIMHIP_PREC_FP32 && dtype[t] != TIMHIP_PREC_F16 && dtype[t] != TIMHIP_PREC_BF16) return TIMHIP_EINVAL;
    const long long esz = dtype[t] == TIMHIP_PREC_FP32 ? 4 : 2, per = 16 / esz;
    if ((((uintptr_t)src[t]) | ((uintptr_t)dst[t])) & (uintptr_t)(esz - 1)) return TIMHIP_EALIGN;
    if (elems[t] > (1ll << 40) / B) return TIMHIP_EUNSUPPORTED;   // (the flat index stays far inside 63 bits)
    a.src[t] = src[t];
    a.dst[t] = dst[t];
    a.elems[t] = elems[t];
    a.chunks[t] = (elems[t] + per - 1) / per;
    a.dtype[t] = dtype[t];
    total += a.chunks[t] * (long long)B;
  }
  a.first[TIMHIP_MIXUP_MAX_TENSORS] = total;
  for (int t = nt; t < TIMHIP_MIXUP_MAX_TENSORS; ++t) a.first[t] = total;
  // byte-bound: 256 CUs x 8 blocks of 256 threads and a grid-stride loop over the rest
  const long long want = (total + 255) / 256;
  const int blocks = (int)(want > 2048 ? 2048 : want);
  hipLaunchKernelGGL(mixup_apply_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a, lam, (const int*)index);
  TIM_CHECK_LAUNCH();
  return TIMHIP_OK;
}

}  // extern "C"
