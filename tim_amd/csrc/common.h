// Shared device/host helpers for libtimhip (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/timhip.h"

// 16-bit MFMA operand types: HT = bf16_t (TIMHIP_PREC_BF16) or f16_t (TIMHIP_PREC_F16).  Every 16-bit kernel is a template
// over H; the two differ in the MFMA opcode and the f32 <-> H conversions only (same fragment layouts, same LDS images).
typedef __bf16 bf16_t;
typedef _Float16 f16_t;
template <typename T> using vec8 = T __attribute__((ext_vector_type(8)));
template <typename T> using vec4 = T __attribute__((ext_vector_type(4)));
typedef vec8<bf16_t> bf16x8_t;
typedef vec4<bf16_t> bf16x4_t;
typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef float f32x16_t __attribute__((ext_vector_type(16)));
typedef short s16x4_t __attribute__((ext_vector_type(4)));

#define TIM_CHECK_LAUNCH()                                   \
  do {                                                       \
    if (hipGetLastError() != hipSuccess) return TIMHIP_ELAUNCH; \
  } while (0)

static inline int round_up(int x, int m) { return (x + m - 1) / m * m; }
__host__ __device__ static inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// Byte layouts of the library's blocks (a layer's saved block, its workspaces, the evaluation arena): the fields lie back to
// back in the order they are taken, each on a 256-byte boundary; a layout keeps the Field (where, how many bytes) of each.
struct Field {
  size_t off, bytes;
  char* at(void* base) const { return (char*)base + off; }
  const char* at(const void* base) const { return (const char*)base + off; }
};
struct Arena {
  size_t off = 0;
  Field take(size_t bytes) { const Field f{off, bytes}; off = align_up(off + bytes, 256); return f; }
  size_t total() const { return off; }
};

// ----------------------------------------------------------------------------
// operand-type traits
// ----------------------------------------------------------------------------
template <typename T> struct OpT;
template <> struct OpT<float> {
  static __device__ __forceinline__ float to_f(float v) { return v; }
  static __device__ __forceinline__ float from_f(float v) { return v; }
};
template <> struct OpT<bf16_t> {
  static __device__ __forceinline__ float to_f(bf16_t v) { return (float)v; }
  static __device__ __forceinline__ bf16_t from_f(float v) { return (bf16_t)v; }
};

template <> struct OpT<f16_t> {
  static __device__ __forceinline__ float to_f(f16_t v) { return (float)v; }
  static __device__ __forceinline__ f16_t from_f(float v) { return (f16_t)v; }
};

// feature-store element types (TIMHIP_STORE_*; batch.hip, sampler.hip): T = the stored element, CHUNK = elements of a 16-byte
// chunk, widen = the exact fp32 value of a stored element (fp16: v_cvt_f32_f16, which honours fp16 subnormals in the default
// kernel mode; bf16: the word moved to the upper half)
template <int ST> struct StoreT;
template <> struct StoreT<TIMHIP_STORE_F32> {
  typedef float T;
  static constexpr int CHUNK = 4;
  static __device__ __forceinline__ float widen(float v) { return v; }
};
template <> struct StoreT<TIMHIP_STORE_F16> {
  typedef uint16_t T;
  static constexpr int CHUNK = 8;
  static __device__ __forceinline__ float widen(uint16_t h) { return (float)__builtin_bit_cast(f16_t, h); }
};
template <> struct StoreT<TIMHIP_STORE_BF16> {
  typedef uint16_t T;
  static constexpr int CHUNK = 8;
  static __device__ __forceinline__ float widen(uint16_t h) { return __uint_as_float((uint32_t)h << 16); }
};
static inline bool valid_store(int st) { return st >= TIMHIP_STORE_F32 && st <= TIMHIP_STORE_BF16; }
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
// the eight elements of one 16-byte chunk of a 16-bit store (element 2 i in the low half of word i) as two fp32 quads
template <int ST>
__device__ __forceinline__ void widen8(u32x4_t w, f32x4_t& lo, f32x4_t& hi) {
  typedef StoreT<ST> S;
  lo[0] = S::widen((uint16_t)w[0]); lo[1] = S::widen((uint16_t)(w[0] >> 16));
  lo[2] = S::widen((uint16_t)w[1]); lo[3] = S::widen((uint16_t)(w[1] >> 16));
  hi[0] = S::widen((uint16_t)w[2]); hi[1] = S::widen((uint16_t)(w[2] >> 16));
  hi[2] = S::widen((uint16_t)w[3]); hi[3] = S::widen((uint16_t)(w[3] >> 16));
}
// run the statement with the constant ST = the store type `st` (which must satisfy valid_store)
#define DISPATCH_STORE(st, ...)                                                              \
  do {                                                                                       \
    if ((st) == TIMHIP_STORE_F16) { constexpr int ST = TIMHIP_STORE_F16; __VA_ARGS__; }      \
    else if ((st) == TIMHIP_STORE_BF16) { constexpr int ST = TIMHIP_STORE_BF16; __VA_ARGS__; } \
    else { constexpr int ST = TIMHIP_STORE_F32; __VA_ARGS__; }                               \
  } while (0)

// v_mfma_f32_32x32x16_{bf16,f16}: D[32x32] += A[32x16] B[16x32], 8 operand values per lane, fp32 accumulate
template <typename HT> __device__ __forceinline__ f32x16_t mfma16(vec8<HT> a, vec8<HT> b, f32x16_t c);
template <> __device__ __forceinline__ f32x16_t mfma16<bf16_t>(vec8<bf16_t> a, vec8<bf16_t> b, f32x16_t c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
template <> __device__ __forceinline__ f32x16_t mfma16<f16_t>(vec8<f16_t> a, vec8<f16_t> b, f32x16_t c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}

// v_mfma_f32_16x16x32_{bf16,f16}: D[16x16] += A[16x32] B[32x16]; lane l holds A[l & 15][8 (l >> 4) .. +7], the same of B^T,
// and D[4 (l >> 4) + r][l & 15], r = 0..3
template <typename HT> __device__ __forceinline__ f32x4_t mfma16x16(vec8<HT> a, vec8<HT> b, f32x4_t c);
template <> __device__ __forceinline__ f32x4_t mfma16x16<bf16_t>(vec8<bf16_t> a, vec8<bf16_t> b, f32x4_t c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
template <> __device__ __forceinline__ f32x4_t mfma16x16<f16_t>(vec8<f16_t> a, vec8<f16_t> b, f32x4_t c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}

template <typename T>
__device__ __forceinline__ void store4(T* p, float a, float b, float c, float d);
template <>
__device__ __forceinline__ void store4<float>(float* p, float a, float b, float c, float d) {
  *reinterpret_cast<float4*>(p) = make_float4(a, b, c, d);
}
template <>
__device__ __forceinline__ void store4<bf16_t>(bf16_t* p, float a, float b, float c, float d) {
  bf16x4_t v;
  v[0] = (bf16_t)a; v[1] = (bf16_t)b; v[2] = (bf16_t)c; v[3] = (bf16_t)d;
  *reinterpret_cast<bf16x4_t*>(p) = v;
}
template <>
__device__ __forceinline__ void store4<f16_t>(f16_t* p, float a, float b, float c, float d) {
  vec4<f16_t> v;
  v[0] = (f16_t)a; v[1] = (f16_t)b; v[2] = (f16_t)c; v[3] = (f16_t)d;
  *reinterpret_cast<vec4<f16_t>*>(p) = v;
}
template <typename T>
__device__ __forceinline__ void load4(const T* p, float& a, float& b, float& c, float& d);
template <>
__device__ __forceinline__ void load4<float>(const float* p, float& a, float& b, float& c, float& d) {
  float4 v = *reinterpret_cast<const float4*>(p);
  a = v.x; b = v.y; c = v.z; d = v.w;
}
template <>
__device__ __forceinline__ void load4<bf16_t>(const bf16_t* p, float& a, float& b, float& c, float& d) {
  bf16x4_t v = *reinterpret_cast<const bf16x4_t*>(p);
  a = (float)v[0]; b = (float)v[1]; c = (float)v[2]; d = (float)v[3];
}

template <>
__device__ __forceinline__ void load4<f16_t>(const f16_t* p, float& a, float& b, float& c, float& d) {
  vec4<f16_t> v = *reinterpret_cast<const vec4<f16_t>*>(p);
  a = (float)v[0]; b = (float)v[1]; c = (float)v[2]; d = (float)v[3];
}

// ----------------------------------------------------------------------------
// Philox4x32-7 counter RNG (7 rounds: the fewest that pass BigCrush, Salmon et al. 2011): dropout masks are a pure function of
// (seed, site, element index) so the backward regenerates them.
// ----------------------------------------------------------------------------
struct Philox4 { uint32_t x, y, z, w; };

__host__ __device__ __forceinline__ uint32_t mulhi32(uint32_t a, uint32_t b) {
#ifdef __HIP_DEVICE_COMPILE__
  return __umulhi(a, b);
#else
  return (uint32_t)(((uint64_t)a * b) >> 32);
#endif
}

constexpr int PHILOX_ROUNDS = 7;
__host__ __device__ __forceinline__ Philox4 philox4x32_7(uint64_t seed, uint32_t site, uint64_t ctr) {
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  uint32_t c0 = (uint32_t)ctr, c1 = (uint32_t)(ctr >> 32), c2 = site, c3 = 0x7149u;
#pragma unroll
  for (int r = 0; r < PHILOX_ROUNDS; ++r) {
    // one 64-bit product per multiplier: v_mad_u64_u32 yields the high and the low word together (separate mul_hi / mul_lo
    // are two quarter-rate instructions; tools/px/philox_mad.hip: 590 -> 780 G Philox/s, same bits)
    const uint64_t p0 = (uint64_t)0xD2511F53u * (uint64_t)c0, p1 = (uint64_t)0xCD9E8D57u * (uint64_t)c2;
    const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0, hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
    uint32_t n0 = hi1 ^ c1 ^ k0, n1 = lo1, n2 = hi0 ^ c3 ^ k1, n3 = lo0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return Philox4{c0, c1, c2, c3};
}

// Dropout seed as the kernels see it: the launch-time seed plus, when the caller registered one (timhip_dropout_salt), a
// 64-bit salt read from device memory at run time.  A step captured in a HIP graph bakes its launch arguments in; the salt
// is what lets every replay draw fresh masks (the host bumps the device word between replays, or inside the graph).
extern const unsigned long long* tim_salt_ptr;  // host variable holding a device pointer (api.hip)
struct TimSeed {
  uint64_t base;
  const unsigned long long* salt;
  __host__ __device__ TimSeed() : base(0), salt(nullptr) {}
  __host__ TimSeed(uint64_t s) : base(s), salt(tim_salt_ptr) {}
  // (gemm_pp.hip: pp_epilogue_wt_res forms the same sum from a scalar load of *salt - change the two together)
  __device__ __forceinline__ operator uint64_t() const { return salt ? base + (uint64_t)*salt : base; }
};

// keep-threshold: element kept iff rnd >= thr  (P[drop] = thr / 2^32 = p)
__host__ __device__ __forceinline__ uint32_t drop_threshold(float p) {
  double t = (double)p * 4294967296.0;
  if (t < 0) t = 0;
  if (t > 4294967295.0) t = 4294967295.0;
  return (uint32_t)t;
}

// Dropout decisions are 16-bit draws: ONE Philox call serves the 8 consecutive elements 8*c .. 8*c+7 (element e of the group
// = bits 16*(e&1) .. +15 of word e>>1; kept iff that halfword >= thr >> 16).  Half the Philox work of 32-bit draws - it was
// ~70 % of the attention kernels' VALU instructions and 8 us of LayerNorm-1 - at a drop probability quantised to 1/65536
// (0.1 -> 0.09999).  Every kernel and timhip_dropout_mask derive their masks from these helpers, so forward, backward and the
// tests' oracle agree by construction.
//
// masks of the 4 consecutive elements whose linear index is 4*q .. 4*q+3 (one half of counter q >> 1)
__device__ __forceinline__ void drop_mask4(uint64_t seed, uint32_t site, uint64_t q, uint32_t thr,
                                           float scale, float& m0, float& m1, float& m2, float& m3) {
  const Philox4 r = philox4x32_7(seed, site, q >> 1);
  const uint32_t a = (q & 1) ? r.z : r.x, b = (q & 1) ? r.w : r.y, t = thr >> 16;
  m0 = (a & 0xffffu) >= t ? scale : 0.f;
  m1 = (a >> 16) >= t ? scale : 0.f;
  m2 = (b & 0xffffu) >= t ? scale : 0.f;
  m3 = (b >> 16) >= t ? scale : 0.f;
}
// the same four factors from two words of a counter somebody else drew (lane pairs of the attention kernels share calls)
__device__ __forceinline__ void drop_mask4_words(uint32_t a, uint32_t b, uint32_t thr, float scale, float& m0, float& m1,
                                                 float& m2, float& m3) {
  const uint32_t t = thr >> 16;
  m0 = (a & 0xffffu) >= t ? scale : 0.f;
  m1 = (a >> 16) >= t ? scale : 0.f;
  m2 = (b & 0xffffu) >= t ? scale : 0.f;
  m3 = (b >> 16) >= t ? scale : 0.f;
}
// factor of the single element with linear index idx
__device__ __forceinline__ float drop_mask1(uint64_t seed, uint32_t site, uint64_t idx, uint32_t thr, float scale) {
  const Philox4 r = philox4x32_7(seed, site, idx >> 3);
  const int e = (int)(idx & 7), wsel = e >> 1;
  const uint32_t w = wsel == 0 ? r.x : (wsel == 1 ? r.y : (wsel == 2 ? r.z : r.w));
  return ((w >> (16 * (e & 1))) & 0xffffu) >= (thr >> 16) ? scale : 0.f;
}
// keep-bits of the 8 consecutive elements 8*c .. 8*c+7 (bit e = element 8*c + e kept)
__device__ __forceinline__ uint32_t drop_bits8(uint64_t seed, uint32_t site, uint64_t c, uint32_t thr) {
  const Philox4 r = philox4x32_7(seed, site, c);
  const uint32_t t = thr >> 16;
  return ((r.x & 0xffffu) >= t ? 1u : 0u) | ((r.x >> 16) >= t ? 2u : 0u) | ((r.y & 0xffffu) >= t ? 4u : 0u) |
         ((r.y >> 16) >= t ? 8u : 0u) | ((r.z & 0xffffu) >= t ? 16u : 0u) | ((r.z >> 16) >= t ? 32u : 0u) |
         ((r.w & 0xffffu) >= t ? 64u : 0u) | ((r.w >> 16) >= t ? 128u : 0u);
}

// keep-bits of the 32 consecutive elements 4*q0 .. 4*q0+31 (q0 a multiple of 2; bit i = element 4*q0 + i kept): the packed
// form of drop_mask4, produced ahead of time by a memory-bound kernel with idle VALU (LayerNorm forward) for a GEMM epilogue
// that would otherwise spend 15-18 us per launch drawing the same numbers while the matrix pipes wait
__device__ __forceinline__ uint32_t drop_bits32(uint64_t seed, uint32_t site, uint64_t q0, uint32_t thr) {
  uint32_t bits = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) bits |= drop_bits8(seed, site, (q0 >> 1) + j, thr) << (8 * j);
  return bits;
}
// factors of 4 consecutive elements from their keep-bits (low 4 bits of `nib`)
__device__ __forceinline__ void drop_mask4_bits(uint32_t nib, float scale, float& m0, float& m1, float& m2, float& m3) {
  m0 = (nib & 1u) ? scale : 0.f;
  m1 = (nib & 2u) ? scale : 0.f;
  m2 = (nib & 4u) ? scale : 0.f;
  m3 = (nib & 8u) ? scale : 0.f;
}

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is a PER-DEVICE attribute: the "already done" flag of a launcher is kept per
// device (a process that drives a second GPU would otherwise skip the call there and fail its launches)
struct PerDeviceOnce {
  bool done[32] = {};
  bool first() {   // true the first time it is asked on the current device
    int dev = 0;
    (void)hipGetDevice(&dev);
    dev = dev < 0 ? 0 : (dev > 31 ? 31 : dev);
    if (done[dev]) return false;
    done[dev] = true;
    return true;
  }
};

// dropout site ids (stream id = site; per-layer sites add 16*layer)
enum {
  SITE_FEAT_V = 1, SITE_FEAT_A = 2, SITE_SEQ = 3,
  SITE_MIXUP = 8,   // mixup.hip: lam and the permutation (not a dropout site: no salt, its own device counter)
  SITE_SAMPLER = 9, SITE_DRLOC = 10,   // sampler.hip: the batch order with its augmentation indices, the DRLoc positions (as SITE_MIXUP)
  SITE_L_BASE = 16, SITE_L_ATTN = 0, SITE_L_DROP1 = 1, SITE_L_FFN = 2, SITE_L_DROP2 = 3, SITE_L_STRIDE = 8
};
static inline uint32_t layer_site(int layer, int which) {
  return SITE_L_BASE + (uint32_t)layer * SITE_L_STRIDE + (uint32_t)which;
}

// ----------------------------------------------------------------------------
// math
// ----------------------------------------------------------------------------
// erf by Abramowitz-Stegun 7.1.26 (|abs error| <= 1.5e-7): 1 rcp + 1 exp + 5 fma instead of the
// ~40-instruction libm erff; the epilogues that apply GELU run once per output element and their
// VALU time is otherwise comparable to the MFMA main loop of a K=1024 tile.
// Returns erf(x/sqrt2) given x, and e = exp(-x*x/2) for reuse by the derivative.
__device__ __forceinline__ float erf_half_f(float x, float& e) {
  const float z = fabsf(x) * 0.70710678118654752440f;
  const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, z, 1.0f));
  e = __expf(-0.5f * x * x);
  float p = fmaf(1.061405429f, t, -1.453152027f);
  p = fmaf(p, t, 1.421413741f);
  p = fmaf(p, t, -0.284496736f);
  p = fmaf(p, t, 0.254829592f);
  const float r = fmaf(-p * t, e, 1.0f);
  return copysignf(r, x);
}
__device__ __forceinline__ float gelu_f(float x) {
  float e;
  return 0.5f * x * (1.0f + erf_half_f(x, e));
}
__device__ __forceinline__ float gelu_grad_f(float x) {
  const float kInvSqrt2Pi = 0.3989422804014327f;
  float e;
  const float er = erf_half_f(x, e);
  return fmaf(x * kInvSqrt2Pi, e, 0.5f * (1.0f + er));
}

// gelu(x) and gelu'(x) from one erf / exp evaluation
__device__ __forceinline__ void gelu_both_f(float x, float& gl, float& dg) {
  const float kInvSqrt2Pi = 0.3989422804014327f;
  float e;
  const float ph = 0.5f * (1.0f + erf_half_f(x, e));   // Phi(x)
  gl = x * ph;
  dg = fmaf(x * kInvSqrt2Pi, e, ph);
}

// gelu_both_f on two elements at once: per component the SAME IEEE operations in the same order (every fused multiply-add is
// explicit in both forms, the exponential is the v_exp_f32 of h * log2(e) that __expf issues), written on 2-vectors so that all
// but |x|, the copysign, v_rcp_f32 and v_exp_f32 issue as v_pk_{fma,mul,add}_f32 - half the vector instructions per element
typedef float f32x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x2_t pk_fma(f32x2_t a, f32x2_t b, f32x2_t c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ f32x2_t pk_set(float v) { return f32x2_t{v, v}; }
__device__ __forceinline__ void gelu_both_f2(f32x2_t x, f32x2_t& gl, f32x2_t& dg) {
  const float kInvSqrt2Pi = 0.3989422804014327f, kLog2e = 1.44269504088896340736f;
  const f32x2_t z = f32x2_t{fabsf(x[0]), fabsf(x[1])} * 0.70710678118654752440f;
  const f32x2_t den = pk_fma(pk_set(0.3275911f), z, pk_set(1.0f));
  const f32x2_t t = {__builtin_amdgcn_rcpf(den[0]), __builtin_amdgcn_rcpf(den[1])};
  const f32x2_t h = ((x * -0.5f) * x) * kLog2e;
  const f32x2_t e = {__builtin_amdgcn_exp2f(h[0]), __builtin_amdgcn_exp2f(h[1])};
  f32x2_t p = pk_fma(pk_set(1.061405429f), t, pk_set(-1.453152027f));
  p = pk_fma(p, t, pk_set(1.421413741f));
  p = pk_fma(p, t, pk_set(-0.284496736f));
  p = pk_fma(p, t, pk_set(0.254829592f));
  const f32x2_t r = pk_fma(-p * t, e, pk_set(1.0f));
  const f32x2_t ph = (f32x2_t{copysignf(r[0], x[0]), copysignf(r[1], x[1])} + 1.0f) * 0.5f;   // Phi(x)
  gl = x * ph;
  dg = pk_fma(x * kInvSqrt2Pi, e, ph);
}

#include "tim_knobs.h"   // TimKnobs, tim_knobs(): the launchers' A/B knobs

// Non-finite watch of the fp16 gradient path.  `out_scale` (where a kernel takes one) points at word 1 of the block
// timhip_grad_scale writes: {S, 1/S, scratch, scratch, FLAG, 0, 0, 0}.  Every kernel that writes FINAL fp32 gradients
// through out_scale folds what it writes into `chk` (0 * v stays 0 unless v is inf / nan, then chk is nan for good) and ORs
// the flag word once per lane that saw one: what GradScaler's inf check (reference scripts/train.py:351,357-363) looks
// for, found where the values are produced instead of in a pass over 233 MB of gradients.
__device__ __forceinline__ void nf_note(float& chk, float v) { chk = fmaf(v, 0.f, chk); }
__device__ __forceinline__ void nf_commit(const float* out_scale, float chk) {
  if (out_scale != nullptr && chk != chk) atomicOr(reinterpret_cast<unsigned*>(const_cast<float*>(out_scale)) + 3, 1u);
}

// Wave-wide reductions without the LDS crossbar (__shfl_xor compiles to ds_bpermute_b32: six dependent LDS round trips per
// reduction): four DPP row rotations leave every 16-lane row's result in all of its lanes, four v_readlane + three VALU ops
// combine the rows.  Every lane of the wave must be active (as for the shuffles these replace).
template <int CTRL>
__device__ __forceinline__ float dpp_f(float x) {
  return __uint_as_float(__builtin_amdgcn_update_dpp(0u, __float_as_uint(x), CTRL, 0xF, 0xF, false));
}
__device__ __forceinline__ float lane_f(float x, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), l)); }
__device__ __forceinline__ float wave_sum(float v) {
  v += dpp_f<0x128>(v); v += dpp_f<0x124>(v); v += dpp_f<0x122>(v); v += dpp_f<0x121>(v);   // row_ror 8, 4, 2, 1
  return (lane_f(v, 0) + lane_f(v, 16)) + (lane_f(v, 32) + lane_f(v, 48));
}
__device__ __forceinline__ float wave_max(float v) {
  v = fmaxf(v, dpp_f<0x128>(v)); v = fmaxf(v, dpp_f<0x124>(v)); v = fmaxf(v, dpp_f<0x122>(v)); v = fmaxf(v, dpp_f<0x121>(v));
  return fmaxf(fmaxf(lane_f(v, 0), lane_f(v, 16)), fmaxf(lane_f(v, 32), lane_f(v, 48)));
}

// ----------------------------------------------------------------------------
// LDS-DMA (global_load_lds_dwordx4) issued from inline asm: hipcc does not count it, so it inserts no
// conservative `s_waitcnt vmcnt(0)` in front of later LDS reads; the kernel waits with
// glds_wait<N>() itself before the barrier that publishes the stage.  LDS destination =
// wave-uniform base + lane*16.
// ----------------------------------------------------------------------------
__device__ __forceinline__ uint32_t lds_addr_of(const void* p) {
  return (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const char*)p;
}
__device__ __forceinline__ void glds16(const void* gptr, uint32_t lds_base_uniform) {
  uint32_t keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\t"
      "s_mov_b32 m0, %2\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %1, off\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(gptr), "s"(lds_base_uniform)
      : "memory");
}
// make a wave-uniform pointer provably uniform (SGPR pair) for the "s" constraints below
__device__ __forceinline__ const void* uniform_ptr(const void* p) {
  const uint64_t v = (uint64_t)(uintptr_t)p;
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
  return (const void*)(uintptr_t)(((uint64_t)hi << 32) | lo);
}
// SGPR base (wave-uniform 64-bit address) + per-lane 32-bit byte offset: the per-step address update is
// one scalar add instead of a 64-bit vector add per load.
__device__ __forceinline__ void glds16_s(const void* sbase, uint32_t voff, uint32_t lds_base_uniform) {
  uint32_t keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\t"
      "s_mov_b32 m0, %3\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %1, %2\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(voff), "s"(sbase), "s"(lds_base_uniform)
      : "memory");
}
// four loads to LDS base, base+1 KiB, +2 KiB, +3 KiB with one M0 save/restore
__device__ __forceinline__ void glds16_x4(const void* sbase, uint32_t o0, uint32_t o1, uint32_t o2, uint32_t o3,
                                          uint32_t lds_base_uniform) {
  uint32_t keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\t"
      "s_mov_b32 m0, %6\n\t" "s_nop 0\n\t" "global_load_lds_dwordx4 %1, %5\n\t"
      "s_add_u32 m0, m0, 0x400\n\t" "s_nop 0\n\t" "global_load_lds_dwordx4 %2, %5\n\t"
      "s_add_u32 m0, m0, 0x400\n\t" "s_nop 0\n\t" "global_load_lds_dwordx4 %3, %5\n\t"
      "s_add_u32 m0, m0, 0x400\n\t" "s_nop 0\n\t" "global_load_lds_dwordx4 %4, %5\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(o0), "v"(o1), "v"(o2), "v"(o3), "s"(sbase), "s"(lds_base_uniform)
      : "memory", "scc");
}
template <int N>
__device__ __forceinline__ void glds16_xn(const void* sbase_, const uint32_t (&off)[N], uint32_t lds_base_uniform) {
  const void* sbase = uniform_ptr(sbase_);
  if constexpr (N % 4 == 0) {
#pragma unroll
    for (int i = 0; i < N; i += 4) glds16_x4(sbase, off[i], off[i + 1], off[i + 2], off[i + 3], lds_base_uniform + i * 1024);
  } else {
#pragma unroll
    for (int i = 0; i < N; ++i) glds16_s(sbase, off[i], lds_base_uniform + i * 1024);
  }
}
template <int N>
__device__ __forceinline__ void glds_wait() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// ----------------------------------------------------------------------------
// internal C++ launchers shared between translation units
// ----------------------------------------------------------------------------
// timing.hip: brackets a GEMM-family launch with HIP events while timhip_gemm_timing_start() is armed (bench.py roofline)
struct TimGemmScope {
  TimGemmScope(double flops, hipStream_t s, int family = 0);   // family 1: attention, 2: LayerNorm (work = algorithmic bytes)
  ~TimGemmScope();
  int slot;
  hipStream_t stream;
};

int tim_gemm_nt(int precision, int epi, const void* A, int lda, const void* B, int ldb, int M, int N,
                int K, const TimEpi& e, int splitk, hipStream_t s);
int tim_gemm_nt_group(int precision, int epi, const TimGemmItem* items, int n, hipStream_t s);
// gemm_pp.hip: out-projection / linear2 with the LayerNorm that follows fused into the epilogue (gemm_nt_ldln_kernel)
struct TimLnFuse {
  void* xt; int ldt; float* xf; int ldx; float* stats; const float* g; const float* b;            // LayerNorm outputs / parameters
  uint8_t* mask_out; int mask_cols; float mask_p; uint64_t mask_seed; uint32_t mask_site;           // keep-bits as tim_layernorm_fwd draws them
};
int tim_gemm_nt_pp_ln(int precision, const void* A, int lda, const void* B, int ldb, int M, int N, int K, const void* epi_dev,
                      const TimLnFuse& lf, const uint32_t** fail, hipStream_t s);
int tim_gemm_nt_fuse_ln(int precision, const void* A, int lda, const void* B, int ldb, int M, int N, int K, const TimEpi& te,
                        const TimLnFuse& lf, const uint32_t** fail, hipStream_t s);
// gemm_pp.hip: the one-block-per-CU kernels for the encoder-layer shapes, launched as gemm_plan.h's plan says (a plan of one of
// their families; epi_dev: the caller's EpiDev)
struct GemmPlan;
int tim_gemm_nt_pp(const GemmPlan& p, int precision, int epi, const void* A, int lda, const void* B, int ldb, int M, int N, int K,
                   const void* epi_dev, hipStream_t s);
int tim_transpose(int precision, const void* src, int rows, int cols, int lds, void* dst, int ld,
                  float* colsum, hipStream_t s);
int tim_slab_reduce(const float* slab, long long n, int nslab, float* dW, hipStream_t s);
size_t tim_wgrad_tn_ws(int Nout, int Kout, int M);
// out_scale: NULL, or a device scalar the written gradients are multiplied by (TIMHIP_PREC_F16 stores its gradient operands
// multiplied by S and passes 1/S here, see timhip_grad_scale)
int tim_wgrad_tn_h16(int precision, const void* dY, int ldy, int Nout, const void* X, int ldx, int Kout, int M, float* dW,
                     float* db, void* ws, size_t ws_bytes, hipStream_t s, int accumulate = 1, const float* out_scale = nullptr);
// which kernel a group gets, its geometry and its workspace: wgrad_plan.h (tim_wgrad_group_ws = the plan's ws_bytes)
size_t tim_wgrad_group_ws(const TimWgradItem* it, int n, int M);
int tim_wgrad_group_h16(int precision, const TimWgradItem* it, int n, int M, int accumulate, void* ws, size_t ws_bytes,
                        const float* out_scale, hipStream_t s);
// wgrad_pp.hip: launches a plan of one of the one-block-per-CU families (ping-pong, loader-wave, eight-phase: no split of the
// contraction, no workspace); the caller has checked the group's contract
struct WgradPlan;
int tim_wgrad_group_pp(const WgradPlan& p, int precision, const TimWgradItem* it, int n, int M, int accumulate, const float* out_scale,
                       hipStream_t s);
int tim_colsum(int precision, const void* src, int rows, int cols, int ld, float* out, hipStream_t s);
// mask_out != NULL: additionally writes the dropout keep-bits of a [rows, mask_cols] site (1 bit per element, row stride
// mask_cols / 8 bytes, element index r * mask_cols + c as in the GEMM epilogues) - see drop_bits32
int tim_layernorm_fwd(int precision, const float* y, int rows, int cols, int ldy, int act,
                      const float* w, const float* b, float* x_f32, int ldx, void* x_T, int ldt,
                      float* stats, hipStream_t s, uint8_t* mask_out = nullptr, int mask_cols = 0, float mask_p = 0.f,
                      uint64_t mask_seed = 0, uint32_t mask_site = 0,
                      const uint32_t* run_if = nullptr,   // run_if: control words of gemm_nt_ldln_kernel; the launch does nothing unless a tile of the launch in front of it timed out
                      int split_row = 0, const float* w2 = nullptr, const float* b2 = nullptr);   // rows >= split_row (> 0) use w2 / b2
int tim_layernorm_bwd(int precision, const float* dx, int lddx, const float* y, int ldy,
                      const float* stats, int rows, int cols, int act, const float* w, float* dy_f32,
                      int lddy, void* dy_T, int ldt, float p_drop, uint64_t seed, uint32_t site,
                      float* dgamma, float* dbeta, float* partial_ws, hipStream_t s, bool defer_colsum = false,
                      const float* t_scale = nullptr,   // t_scale: device scalar multiplied into the operand-dtype copy dy_T
                      const void* add_T = nullptr, int ldadd = 0, const float* add_scale = nullptr,   // dx += add_scale * add_T
                      int stream16 = 0,   // bit 0: dx is a T matrix (times 1 / add_scale); bit 1: dy_f32 is written as a T matrix times t_scale
                      int split_row = 0, const float* w2 = nullptr, float* dgamma2 = nullptr, float* dbeta2 = nullptr);   // blocks from split_row on: second parameter set
size_t tim_layernorm_bwd_ws(int rows, int cols);
int tim_layernorm_bwd_blocks(int rows);   // partial rows one backward launch over `rows` rows writes
// kbits (round 6): the layer's attention keep-bits as tim_attn_keep_bits wrote them (nullptr: the kernels draw their own)
// lse == nullptr: no log-sum-exp store (a forward without a backward).  s0 > 0: only the token rows s0 .. S - 1 of every window, written
// compactly - o[b * (S - s0) + (s - s0), :] - with the per-row arithmetic of the full form (timhip_attention_fwd_rows)
int tim_attention_fwd(const TimDesc& d, const void* qkv, void* o, float* lse, hipStream_t s, const unsigned long long* kbits = nullptr,
                      int s0 = 0);
int tim_attention_bwd(const TimDesc& d, const void* qkv, const void* o, const float* lse,
                      const void* d_o, void* dqkv, void* ws, size_t ws_bytes, hipStream_t s, const unsigned long long* kbits = nullptr);
// attention_mfma.hip: keep-bits of layers first .. first + n - 1 (n <= 8) into out[i]: [B * H * S][2] 64-bit words
int tim_attn_keep_bits(const TimDesc& d, int first_layer, int n, unsigned long long* const* out, hipStream_t s);
size_t tim_attention_bwd_ws(const TimDesc& d);
// attn_maps.hip: the head-averaged (per_head: per-head) softmax weights of the rows s0 .. S - 1, [.., S - s0, ld] fp32
int tim_attention_weights(const TimDesc& d, const void* qkv, int s0, int per_head, float* w, int ld, hipStream_t s);
// attention_query.hip: d.B groups of d.S query rows (qkv_q: q | own k | own v, compact) against the K | V rows of window widx[g] (or g)
// of a cache - kv: K of row 0 of window 0, V E elements behind it, row pitch ldkv, wrows rows per window, W windows
int tim_attention_query_fwd(const TimDesc& d, const void* qkv_q, const void* kv, int ldkv, int wrows, int W, const int* widx, void* o,
                            hipStream_t s);
// attn_maps.hip: the attention weights of those rows (tim_attention_weights' bodies, keys through the window index): w[g S + i, 0 .. F]
// fp32, row pitch ld; per_head: [G, H, S, ld]
int tim_attention_query_weights(const TimDesc& d, const void* qkv_q, const void* kv, int ldkv, int wrows, int W, const int* widx,
                                int per_head, float* w, int ld, hipStream_t s);

// operand storage: bf16 for TIMHIP_PREC_BF16, fp16 for TIMHIP_PREC_F16, fp32 for TIMHIP_PREC_FP32 and TIMHIP_PREC_BF16X3
static inline bool h16_storage(int precision) { return precision == TIMHIP_PREC_BF16 || precision == TIMHIP_PREC_F16; }
static inline bool f32_storage(int precision) { return !h16_storage(precision); }
static inline bool valid_precision(int precision) { return precision >= TIMHIP_PREC_BF16 && precision <= TIMHIP_PREC_F16; }
// run the statement with HT = the 16-bit operand type of `precision` (which must satisfy h16_storage)
// run the statement with T = the operand STORAGE type of `precision` (float / bf16_t / f16_t)
#define DISPATCH_T(prec, ...)                                           \
  do {                                                                  \
    if (f32_storage(prec)) { using T = float; __VA_ARGS__; }            \
    else if ((prec) == TIMHIP_PREC_F16) { using T = f16_t; __VA_ARGS__; } \
    else { using T = bf16_t; __VA_ARGS__; }                             \
  } while (0)
#define DISPATCH_H16(precision, ...)                                   \
  do {                                                                 \
    if ((precision) == TIMHIP_PREC_F16) { using HT = f16_t; __VA_ARGS__; } \
    else { using HT = bf16_t; __VA_ARGS__; }                            \
  } while (0)
static inline size_t opsize(int precision) { return f32_storage(precision) ? 4 : 2; }
