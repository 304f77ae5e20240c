// The tail of a training iteration as device-side passes over a table of parameters (include/timhip.h: timhip_optim_*):
// global gradient norm -> clip coefficient / non-finite decision / step count -> AdamW on the fp32 masters, writing the
// operand-dtype copies of the updated weights in the same pass.  Nothing here reads a scalar from the host: the learning
// rate, the step count and the skip decision live in the optimizer's state block, so a captured step replays correctly.
// HBM-bound streaming kernels: 16-byte accesses on the aligned body, scalar edges, grid capped with a block -> (item, tile)
// walk over a prefix table in the kernel arguments (the form of cast_weights_kernel, rowops.hip).
#include <math.h>

#include "common.h"

namespace {

constexpr int OPT_MAX = 48;      // items per launch: the table travels in the kernel arguments (48 x 64 B + prefix < 4 KB)
constexpr int OPT_TILE = 4096;   // elements per tile: 64 x 64 of a weight with copies, 4096 consecutive ones otherwise
constexpr int OPT_GRID = 2048;   // block cap (256 CUs x 8); a block strides over the tiles beyond it
constexpr int OPT_FLAGS = 32;
constexpr int OPT_STATES = 8;

struct OptBatch {
  int n;
  int tile0[OPT_MAX + 1];  // first tile of item i
  TimOptItem it[OPT_MAX];
};

struct OptFinish {
  int n_states, n_flags;
  float* state[OPT_STATES];
  double beta1[OPT_STATES], beta2[OPT_STATES];
  const uint32_t* flags[OPT_FLAGS];
};

__host__ __device__ inline int opt_mis(const void* p) { return (int)(((uintptr_t)p & 15) >> 2); }

// ---------------------------------------------------------------------------
// norm pass: partials[block] = sum of g^2 over the block's tiles (fp32 inside a tile, fp64 across tiles and lanes;
// every order is fixed by the table and the grid, so a replay reproduces the eager sum bit for bit)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void optim_norm_kernel(OptBatch ob, double* __restrict__ partials) {
  __shared__ double red[4];
  const int total = ob.tile0[ob.n];
  double acc = 0.0;
  int w = 0;
  for (int t = blockIdx.x; t < total; t += gridDim.x) {
    while (t >= ob.tile0[w + 1]) ++w;
    const float* __restrict__ g = ob.it[w].g;
    const int numel = ob.it[w].rows * ob.it[w].cols;
    // tiles are cut in the index space shifted by the start's offset from a 16-byte boundary: quad j is aligned iff j % 4 == 0
    const int s = opt_mis(g);
    const int j0 = (t - ob.tile0[w]) * OPT_TILE;
    float a = 0.f;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = j0 + 4 * ((int)threadIdx.x + 256 * u) - s;
      if (i >= 0 && i + 3 < numel) {
        const float4 x = *reinterpret_cast<const float4*>(g + i);
        a += x.x * x.x + x.y * x.y + x.z * x.z + x.w * x.w;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (i + e >= 0 && i + e < numel) a += g[i + e] * g[i + e];
      }
    }
    acc += (double)a;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__device__ inline double opt_ipow(double b, uint32_t t) {   // b^t by squaring: the bias corrections want fp64, once per step
  double r = 1.0;
  while (t) {
    if (t & 1u) r *= b;
    b *= b;
    t >>= 1;
  }
  return r;
}

// one block: the fixed-order sum of the partials, the external non-finite words, then every scalar of the step
__global__ __launch_bounds__(256) void optim_finish_kernel(const double* __restrict__ partials, int n, float max_norm,
                                                           OptFinish f) {
  __shared__ double red[256];
  __shared__ uint32_t bad;
  const int tid = threadIdx.x;
  double a = 0.0;
  for (int i = tid; i < n; i += 256) a += partials[i];
  red[tid] = a;
  if (tid == 0) bad = 0u;
  __syncthreads();
  if (tid < f.n_flags && *f.flags[tid] != 0u) atomicOr(&bad, 1u);
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  if (tid != 0) return;
  const float norm = (float)sqrt(red[0]);
  const bool found_inf = bad != 0u || !isfinite(norm);
  const float coef = max_norm > 0.f ? fminf(1.f, max_norm / (norm + 1e-6f)) : 1.f;
  for (int k = 0; k < f.n_states; ++k) {
    float* st = f.state[k];
    uint32_t* wi = reinterpret_cast<uint32_t*>(st);
    st[TIMHIP_OPT_NORM] = norm;
    st[TIMHIP_OPT_COEF] = coef;
    wi[TIMHIP_OPT_FOUND_INF] = found_inf ? 1u : 0u;
    if (found_inf) {
      wi[TIMHIP_OPT_SKIPPED] += 1u;
    } else {
      const uint32_t t = wi[TIMHIP_OPT_STEP] + 1u;
      wi[TIMHIP_OPT_STEP] = t;
      st[TIMHIP_OPT_BC1] = (float)(1.0 - opt_ipow(f.beta1[k], t));
      st[TIMHIP_OPT_BC2_SQRT] = (float)sqrt(1.0 - opt_ipow(f.beta2[k], t));
    }
  }
}

// ---------------------------------------------------------------------------
// update pass
// ---------------------------------------------------------------------------
struct OptCoef { float coef, decay, step_size, b1, omb1, b2, omb2, bc2s, eps; };

__device__ __forceinline__ void adamw1(float& p, float g, float& m, float& v, const OptCoef& k) {
  g *= k.coef;
  p *= k.decay;
  m = k.b1 * m + k.omb1 * g;
  v = k.b2 * v + k.omb2 * g * g;
  p -= k.step_size * (m / (sqrtf(v) / k.bc2s + k.eps));
}

template <typename T>
__device__ __forceinline__ void store8(T* dst, const float* v) {
  if constexpr (sizeof(T) == 2) {
    vec8<T> pk;
#pragma unroll
    for (int u = 0; u < 8; ++u) pk[u] = OpT<T>::from_f(v[u]);
    *reinterpret_cast<vec8<T>*>(dst) = pk;
  } else {
    store4<T>(dst, v[0], v[1], v[2], v[3]);
    store4<T>(dst + 4, v[4], v[5], v[6], v[7]);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void optim_update_kernel(OptBatch ob, const float* __restrict__ state, float b1, float omb1,
                                                           float b2, float omb2, float eps, float wd) {
  __shared__ float tile[64][65];
  if (reinterpret_cast<const uint32_t*>(state)[TIMHIP_OPT_FOUND_INF] != 0u) return;   // skipped step: nothing is touched
  OptCoef k;
  const float lr = state[TIMHIP_OPT_LR];
  k.coef = state[TIMHIP_OPT_COEF];
  k.decay = 1.f - lr * wd;
  k.step_size = lr / state[TIMHIP_OPT_BC1];
  k.b1 = b1; k.omb1 = omb1; k.b2 = b2; k.omb2 = omb2;
  k.bc2s = state[TIMHIP_OPT_BC2_SQRT];
  k.eps = eps;
  const int total = ob.tile0[ob.n];
  int w = 0;
  for (int t = blockIdx.x; t < total; t += gridDim.x) {
    while (t >= ob.tile0[w + 1]) ++w;
    const TimOptItem it = ob.it[w];
    float* __restrict__ p = it.p;
    const float* __restrict__ g = it.g;
    float* __restrict__ m = it.m;
    float* __restrict__ v = it.v;
    const int lt = t - ob.tile0[w];
    if (it.plain == nullptr) {
      // flat tile; 16-byte accesses when the four arrays sit at the same offset from a 16-byte boundary
      const int numel = it.rows * it.cols;
      const int s = opt_mis(p);
      const bool vec = s == opt_mis(g) && s == opt_mis(m) && s == opt_mis(v);
      const int j0 = lt * OPT_TILE;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = j0 + 4 * ((int)threadIdx.x + 256 * u) - (vec ? s : 0);
        if (vec && i >= 0 && i + 3 < numel) {
          float4 pp = *reinterpret_cast<const float4*>(p + i);
          const float4 gg = *reinterpret_cast<const float4*>(g + i);
          float4 mm = *reinterpret_cast<const float4*>(m + i);
          float4 vv = *reinterpret_cast<const float4*>(v + i);
          adamw1(pp.x, gg.x, mm.x, vv.x, k);
          adamw1(pp.y, gg.y, mm.y, vv.y, k);
          adamw1(pp.z, gg.z, mm.z, vv.z, k);
          adamw1(pp.w, gg.w, mm.w, vv.w, k);
          *reinterpret_cast<float4*>(p + i) = pp;
          *reinterpret_cast<float4*>(m + i) = mm;
          *reinterpret_cast<float4*>(v + i) = vv;
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (i + e >= 0 && i + e < numel) {
              float pp = p[i + e], mm = m[i + e], vv = v[i + e];
              adamw1(pp, g[i + e], mm, vv, k);
              p[i + e] = pp; m[i + e] = mm; v[i + e] = vv;
            }
        }
      }
      continue;
    }
    // a weight with operand copies: a 64 x 64 tile.  A lane owns 8 consecutive columns of a row on the way in (the updated
    // values leave as fp32 masters and as one 16-byte store of the plain copy) and 8 consecutive rows of a column on the way
    // out of the LDS tile (the transposed copy): full 128-byte lines in both orientations
    const int rows = it.rows, cols = it.cols, ldp = it.ldp, ldt = it.ldt;
    T* __restrict__ plain = (T*)it.plain;
    T* __restrict__ tr = (T*)it.tr;
    const int tiles_x = (cols + 63) >> 6;
    const int ty_ = lt / tiles_x;
    const int c0 = (lt - ty_ * tiles_x) * 64, r0 = ty_ * 64;
    const int tx = threadIdx.x & 7, ty = threadIdx.x >> 3;
    const bool vec = (cols & 3) == 0 && (opt_mis(p) | opt_mis(g) | opt_mis(m) | opt_mis(v)) == 0;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int r = r0 + ty + 32 * i, c = c0 + tx * 8;
      float pv[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) pv[u] = 0.f;
      if (r < rows && c < cols) {
        const size_t o = (size_t)r * cols + c;
        if (vec && c + 7 < cols) {
          float gv[8], mv[8], vv[8];
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const float4 a = *reinterpret_cast<const float4*>(p + o + 4 * h);
            const float4 b = *reinterpret_cast<const float4*>(g + o + 4 * h);
            const float4 cm = *reinterpret_cast<const float4*>(m + o + 4 * h);
            const float4 d = *reinterpret_cast<const float4*>(v + o + 4 * h);
            pv[4 * h] = a.x; pv[4 * h + 1] = a.y; pv[4 * h + 2] = a.z; pv[4 * h + 3] = a.w;
            gv[4 * h] = b.x; gv[4 * h + 1] = b.y; gv[4 * h + 2] = b.z; gv[4 * h + 3] = b.w;
            mv[4 * h] = cm.x; mv[4 * h + 1] = cm.y; mv[4 * h + 2] = cm.z; mv[4 * h + 3] = cm.w;
            vv[4 * h] = d.x; vv[4 * h + 1] = d.y; vv[4 * h + 2] = d.z; vv[4 * h + 3] = d.w;
          }
#pragma unroll
          for (int u = 0; u < 8; ++u) adamw1(pv[u], gv[u], mv[u], vv[u], k);
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            *reinterpret_cast<float4*>(p + o + 4 * h) = make_float4(pv[4 * h], pv[4 * h + 1], pv[4 * h + 2], pv[4 * h + 3]);
            *reinterpret_cast<float4*>(m + o + 4 * h) = make_float4(mv[4 * h], mv[4 * h + 1], mv[4 * h + 2], mv[4 * h + 3]);
            *reinterpret_cast<float4*>(v + o + 4 * h) = make_float4(vv[4 * h], vv[4 * h + 1], vv[4 * h + 2], vv[4 * h + 3]);
          }
        } else {
#pragma unroll
          for (int u = 0; u < 8; ++u)
            if (c + u < cols) {
              float mm = m[o + u], vv = v[o + u];
              pv[u] = p[o + u];
              adamw1(pv[u], g[o + u], mm, vv, k);
              p[o + u] = pv[u]; m[o + u] = mm; v[o + u] = vv;
            }
        }
        // (ldp % 64 == 0, so the octet is inside the row; its padding columns, if any, stay as they are)
        if (c + 7 < cols) {
          store8<T>(plain + (size_t)r * ldp + c, pv);
        } else {
#pragma unroll
          for (int u = 0; u < 8; ++u)
            if (c + u < cols) plain[(size_t)r * ldp + c + u] = OpT<T>::from_f(pv[u]);
        }
      }
      float* tl = &tile[ty + 32 * i][tx * 8];
#pragma unroll
      for (int u = 0; u < 8; ++u) tl[u] = pv[u];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int lc = ty + 32 * i, lr = tx * 8;
      const int c = c0 + lc, r = r0 + lr;
      if (c < cols && r < rows) {
        if (r + 7 < rows) {
          float tv[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) tv[u] = tile[lr + u][lc];
          store8<T>(tr + (size_t)c * ldt + r, tv);
        } else {
#pragma unroll
          for (int u = 0; u < 8; ++u)
            if (r + u < rows) tr[(size_t)c * ldt + r + u] = OpT<T>::from_f(tile[lr + u][lc]);
        }
      }
    }
    __syncthreads();   // the next tile of this block rewrites the LDS tile
  }
}

int opt_check_item(const TimOptItem& it) {
  if (!it.p || !it.g || !it.m || !it.v || it.rows <= 0 || it.cols <= 0) return TIMHIP_EINVAL;
  if ((long long)it.rows * it.cols >= (1ll << 31) - 2 * OPT_TILE) return TIMHIP_EUNSUPPORTED;
  if ((((uintptr_t)it.p | (uintptr_t)it.g | (uintptr_t)it.m | (uintptr_t)it.v) & 3) != 0) return TIMHIP_EALIGN;
  if ((it.plain == nullptr) != (it.tr == nullptr)) return TIMHIP_EINVAL;
  if (it.plain) {
    if (it.ldp % 64 || it.ldt % 64 || it.ldp < it.cols || it.ldt < it.rows) return TIMHIP_EINVAL;
    if ((((uintptr_t)it.plain | (uintptr_t)it.tr) & 15) != 0) return TIMHIP_EALIGN;
  }
  return TIMHIP_OK;
}

int opt_norm_tiles(const TimOptItem& it) { return (opt_mis(it.g) + it.rows * it.cols + OPT_TILE - 1) / OPT_TILE; }

int opt_update_tiles(const TimOptItem& it) {
  if (it.plain) return ((it.rows + 63) / 64) * ((it.cols + 63) / 64);
  return (3 + it.rows * it.cols + OPT_TILE - 1) / OPT_TILE;   // (room for any start offset: an empty last tile costs nothing)
}

// fills the chunk [i0, i0 + ob.n) of the table; returns the chunk's block count or a TIMHIP_E* code
template <typename F>
int opt_fill(OptBatch& ob, const TimOptItem* items, int i0, int n, F tiles_of) {
  ob.n = n - i0 < OPT_MAX ? n - i0 : OPT_MAX;
  int tiles = 0;
  for (int i = 0; i < ob.n; ++i) {
    const int rc = opt_check_item(items[i0 + i]);
    if (rc != TIMHIP_OK) return rc;
    ob.it[i] = items[i0 + i];
    ob.tile0[i] = tiles;
    tiles += tiles_of(items[i0 + i]);
  }
  for (int i = ob.n; i <= OPT_MAX; ++i) ob.tile0[i] = tiles;
  return tiles < OPT_GRID ? tiles : OPT_GRID;
}

}  // namespace

extern "C" {

int timhip_optim_norm_partials(const TimOptItem* items, int n) {
  if ((!items && n > 0) || n < 0) return TIMHIP_EINVAL;
  OptBatch ob;
  int count = 0;
  for (int i0 = 0; i0 < n; i0 += OPT_MAX) {
    const int blocks = opt_fill(ob, items, i0, n, opt_norm_tiles);
    if (blocks < 0) return blocks;
    count += blocks;
  }
  return count;
}

int timhip_optim_norm(const TimOptItem* items, int n, double* partials, void* stream) {
  if ((!items && n > 0) || n < 0 || (!partials && n > 0)) return TIMHIP_EINVAL;
  if ((uintptr_t)partials & 7) return TIMHIP_EALIGN;
  OptBatch ob;
  for (int i0 = 0; i0 < n; i0 += OPT_MAX) {
    const int blocks = opt_fill(ob, items, i0, n, opt_norm_tiles);
    if (blocks < 0) return blocks;
    hipLaunchKernelGGL(optim_norm_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, ob, partials);
    TIM_CHECK_LAUNCH();
    partials += blocks;
  }
  return TIMHIP_OK;
}

int timhip_optim_finish(const double* partials, int n_partials, const uint32_t* const* flags, int n_flags, float max_norm,
                        float* const* states, const double* beta1, const double* beta2, int n_states, void* stream) {
  if (n_partials < 0 || (n_partials > 0 && !partials) || n_flags < 0 || n_flags > OPT_FLAGS || (n_flags > 0 && !flags) ||
      n_states <= 0 || n_states > OPT_STATES || !states || !beta1 || !beta2)
    return TIMHIP_EINVAL;
  OptFinish f;
  f.n_states = n_states;
  f.n_flags = n_flags;
  for (int i = 0; i < OPT_STATES; ++i) {
    f.state[i] = i < n_states ? states[i] : nullptr;
    f.beta1[i] = i < n_states ? beta1[i] : 0.0;
    f.beta2[i] = i < n_states ? beta2[i] : 0.0;
    if (i < n_states && (!states[i] || ((uintptr_t)states[i] & 3))) return TIMHIP_EINVAL;
  }
  for (int i = 0; i < OPT_FLAGS; ++i) {
    f.flags[i] = i < n_flags ? flags[i] : nullptr;
    if (i < n_flags && (!flags[i] || ((uintptr_t)flags[i] & 3))) return TIMHIP_EINVAL;
  }
  hipLaunchKernelGGL(optim_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partials, n_partials, max_norm, f);
  TIM_CHECK_LAUNCH();
  return TIMHIP_OK;
}

int timhip_optim_update(int precision, const TimOptItem* items, int n, const float* state, double beta1, double beta2,
                        double eps, double weight_decay, void* stream) {
  if ((!items && n > 0) || n < 0 || !state || !valid_precision(precision)) return TIMHIP_EINVAL;
  OptBatch ob;
  for (int i0 = 0; i0 < n; i0 += OPT_MAX) {
    const int blocks = opt_fill(ob, items, i0, n, opt_update_tiles);
    if (blocks < 0) return blocks;
    if (blocks == 0) continue;
    DISPATCH_T(precision, hipLaunchKernelGGL(optim_update_kernel<T>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, ob, state,
                                             (float)beta1, (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps,
                                             (float)weight_decay));
    TIM_CHECK_LAUNCH();
  }
  return TIMHIP_OK;
}

}  // extern "C"
