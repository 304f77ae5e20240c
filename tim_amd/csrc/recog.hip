// Recognition inference tail: the head logits of the evaluation batches become per-action scores and the
// top-1 / top-5 counts without leaving the device.  It restates what the reference does on the host in
// recognition/time_interval_machine/utils/meters.py (InferenceMeter.update / update_epoch, FeatureMeter.update /
// finalize_metrics: index_add_ of the valid query rows into per-action accumulators, division by the seen count, softmax) and
// utils/metrics.py (accuracy, multitask_accuracy).
//
// Accumulation order is the contract.  The reference's index_add_ runs on the CPU, serially in row order, batch after batch,
// so an action's accumulator is ((((0 + x_r0) + x_r1) + ...) in fp32 over its valid rows in stream order.  The kernels
// reproduce exactly that, whatever the dispatch order and however the stream is cut into batches:
//   rec_eid_kernel         one thread per row: the row's effective id (-1: not valid, not read again) -> work[0 .. R); a valid
//                          row whose id is outside [0, num_actions) is dropped and ORs the error word (an integer atomic)
//   rec_link_kernel        one wavefront per row: the next later row with the same id (-1: none) -> work[2R .. 3R), and that
//                          row's "has a predecessor" mark -> work[R .. 2R).  A row is the successor of at most one row, so
//                          every mark has one writer.
//   rec_accumulate_kernel  one wavefront per (row, head, 256-column chunk): only the FIRST row of an id works; it loads the
//                          accumulator chunk, walks its chain in ascending row order adding one logits row at a time, and
//                          stores the chunk back.  The (row, first chunk of the first head) wavefront also adds the chain
//                          length to `seen`, sets the touched byte and copies the labels of the chain's LAST row.
// No floating-point atomics; every accumulator element has one writer per call, and calls on one stream are ordered.
//
// rec_finalize_kernel    one wavefront per touched action of one head:
//   mean_c = sum_c / seen                         fp32, the correctly rounded division (what the reference's tensors carry)
//   rank   = #{c : mean_c > mean_label} + #{c < label : mean_c == mean_label}       on the MEAN logits: softmax is monotone
//                                                 and can only merge neighbours by rounding, so this is the reference's topk
//                                                 position wherever its own fp32 probabilities do not tie at the boundary
//   prob_c = (float)(exp((double)mean_c - (double)max) / S),  S = sum of the exps in double: each lane adds its columns in
//            ascending order, then a fixed xor butterfly over the 64 lanes.  Reproducible on a CPU to the last bit of the
//            double exp, like the sigmoid of detect.hip.
// rec_counts_kernel      one block: #(rank < 1), #(rank < 5) and the number of touched actions; with a second rank vector
//                        the rank is the larger of the two (verb + noun multitask accuracy).
// rec_combined_kernel    the AVE-only "combined" accuracy: the action and the audio probabilities of the labelled
//                        actions paired by position, averaged in fp32 and ranked; described at the kernel.
//
// The unit is compiled with contraction off (no product here feeds an add, and none may start to).  Loads are one dword per
// lane, 256 contiguous bytes per wave instruction, four chunks in flight, as in detect.hip: rows of 97 or 3,806 floats are
// not 16-byte aligned.  The accumulator pitch is the caller's; a multiple of 64 floats puts every wave store on one aligned
// 256-byte segment.
#include <math.h>

#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kWavesPerBlock = 4;
constexpr int kMaxBlocks = 2048;   // memory-bound grids: cap them and stride over the items
constexpr int kChunk = 256;        // columns one wavefront owns: 4 dwords per lane
constexpr int kNoRank = 0x7fffffff;

struct RecHeads {
  const float* logits[TIMHIP_REC_MAX_HEADS];
  float* sum[TIMHIP_REC_MAX_HEADS];
  long long ld[TIMHIP_REC_MAX_HEADS];
  int C[TIMHIP_REC_MAX_HEADS];
  int pitch[TIMHIP_REC_MAX_HEADS];
  int nch[TIMHIP_REC_MAX_HEADS];    // chunks of a row of head h
};

// (a select chain, not an indexed read: the struct is a kernel argument and stays in scalar registers this way)
template <typename T> __device__ __forceinline__ T pick(int h, const T (&a)[TIMHIP_REC_MAX_HEADS]) {
  return h == 0 ? a[0] : (h == 1 ? a[1] : a[2]);
}

__global__ __launch_bounds__(256) void rec_eid_kernel(const long long* __restrict__ ids, const uint8_t* __restrict__ valid,
                                                      const long long* __restrict__ labels, long long ldl, int valid_col, int R,
                                                      int num_actions, int* __restrict__ err, int* __restrict__ work) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= R) return;
  const bool v = valid ? valid[r] != 0 : labels[(size_t)r * (size_t)ldl + valid_col] != -1;
  int e = -1;
  if (v) {
    const long long id = ids[r];
    if (id >= 0 && id < (long long)num_actions) e = (int)id;
    else atomicOr(err, 1);
  }
  work[r] = e;
  work[R + r] = 0;
}

__global__ __launch_bounds__(64 * kWavesPerBlock) void rec_link_kernel(int R, int* __restrict__ work) {
  const int lane = threadIdx.x & 63;
  const int wave = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  const int nwaves = gridDim.x * kWavesPerBlock;
  const int* eid = work;
  for (int r = wave; r < R; r += nwaves) {
    const int e = eid[r];
    int next = -1;
    if (e >= 0) {
      for (int base = r + 1; base < R && next < 0; base += kChunk) {
        int v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int j = base + 64 * k + lane;
          v[k] = j < R ? eid[j] : -1;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const unsigned long long m = __ballot(v[k] == e);
          if (m != 0ull && next < 0) next = base + 64 * k + (int)__ffsll((long long)m) - 1;
        }
      }
    }
    if (lane == 0) {
      work[2 * (size_t)R + r] = next;
      if (next >= 0) work[(size_t)R + next] = 1;
    }
  }
}

__global__ __launch_bounds__(64 * kWavesPerBlock) void rec_accumulate_kernel(
    RecHeads hd, int chunks_per_row, const long long* __restrict__ labels, long long ldl, int n_labels, int R,
    const int* __restrict__ work, float* __restrict__ seen, int* __restrict__ labels_state, uint8_t* __restrict__ touched) {
  const int lane = threadIdx.x & 63;
  const int wave = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  const int nwaves = gridDim.x * kWavesPerBlock;
  const int* eid = work;
  const int* has_pred = work + R;
  const int* nxt = work + 2 * (size_t)R;
  const int items = R * chunks_per_row;
  for (int it = wave; it < items; it += nwaves) {
    const int r = it / chunks_per_row, t = it - r * chunks_per_row;
    const int e = eid[r];
    if (e < 0 || has_pred[r]) continue;                         // not valid, or a later link of another row's chain
    const int h = (t >= hd.nch[0]) + (t >= hd.nch[0] + hd.nch[1]);
    const int cb = (t - (h > 0 ? hd.nch[0] : 0) - (h > 1 ? hd.nch[1] : 0)) * kChunk;
    const float* lg = pick(h, hd.logits);
    const long long ld = pick(h, hd.ld);
    const int C = pick(h, hd.C);
    float* acc_row = pick(h, hd.sum) + (size_t)e * (size_t)pick(h, hd.pitch);
    float acc[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = cb + 64 * k + lane;
      acc[k] = c < C ? acc_row[c] : 0.0f;
    }
    int n = 0, last = r;
    for (int j = r; j >= 0; j = nxt[j]) {                       // ascending rows: the order of a serial index_add_
      const float* row = lg + (size_t)j * (size_t)ld;
      float x[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int c = cb + 64 * k + lane;
        x[k] = c < C ? row[c] : 0.0f;
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) acc[k] = __fadd_rn(acc[k], x[k]);
      last = j;
      ++n;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = cb + 64 * k + lane;
      if (c < C) acc_row[c] = acc[k];
    }
    if (t == 0) {
      if (lane == 0) {
        seen[e] = __fadd_rn(seen[e], (float)n);                 // whole numbers: exact, whatever the grouping
        touched[e] = 1;
      }
      if (labels && lane < n_labels)
        labels_state[(size_t)e * n_labels + lane] = (int)labels[(size_t)last * (size_t)ldl + lane];
    }
  }
}

__global__ __launch_bounds__(64 * kWavesPerBlock) void rec_finalize_kernel(
    const float* __restrict__ sum, int pitch, int C, const float* __restrict__ seen, const int* __restrict__ labels_state,
    int n_labels, int label_col, const uint8_t* __restrict__ touched, int num_actions, float* __restrict__ prob,
    int* __restrict__ rank) {
  const int lane = threadIdx.x & 63;
  const int wave = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  const int nwaves = gridDim.x * kWavesPerBlock;
  for (int a = wave; a < num_actions; a += nwaves) {
    if (!touched[a]) {
      if (lane == 0) rank[a] = kNoRank;
      continue;
    }
    const float s = seen[a];
    const float* row = sum + (size_t)a * (size_t)pitch;
    const int lab = labels_state ? labels_state[(size_t)a * n_labels + label_col] : -1;
    const bool has = lab >= 0 && lab < C;
    const float ml = has ? __fdiv_rn(row[lab], s) : 0.0f;
    // ---- pass 1: the row maximum and the label's rank, both on the mean logits
    float mx = -INFINITY;
    int above = 0, nan = 0;
    for (int cb = 0; cb < C; cb += kChunk) {
      float x[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int c = cb + 64 * k + lane;
        x[k] = c < C ? row[c] : 0.0f;
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int c = cb + 64 * k + lane;
        if (c < C) {
          const float m = __fdiv_rn(x[k], s);
          nan |= m != m;
          mx = fmaxf(mx, m);
          above += has && (m > ml || (m == ml && c < lab));
        }
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      mx = fmaxf(mx, __shfl_xor(mx, o, 64));
      above += __shfl_xor(above, o, 64);
      nan |= __shfl_xor(nan, o, 64);
    }
    if (lane == 0) rank[a] = has ? above : kNoRank;
    if (!prob) continue;
    // ---- pass 2: S in double, a fixed order
    const double dmx = nan ? (double)NAN : (double)mx;          // a NaN mean makes the whole row NaN, as torch's softmax does
    double acc = 0.0;
    for (int cb = 0; cb < C; cb += kChunk) {
      float x[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int c = cb + 64 * k + lane;
        x[k] = c < C ? row[c] : 0.0f;
      }
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (cb + 64 * k + lane < C) acc = __dadd_rn(acc, exp(__dsub_rn((double)__fdiv_rn(x[k], s), dmx)));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc = __dadd_rn(acc, __shfl_xor(acc, o, 64));
    // ---- pass 3: the probabilities, rounded once
    float* out = prob + (size_t)a * (size_t)pitch;
    for (int cb = 0; cb < C; cb += kChunk) {
      float x[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int c = cb + 64 * k + lane;
        x[k] = c < C ? row[c] : 0.0f;
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int c = cb + 64 * k + lane;
        if (c < C) out[c] = (float)__ddiv_rn(exp(__dsub_rn((double)__fdiv_rn(x[k], s), dmx)), acc);
      }
    }
  }
}

__global__ __launch_bounds__(1024) void rec_counts_kernel(const int* __restrict__ rank_a, const int* __restrict__ rank_b,
                                                          const uint8_t* __restrict__ touched, int num_actions,
                                                          int* __restrict__ out) {
  __shared__ int part[3][16];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  int v[3] = {0, 0, 0};
  for (int a = tid; a < num_actions; a += 1024) {
    if (!touched[a]) continue;
    int r = rank_a[a];
    if (rank_b) r = max(r, rank_b[a]);
    v[0] += r < 1;
    v[1] += r < 5;
    v[2] += 1;
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[i] += __shfl_xor(v[i], o, 64);
    if (lane == 0) part[i][w] = v[i];
  }
  __syncthreads();
  if (tid < 3) {
    int s = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) s += part[tid][k];
    out[tid] = s;
  }
}

// The AVE-only "combined" accuracy (meters.py:283-285): the reference adds the visual and the audio probabilities of the
// labelled actions POSITIONALLY, the k-th labelled visual action with the k-th labelled audio action in ascending id order.
// One wavefront per touched visual action a: k = #touched visual ids below a, b = the k-th touched audio id (two ballot
// scans over the touched bytes: num_actions / 64 steps each, a few thousand ids on AVE), then the rank of a's label over
// (p_action[a] + p_audio[b]) * 0.5f in fp32, with rec_finalize_kernel's tie rule.  No partner: kNoRank.
__global__ __launch_bounds__(64 * kWavesPerBlock) void rec_combined_kernel(
    const float* __restrict__ prob_v, int pitch_v, const float* __restrict__ prob_a, int pitch_a, int C,
    const int* __restrict__ labels_state, int n_labels, int label_col, const uint8_t* __restrict__ touched_v,
    const uint8_t* __restrict__ touched_a, int num_actions, int* __restrict__ rank) {
  const int lane = threadIdx.x & 63;
  const int wave = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  const int nwaves = gridDim.x * kWavesPerBlock;
  for (int a = wave; a < num_actions; a += nwaves) {
    if (!touched_v[a]) {
      if (lane == 0) rank[a] = kNoRank;
      continue;
    }
    int k = 0;
    for (int base = 0; base < a; base += 64) {
      const int j = base + lane;
      k += __popcll(__ballot(j < a && touched_v[j] != 0));
    }
    int b = -1, seen = 0;
    for (int base = 0; base < num_actions && b < 0; base += 64) {
      const int j = base + lane;
      unsigned long long m = __ballot(j < num_actions && touched_a[j] != 0);
      const int pc = __popcll(m);
      if (seen + pc > k) {
        for (int i = seen; i < k; ++i) m &= m - 1;              // drop the set bits in front of the k-th
        b = base + (int)__ffsll((long long)m) - 1;
      }
      seen += pc;
    }
    const int lab = labels_state[(size_t)a * n_labels + label_col];
    const bool has = b >= 0 && lab >= 0 && lab < C;
    if (!has) {
      if (lane == 0) rank[a] = kNoRank;
      continue;
    }
    const float* pv = prob_v + (size_t)a * (size_t)pitch_v;
    const float* pa = prob_a + (size_t)b * (size_t)pitch_a;
    const float sl = __fmul_rn(__fadd_rn(pv[lab], pa[lab]), 0.5f);
    int above = 0;
    for (int cb = 0; cb < C; cb += kChunk) {
      float x[4], y[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int c = cb + 64 * q + lane;
        x[q] = c < C ? pv[c] : 0.0f;
        y[q] = c < C ? pa[c] : 0.0f;
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int c = cb + 64 * q + lane;
        const float s = __fmul_rn(__fadd_rn(x[q], y[q]), 0.5f);
        above += c < C && (s > sl || (s == sl && c < lab));
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) above += __shfl_xor(above, o, 64);
    if (lane == 0) rank[a] = above;
  }
}

int rec_grid(long long waves) {
  const long long blocks = (waves + kWavesPerBlock - 1) / kWavesPerBlock;
  return blocks < 1 ? 1 : (blocks > kMaxBlocks ? kMaxBlocks : (int)blocks);
}

}  // namespace

extern "C" {

int timhip_rec_accumulate(const TimRecHead* heads, int n_heads, const int64_t* ids, const uint8_t* valid,
                          const int64_t* labels, int64_t ld_labels, int n_labels, int valid_col, int R, int num_actions,
                          float* seen, int32_t* labels_state, uint8_t* touched, int32_t* err, int32_t* work, void* stream) {
  if (!heads || n_heads < 1 || n_heads > TIMHIP_REC_MAX_HEADS || R < 0 || num_actions < 1) return TIMHIP_EINVAL;
  if (n_labels < 0 || n_labels > 64 || (labels && (n_labels < 1 || ld_labels < n_labels))) return TIMHIP_EINVAL;
  if (!valid && (!labels || valid_col < 0 || valid_col >= n_labels)) return TIMHIP_EINVAL;
  if (labels && !labels_state) return TIMHIP_EINVAL;
  if (!seen || !touched || !err) return TIMHIP_EINVAL;
  RecHeads hd = {};
  int chunks = 0;
  for (int h = 0; h < n_heads; ++h) {
    const TimRecHead& x = heads[h];
    if (x.C < 1 || x.pitch < x.C || x.ld < x.C || !x.sum || (R > 0 && !x.logits)) return TIMHIP_EINVAL;
    hd.logits[h] = x.logits; hd.sum[h] = x.sum; hd.ld[h] = x.ld; hd.C[h] = x.C; hd.pitch[h] = x.pitch;
    hd.nch[h] = (x.C + kChunk - 1) / kChunk;
    chunks += hd.nch[h];
  }
  if (R == 0) return TIMHIP_OK;
  if (!ids || !work) return TIMHIP_EINVAL;
  if ((long long)R * (long long)chunks > 0x7fffffffLL || R > 0x7fffffff / 3) return TIMHIP_EUNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(rec_eid_kernel, dim3((R + 255) / 256), dim3(256), 0, s, (const long long*)ids, valid,
                     (const long long*)labels, (long long)ld_labels, valid_col, R, num_actions, err, work);
  TIM_CHECK_LAUNCH();
  hipLaunchKernelGGL(rec_link_kernel, dim3(rec_grid(R)), dim3(64 * kWavesPerBlock), 0, s, R, work);
  TIM_CHECK_LAUNCH();
  hipLaunchKernelGGL(rec_accumulate_kernel, dim3(rec_grid((long long)R * chunks)), dim3(64 * kWavesPerBlock), 0, s, hd, chunks,
                     (const long long*)labels, (long long)ld_labels, n_labels, R, work, seen, labels_state, touched);
  TIM_CHECK_LAUNCH();
  return TIMHIP_OK;
}

int timhip_rec_finalize(const float* sum, int pitch, int C, const float* seen, const int32_t* labels_state, int n_labels,
                        int label_col, const uint8_t* touched, int num_actions, float* prob, int32_t* rank, void* stream) {
  if (!sum || !seen || !touched || !rank || C < 1 || pitch < C || num_actions < 1) return TIMHIP_EINVAL;
  if (labels_state && (n_labels < 1 || label_col < 0 || label_col >= n_labels)) return TIMHIP_EINVAL;
  hipLaunchKernelGGL(rec_finalize_kernel, dim3(rec_grid(num_actions)), dim3(64 * kWavesPerBlock), 0, (hipStream_t)stream, sum,
                     pitch, C, seen, labels_state, n_labels, label_col, touched, num_actions, prob, rank);
  TIM_CHECK_LAUNCH();
  return TIMHIP_OK;
}

int timhip_rec_combined(const float* prob_v, int pitch_v, const float* prob_a, int pitch_a, int C, const int32_t* labels_state,
                        int n_labels, int label_col, const uint8_t* touched_v, const uint8_t* touched_a, int num_actions,
                        int32_t* rank, void* stream) {
  if (!prob_v || !prob_a || !labels_state || !touched_v || !touched_a || !rank) return TIMHIP_EINVAL;
  if (C < 1 || pitch_v < C || pitch_a < C || num_actions < 1 || n_labels < 1 || label_col < 0 || label_col >= n_labels)
    return TIMHIP_EINVAL;
  hipLaunchKernelGGL(rec_combined_kernel, dim3(rec_grid(num_actions)), dim3(64 * kWavesPerBlock), 0, (hipStream_t)stream, prob_v,
                     pitch_v, prob_a, pitch_a, C, labels_state, n_labels, label_col, touched_v, touched_a, num_actions, rank);
  TIM_CHECK_LAUNCH();
  return TIMHIP_OK;
}

int timhip_rec_counts(const int32_t* rank_a, const int32_t* rank_b, const uint8_t* touched, int num_actions, int32_t* counts,
                      void* stream) {
  if (!rank_a || !touched || !counts || num_actions < 1) return TIMHIP_EINVAL;
  hipLaunchKernelGGL(rec_counts_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, rank_a, rank_b, touched, num_actions,
                     counts);
  TIM_CHECK_LAUNCH();
  return TIMHIP_OK;
}

}  // extern "C"
