// Detection scoring: per-video detections and ground-truth segments become the true-positive flags, per-class
// interpolated average precision and mAP of the reference's scoring script (detection/eval_detection/
// evaluate_detection_json.py: compute_average_precision_detection, segment_iou, interpolated_prec_rec) without leaving the
// device.  Matching is independent per (class, video), AP per (class, threshold).
//
// det_match_kernel   one wavefront per (class, video) group of ground-truth segments, four groups per 256-thread block.  The
//                    wave walks the group's predictions in the class's score order, one after another; lane l holds segments
//                    l, l + 64, ... of the group.  Per prediction:
//                      inter = max(min(pe, ge) - max(ps, gs), 0);  union = (ge - gs) + (pe - ps) - inter;  tiou = inter / union
//                    in double - no product, so nothing can contract - and for each threshold t the segment with the largest
//                    tiou among those with tiou >= thr[t] that are not yet locked at t (equal tiou: the higher index inside the
//                    group) is locked at t: tp[t, pos] = 1, lock[t, segment] = the prediction's rank inside its class.  That is
//                    the reference's walk over the descending tiou order (skip the locked, stop below the threshold).  A NaN
//                    tiou (two zero-length segments) matches nothing.
//                    Lock state is one T-bit word per segment: in registers for groups of up to 256 segments, in the caller's
//                    workspace beyond.  A segment belongs to one lane of one wave for the whole launch, which is the only
//                    reader and writer of its word, its lock entries and (lane 0) the group's tp entries: plain loads and
//                    stores, no atomics, nothing depends on dispatch order.
// det_ap_kernel      one 256-thread block per (class, threshold) over the class's contiguous tp range: the true-positive total,
//                    then one walk from the right in chunks of 256 with two carries (true positives further right, largest
//                    precision further right): tpc_k = total - (those to the right), prec_k = tpc_k / (k + 1), its running
//                    maximum from the right, and the sum of (tpc_k / npos - (tpc_k - 1) / npos) * maxprec_k over tp_k = 1 -
//                    interpolated_prec_rec with its two sentinels (the trailing one adds (1 - rec_last) * 0).  Counts are
//                    integers and the maximum is exact, so the result differs from the reference's only in the order of a sum
//                    of at most npos positive terms that total at most 1.
//
// The unit is compiled with contraction off.
#include <math.h>

#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kWavesPerBlock = 4;
constexpr int kMaxBlocks = 2048;   // the grid is capped and the waves stride over the groups
constexpr int kRegSegs = 4;        // segments a lane keeps in registers: groups of up to 64 * kRegSegs
constexpr int kApBlock = 256;

__device__ __forceinline__ double seg_tiou(double ps, double pe, double gs, double ge) {
  const double inter = fmax(fmin(pe, ge) - fmax(ps, gs), 0.0);
  const double uni = ((ge - gs) + (pe - ps)) - inter;
  return inter / uni;
}

// the wave's best candidate in every lane: the largest value, among equal values the highest index; index -1 = none
__device__ __forceinline__ void wave_best(double& bv, int& bi) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(bv, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (oi >= 0 && (bi < 0 || ov > bv || (ov == bv && oi > bi))) {
      bv = ov;
      bi = oi;
    }
  }
}

struct MatchArgs {
  const double* pseg;     // [N, 2] in class / score order
  const int* gpred;       // [N] positions, grouped
  const double* gseg;     // [G, 2] grouped
  const double* thr;      // [T]
  uint8_t* tp;            // [T, N]
  int* lock;              // [T, G]
  unsigned* work;         // [G]
  long long N, G;
  int T;
};

template <bool REG>
__device__ __forceinline__ void match_group(const MatchArgs& a, int lane, int lo, int hi, int g0, int ng, int pos0) {
  double gs[kRegSegs], ge[kRegSegs];
  unsigned bits[kRegSegs];
  if (REG) {
#pragma unroll
    for (int k = 0; k < kRegSegs; ++k) {
      const int j = lane + 64 * k;
      gs[k] = j < ng ? a.gseg[2 * (size_t)(g0 + j)] : 0.0;
      ge[k] = j < ng ? a.gseg[2 * (size_t)(g0 + j) + 1] : 0.0;
      bits[k] = 0u;
    }
  } else {
    for (int j = lane; j < ng; j += 64) a.work[(size_t)g0 + j] = 0u;
  }
  for (int i = lo; i < hi; ++i) {
    const int pos = a.gpred[i];
    if (pos < 0 || (long long)pos >= a.N) continue;               // (uniform: every lane reads the same word)
    const double ps = a.pseg[2 * (size_t)pos], pe = a.pseg[2 * (size_t)pos + 1];
    double tv[kRegSegs];
    if (REG) {
#pragma unroll
      for (int k = 0; k < kRegSegs; ++k) tv[k] = seg_tiou(ps, pe, gs[k], ge[k]);
    }
    for (int t = 0; t < a.T; ++t) {
      const double th = a.thr[t];
      double bv = 0.0;
      int bi = -1;
      if (REG) {
#pragma unroll
        for (int k = 0; k < kRegSegs; ++k) {                       // ascending index, >=: the higher index keeps a tie
          const int j = lane + 64 * k;
          if (j < ng && tv[k] >= th && !((bits[k] >> t) & 1u) && (bi < 0 || tv[k] >= bv)) {
            bv = tv[k];
            bi = j;
          }
        }
      } else {
        for (int j = lane; j < ng; j += 64) {
          const double v = seg_tiou(ps, pe, a.gseg[2 * (size_t)(g0 + j)], a.gseg[2 * (size_t)(g0 + j) + 1]);
          if (v >= th && !((a.work[(size_t)g0 + j] >> t) & 1u) && (bi < 0 || v >= bv)) {
            bv = v;
            bi = j;
          }
        }
      }
      if (!__any(bi >= 0)) continue;                              // a false positive at t: tp stays 0
      wave_best(bv, bi);
      if ((bi & 63) == lane) {                                    // the lane that holds the segment
        if (REG) {
#pragma unroll
          for (int k = 0; k < kRegSegs; ++k)
            if (k == (bi >> 6)) bits[k] |= 1u << t;
        } else {
          a.work[(size_t)g0 + bi] |= 1u << t;
        }
        a.lock[(size_t)t * (size_t)a.G + (size_t)(g0 + bi)] = pos - pos0;
      }
      if (lane == 0) a.tp[(size_t)t * (size_t)a.N + (size_t)pos] = 1;
    }
  }
}

__global__ __launch_bounds__(64 * kWavesPerBlock) void det_match_kernel(MatchArgs a, const int* __restrict__ pred_lo,
                                                                         const int* __restrict__ pred_hi,
                                                                         const int* __restrict__ pos0,
                                                                         const int* __restrict__ gt_off, int n_groups) {
  const int lane = threadIdx.x & 63;
  const int wave = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  const int nwaves = gridDim.x * kWavesPerBlock;
  for (int g = wave; g < n_groups; g += nwaves) {
    long long lo = pred_lo[g], hi = pred_hi[g], g0 = gt_off[g], g1 = gt_off[g + 1];
    lo = lo < 0 ? 0 : lo;                                         // whatever the tables hold, no index leaves its array
    hi = hi > a.N ? a.N : hi;
    g0 = g0 < 0 ? 0 : g0;
    g1 = g1 > a.G ? a.G : g1;
    if (hi <= lo || g1 <= g0) continue;                           // a group without predictions: its segments stay unlocked
    const int ng = (int)(g1 - g0);
    if (ng <= 64 * kRegSegs) match_group<true>(a, lane, (int)lo, (int)hi, (int)g0, ng, pos0[g]);
    else match_group<false>(a, lane, (int)lo, (int)hi, (int)g0, ng, pos0[g]);
  }
}

// inclusive scans over the block's 256 threads in thread order; `total` = the last thread's value.  Two barriers each.
__device__ __forceinline__ int block_scan_sum(int x, int* sh, int& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int y = __shfl_up(x, o, 64);
    if (lane >= o) x += y;
  }
  if (lane == 63) sh[w] = x;
  __syncthreads();
  int before = 0, all = 0;
#pragma unroll
  for (int k = 0; k < kApBlock / 64; ++k) {
    before += k < w ? sh[k] : 0;
    all += sh[k];
  }
  __syncthreads();
  total = all;
  return x + before;
}

__device__ __forceinline__ double block_scan_max(double x, double* sh, double& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double y = __shfl_up(x, o, 64);
    if (lane >= o) x = fmax(x, y);
  }
  if (lane == 63) sh[w] = x;
  __syncthreads();
  double before = 0.0, all = 0.0;                                 // precisions are >= 0
#pragma unroll
  for (int k = 0; k < kApBlock / 64; ++k) {
    before = k < w ? fmax(before, sh[k]) : before;
    all = fmax(all, sh[k]);
  }
  __syncthreads();
  total = all;
  return fmax(x, before);
}

__global__ __launch_bounds__(kApBlock) void det_ap_kernel(const uint8_t* __restrict__ tp, const int* __restrict__ class_off,
                                                          const int* __restrict__ npos, int C, long long N,
                                                          double* __restrict__ ap) {
  __shared__ int sh_i[kApBlock / 64];
  __shared__ double sh_d[kApBlock / 64];
  const int c = blockIdx.x, t = blockIdx.y, tid = threadIdx.x;
  long long lo = class_off[c], hi = class_off[c + 1];
  lo = lo < 0 ? 0 : lo;
  hi = hi > N ? N : hi;
  const long long n = hi > lo ? hi - lo : 0;
  const double np = (double)npos[c];
  const uint8_t* row = tp + (size_t)t * (size_t)N;
  // ---- pass 1: the class's true positives at this threshold
  int cnt = 0;
  for (long long j = tid; j < n; j += kApBlock) cnt += row[lo + j] != 0;
  int total;
  block_scan_sum(cnt, sh_i, total);
  // ---- pass 2: from the right; thread j of a chunk takes position hi - 1 - (base + j), so "further right" is "earlier thread"
  int right_cnt = 0;             // true positives right of the chunk
  double right_max = 0.0;        // largest precision right of the chunk (the trailing sentinel is 0)
  double acc = 0.0;
  for (long long base = 0; base < n; base += kApBlock) {
    const long long j = base + tid;
    const bool valid = j < n;
    const long long k = hi - 1 - j;
    const int f = valid ? row[k] != 0 : 0;
    int chunk_cnt;
    const int incl = block_scan_sum(f, sh_i, chunk_cnt);
    const int tpc = total - (right_cnt + incl - f);               // inclusive count of true positives up to k
    const double prec = valid ? (double)tpc / (double)(k - lo + 1) : 0.0;
    double chunk_max;
    const double mx = fmax(block_scan_max(prec, sh_d, chunk_max), right_max);
    if (f) acc += ((double)tpc / np - (double)(tpc - 1) / np) * mx;
    right_cnt += chunk_cnt;
    right_max = fmax(right_max, chunk_max);
  }
  // ---- the block's sum, a fixed order: xor butterfly inside a wave, then the four waves in order
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if ((tid & 63) == 0) sh_d[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < kApBlock / 64; ++k) s += sh_d[k];
    ap[(size_t)t * (size_t)C + c] = npos[c] > 0 ? s : 0.0;
  }
}

}  // namespace

extern "C" {

int timhip_det_match(const double* pred_seg, int64_t n_pred, const int32_t* group_pred, const int32_t* group_pred_lo,
                     const int32_t* group_pred_hi, const int32_t* group_pos0, const double* gt_seg, int64_t n_gt,
                     const int32_t* group_gt_off, int n_groups, const double* thresholds, int T, uint8_t* tp, int32_t* lock,
                     uint32_t* work, void* stream) {
  if (T < 1 || T > TIMHIP_DET_MAX_THRESHOLDS || n_pred < 0 || n_gt < 0 || n_groups < 0) return TIMHIP_EINVAL;
  if (n_pred > 0x7fffffffLL || n_gt > 0x7fffffffLL) return TIMHIP_EUNSUPPORTED;
  if (n_groups == 0 || n_pred == 0 || n_gt == 0) return TIMHIP_OK;
  if (!pred_seg || !group_pred || !group_pred_lo || !group_pred_hi || !group_pos0 || !gt_seg || !group_gt_off || !thresholds ||
      !tp || !lock || !work)
    return TIMHIP_EINVAL;
  MatchArgs a = {pred_seg, group_pred, gt_seg, thresholds, tp, lock, work, (long long)n_pred, (long long)n_gt, T};
  int blocks = (n_groups + kWavesPerBlock - 1) / kWavesPerBlock;
  blocks = blocks > kMaxBlocks ? kMaxBlocks : blocks;
  hipLaunchKernelGGL(det_match_kernel, dim3(blocks), dim3(64 * kWavesPerBlock), 0, (hipStream_t)stream, a, group_pred_lo,
                     group_pred_hi, group_pos0, group_gt_off, n_groups);
  TIM_CHECK_LAUNCH();
  return TIMHIP_OK;
}

int timhip_det_ap(const uint8_t* tp, int64_t n_pred, const int32_t* class_off, const int32_t* npos, int n_classes, int T,
                  double* ap, void* stream) {
  if (T < 1 || T > TIMHIP_DET_MAX_THRESHOLDS || n_pred < 0 || n_classes < 0) return TIMHIP_EINVAL;
  if (n_pred > 0x7fffffffLL) return TIMHIP_EUNSUPPORTED;
  if (n_classes == 0 || n_pred == 0) return TIMHIP_OK;
  if (!tp || !class_off || !npos || !ap) return TIMHIP_EINVAL;
  hipLaunchKernelGGL(det_ap_kernel, dim3(n_classes, T), dim3(kApBlock), 0, (hipStream_t)stream, tp, class_off, npos,
                     n_classes, (long long)n_pred, ap);
  TIM_CHECK_LAUNCH();
  return TIMHIP_OK;
}

}  // extern "C"
