// Detection inference tail: the class logits and regressed segments of one batch become the candidate list
// the per-video soft-NMS consumes, without the dense score matrix ever leaving the device.  It restates, per batch, what
// the reference does on the host in detection/time_interval_machine/utils/meters.py (FeatureMeter.update: sigmoid, clamp,
// rescale to seconds) and detection/eval_detection/format_predictions.py (main: round, drop empty proposals, threshold,
// one entry per surviving (proposal, class) pair).
//
// Order is part of the result (the soft-NMS keeps the FIRST maximum of its input order), so the list is produced in the
// reference's order - proposal by proposal, ascending class inside a proposal - by count + scan + emit:
//   det_count_kernel   one wavefront per proposal row: decode + round the segment (fp32 / fp64 split below), count the
//                      classes over the threshold -> row_offsets[r + 1]
//   det_scan_kernel    (candidates.h) one block: in-place inclusive scan -> row_offsets[r] = first output slot of row r, [R] = total
//   det_emit_kernel    the same walk; candidate k of row r lands at row_offsets[r] + k (__ballot + popcount of the lower
//                      lanes inside a 64-class chunk, a running base across chunks)
// No atomics and no look-back between workgroups: nothing depends on dispatch order.
//
// Arithmetic, operation by operation as the reference's tensors carry it:
//   p  = clamp(reg, 0, max_time)                 fp32
//   p  = p * window_size                         fp32 (one rounding)
//   p  = (double)p + window_start[w]             fp64 (the collated window_start is float64 and promotes the sum)
//   p  = rint(p * 1000.0) / 1000.0               fp64, numpy.round(p, 3): round-half-even on the scaled value
//   ok = p[1] - p[0] > 0.0                       fp64
//   score = (float)(1.0 / (1.0 + exp(-(double)x)))   the float64 sigmoid rounded once: reproducible on a CPU, which the
//                                                device's 1-ulp expf is not (nms.hip makes the same choice for its weights)
// The unit is compiled with contraction off so that no product above is fused into the add that follows it.
//
// Pre-filter.  sigmoid is monotone and so is the rounding to fp32, hence score(x) > t  <=>  x > x*(t) for one boundary
// x*(t) near logit(t) = log(t / (1 - t)).  The host computes two fp32 bounds (det_bounds below):
//   lo <= x*:  a real x < logit(t) has sigmoid(x) < t, the fp64 evaluation is within a few 1e-16 relative of it and t is an
//              fp32 number, so the rounded score is <= t.  lo = logit(t) - margin, rounded down.
//   hi >= x*:  t2 = the second fp32 number above t; a real x > logit(t2) has sigmoid(x) > t2, which rounds to at least the
//              first fp32 number above t.  hi = logit(t2) + margin, rounded up (+inf when t2 >= 1: no shortcut).
//   margin = 1e-5 * (1 + |logit|): four orders of magnitude over what it has to cover (the host's double log, ~1e-16
//   relative; the rounding of the bound to fp32, 6e-8 relative; the device's double exp, < 1 ulp of fp64), and still so
//   narrow that the band [lo, hi] holds a vanishing share of the logits.
// x < lo is rejected and, in the count, x > hi is accepted by one fp32 compare; the fp64 path runs for the band (count) and
// for the classes that can pass (emit: the few per cent whose score is written anyway).
//
// Loads are one dword per lane, 256 contiguous bytes per wave instruction, four chunks in flight: rows of 97 or 3,806
// floats are not 16-byte aligned, and the candidate order inside a chunk is the lane order this way.
#include <math.h>

#include "common.h"

#pragma clang fp contract(off)   // ahead of candidates.h: its arithmetic is compiled under it as well
#include "candidates.h"

namespace {

__global__ __launch_bounds__(64 * kWavesPerBlock) void det_count_kernel(
    const float* __restrict__ logits, long long ld, const float* __restrict__ reg, const double* __restrict__ window_start,
    float window_size, const float* __restrict__ max_time, int R, int C, int Nq, float thr, float lo, float hi,
    float* __restrict__ seg32, uint8_t* __restrict__ seg_ok, int* __restrict__ row_offsets) {
  const int lane = threadIdx.x & 63;
  const int wave = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  const int nwaves = gridDim.x * kWavesPerBlock;
  const float tmax = max_time[0];
  for (int r = wave; r < R; r += nwaves) {
    // ---- the proposal (every lane computes the same two numbers; lane 0 stores them)
    const double ws = window_start[r / Nq];
    const double p0 = cand_round3(cand_decode(reg[2 * (size_t)r], tmax, window_size, ws));
    const double p1 = cand_round3(cand_decode(reg[2 * (size_t)r + 1], tmax, window_size, ws));
    const bool ok = __dsub_rn(p1, p0) > 0.0;
    int n = 0;
    if (ok) {
      const float* row = logits + (size_t)r * (size_t)ld;
      for (int cb = 0; cb < C; cb += 256) {
        float x[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int c = cb + 64 * k + lane;
          x[k] = c < C ? row[c] : -INFINITY;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          bool pass = x[k] > hi;
          if (!pass && !(x[k] < lo) && cb + 64 * k + lane < C) pass = cand_sigmoid(x[k]) > thr;
          n += __popcll(__ballot(pass));
        }
      }
    }
    if (lane == 0) {
      seg32[2 * (size_t)r] = (float)p0;
      seg32[2 * (size_t)r + 1] = (float)p1;
      seg_ok[r] = ok ? 1 : 0;
      row_offsets[r + 1] = n;
    }
  }
}

__global__ __launch_bounds__(64 * kWavesPerBlock) void det_emit_kernel(
    const float* __restrict__ logits, long long ld, const float* __restrict__ seg32, const uint8_t* __restrict__ seg_ok,
    const int* __restrict__ row_offsets, const int* __restrict__ video_index, int R, int C, int Nq, float thr, float lo,
    long long capacity, float* __restrict__ seg, float* __restrict__ score, long long* __restrict__ key,
    int* __restrict__ rowid) {
  const int lane = threadIdx.x & 63;
  const int wave = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  const int nwaves = gridDim.x * kWavesPerBlock;
  for (int r = wave; r < R; r += nwaves) {
    if (!seg_ok[r]) continue;                                  // its logits are not read at all
    long long base = row_offsets[r];
    const long long end = cand_row_end(row_offsets, r, capacity);
    if (base >= end) continue;
    const float s0 = seg32[2 * (size_t)r], s1 = seg32[2 * (size_t)r + 1];
    const long long key0 = (long long)video_index[r / Nq] * (long long)C;
    const float* row = logits + (size_t)r * (size_t)ld;
    for (int cb = 0; cb < C; cb += 256) {
      float x[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int c = cb + 64 * k + lane;
        x[k] = c < C ? row[c] : -INFINITY;
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int c = cb + 64 * k + lane;
        float s = 0.f;
        bool pass = false;
        if (!(x[k] < lo) && c < C) { s = cand_sigmoid(x[k]); pass = s > thr; }
        const unsigned long long m = __ballot(pass);
        const long long pos = base + __popcll(m & lanes_below(lane));
        if (pass && pos < end) {
          seg[2 * pos] = s0;
          seg[2 * pos + 1] = s1;
          score[pos] = s;
          key[pos] = key0 + c;
          rowid[pos] = r;
        }
        base += __popcll(m);
      }
    }
  }
}

// fp32 bounds of the pre-filter (derivation at the top of the file)
void det_bounds(float thr, float* lo, float* hi) {
  const double t = (double)thr;
  if (!(t == t)) { *lo = INFINITY; *hi = INFINITY; return; }     // NaN threshold: nothing compares greater
  if (t >= 1.0) { *lo = INFINITY; *hi = INFINITY; return; }       // no fp32 sigmoid exceeds 1
  if (t < 0.0) { *lo = -INFINITY; *hi = -INFINITY; return; }      // every finite or infinite logit passes (NaN: fp64 path)
  // lo
  if (t == 0.0) {
    *lo = -INFINITY;                                              // the fp64 path decides which scores round to zero
  } else {
    const double l = log(t / (1.0 - t));
    const double m = l - 1e-5 * (1.0 + fabs(l));
    *lo = nextafterf((float)m, -INFINITY);
  }
  // hi
  const float t2 = nextafterf(nextafterf(thr, INFINITY), INFINITY);
  if ((double)t2 >= 1.0) {
    *hi = INFINITY;
  } else {
    const double l = log((double)t2 / (1.0 - (double)t2));
    const double m = l + 1e-5 * (1.0 + fabs(l));
    *hi = nextafterf((float)m, INFINITY);
  }
}

int det_check_shape(int R, int C, long long ld, int Nq) {
  if (R < 0 || C < 1 || Nq < 1 || ld < C || R % Nq != 0) return TIMHIP_EINVAL;
  if ((long long)R * (long long)C > 0x7fffffffLL) return TIMHIP_EUNSUPPORTED;   // the offsets are int32
  return TIMHIP_OK;
}

}  // namespace

extern "C" {

int timhip_det_candidates_count(const float* logits, int64_t ld_logits, const float* reg, const double* window_start,
                                float window_size, const float* max_time, int R, int C, int Nq, float score_threshold,
                                float* seg32, uint8_t* seg_ok, int32_t* row_offsets, void* stream) {
  if (!row_offsets) return TIMHIP_EINVAL;
  const int rc = det_check_shape(R, C, ld_logits, Nq);
  if (rc != TIMHIP_OK) return rc;
  if (R > 0 && (!logits || !reg || !window_start || !max_time || !seg32 || !seg_ok)) return TIMHIP_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  float lo, hi;
  det_bounds(score_threshold, &lo, &hi);
  if (R > 0) {
    hipLaunchKernelGGL(det_count_kernel, dim3(cand_grid(R)), dim3(64 * kWavesPerBlock), 0, s, logits, (long long)ld_logits,
                       reg, window_start, window_size, max_time, R, C, Nq, score_threshold, lo, hi, seg32, seg_ok,
                       row_offsets);
    TIM_CHECK_LAUNCH();
  }
  return cand_scan(row_offsets, R, s);
}

int timhip_det_candidates_emit(const float* logits, int64_t ld_logits, const float* seg32, const uint8_t* seg_ok,
                               const int32_t* row_offsets, const int32_t* video_index, int R, int C, int Nq,
                               float score_threshold, int64_t capacity, float* seg, float* score, int64_t* key,
                               int32_t* row, void* stream) {
  const int rc = det_check_shape(R, C, ld_logits, Nq);
  if (rc != TIMHIP_OK) return rc;
  if (capacity < 0) return TIMHIP_EINVAL;
  if (R == 0 || capacity == 0) return TIMHIP_OK;
  if (!logits || !seg32 || !seg_ok || !row_offsets || !video_index || !seg || !score || !key || !row) return TIMHIP_EINVAL;
  float lo, hi;
  det_bounds(score_threshold, &lo, &hi);
  hipLaunchKernelGGL(det_emit_kernel, dim3(cand_grid(R)), dim3(64 * kWavesPerBlock), 0, (hipStream_t)stream, logits,
                     (long long)ld_logits, seg32, seg_ok, row_offsets, video_index, R, C, Nq, score_threshold, lo,
                     (long long)capacity, seg, score, (long long*)key, row);
  TIM_CHECK_LAUNCH();
  return TIMHIP_OK;
}

}  // extern "C"
