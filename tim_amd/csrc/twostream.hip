// Two-stream detection fusion: the class logits and regressed segments of a verb stream and a noun stream
// over the same proposals become the (verb, noun) action candidates the per-video soft-NMS consumes.  It restates, per
// batch, what the reference does on the host in detection/eval_detection/format_two_stream_predictions_epic.py (main: the
// top k classes of each stream per proposal, the three thresholds, the fused score, the score-weighted blend of the two
// segments) on top of FeatureMeter.update's sigmoid and decode (detect.hip).
//
// The list is produced in the reference's order - proposal by proposal, verbs by descending score, nouns by descending
// score inside a verb - by select + scan + emit:
//   ts_select_kernel   one wavefront per proposal row: both rows of logits -> fp32 scores, the top k of each stream, the
//                      k * k pairs (one lane each) -> a small record per row and row_offsets[r + 1] = the survivors
//   det_scan_kernel    candidates.h, shared with detect.hip: in-place inclusive scan
//   ts_emit_kernel     reads only the records; survivor j of row r lands at row_offsets[r] + j
// No atomics and no look-back between workgroups: nothing depends on dispatch order.
//
// Arithmetic, operation by operation as the reference's arrays carry it (NumPy 2: an fp32 scalar combined with a Python
// float stays fp32):
//   vs, ns   = (float)(1.0 / (1.0 + exp(-(double)x)))     cand_sigmoid of candidates.h: the float64 sigmoid, one rounding
//   prop     = (double)(clamp(reg, 0, max_time) * window_size) + window_start     fp32 clamp and product, fp64 sum, per
//                                                          stream, NOT rounded (the saved v_proposals are float64)
//   pass     = vs > thr  &&  ns > thr  &&  score > thr     fp32 compares (a NaN fails them)
//   score    = (float)pow(vs, a32) * (float)pow(ns, b32)   each power the float64 pow rounded once to fp32 (reproducible on
//                                                          a CPU, as cand_sigmoid is), the product fp32 with one rounding
//   w        = vs / (vs + ns),  w1 = 1 - w                 fp32
//   seg      = (double)w * prop_v + (double)w1 * prop_n    two fp64 products, one fp64 add (contraction off)
//   seg      = rint(seg * 1000.0) / 1000.0                 numpy.round(seg, 3)
//   ok       = seg[1] - seg[0] > 0.0                       fp64; the segment is stored as fp32
//
// Selection is on the rounded fp32 score: equal scores go to the lower class index, a NaN ranks above every number (as
// NumPy sorts it) and then fails the threshold, so it costs its slot and nothing else.  Scores lie in [0, 1], so their bit
// patterns order as unsigned integers: (bits + 1, NaN -> all ones, 0 = retired) and the complement of the index make one
// 64-bit key whose wave-wide maximum (xor butterfly) is the round's winner.  A lane keeps the scores of the classes
// c = lane, lane + 64, ... in its own words of LDS (nobody else reads them: no barrier), so each logit is read once and
// each sigmoid evaluated once whatever k is.
//
// Loads are one dword per lane, 256 contiguous bytes per wave instruction: rows of 97 or 300 floats are not 16-byte aligned.
#include <math.h>

#include "common.h"

#pragma clang fp contract(off)   // ahead of candidates.h: its arithmetic is compiled under it as well
#include "candidates.h"

namespace {

constexpr int kMaxTopK = 8;           // k * k pairs, one lane each
constexpr int kMaxClasses = 4096;     // Cv + Cn: 4 waves * 4096 words = the 64 KiB of LDS a block may ask for

__device__ __forceinline__ unsigned ts_key(float s) { return s != s ? 0xffffffffu : __float_as_uint(s) + 1u; }
__device__ __forceinline__ float ts_unkey(unsigned k) {
  return k == 0xffffffffu ? __uint_as_float(0x7fc00000u) : __uint_as_float(k - 1u);
}

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const unsigned lo = __shfl_xor((unsigned)v, o, 64), hi = __shfl_xor((unsigned)(v >> 32), o, 64);
    const unsigned long long u = ((unsigned long long)hi << 32) | lo;
    v = u > v ? u : v;
  }
  return v;
}

// scores of one row into this lane's words of `keys`, then k rounds of maximum; lane j < k returns winner j
__device__ __forceinline__ void ts_top_k(const float* __restrict__ row, int C, int k, int lane, unsigned* keys, unsigned* my_key,
                                         int* my_idx) {
  for (int c = lane; c < C; c += 64) keys[c] = ts_key(cand_sigmoid(row[c]));
  *my_key = 0u;
  *my_idx = 0;
  for (int j = 0; j < k; ++j) {
    unsigned long long best = 0ull;
    for (int c = lane; c < C; c += 64) {
      const unsigned long long v = ((unsigned long long)keys[c] << 32) | (unsigned long long)(0xffffffffu - (unsigned)c);
      best = v > best ? v : best;
    }
    best = wave_max_u64(best);
    const int c = (int)(0xffffffffu - (unsigned)best);
    if (c >= 0 && c < C && (c & 63) == lane) keys[c] = 0u;   // retired (its owner is the only lane that reads it)
    if (lane == j) { *my_key = (unsigned)(best >> 32); *my_idx = c; }
  }
}

__global__ __launch_bounds__(64 * kWavesPerBlock) void ts_select_kernel(
    const float* __restrict__ verb_logits, long long ld_v, const float* __restrict__ noun_logits, long long ld_n,
    const float* __restrict__ verb_reg, const float* __restrict__ noun_reg, const double* __restrict__ window_start,
    float window_size, const float* __restrict__ max_time, int R, int Cv, int Cn, int Nq, int k, float thr, float a32, float b32,
    int* __restrict__ sel_idx, float* __restrict__ sel_score, float* __restrict__ pair_score, float* __restrict__ pair_seg,
    unsigned long long* __restrict__ pair_mask, int* __restrict__ row_offsets) {
  extern __shared__ unsigned ts_lds[];
  const int lane = threadIdx.x & 63;
  unsigned* keys = ts_lds + (size_t)(threadIdx.x >> 6) * (size_t)(Cv + Cn);
  const int wave = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  const int nwaves = gridDim.x * kWavesPerBlock;
  const float tmax = max_time[0];
  const int kk = k * k;
  for (int r = wave; r < R; r += nwaves) {
    unsigned vkey, nkey;
    int vidx, nidx;
    ts_top_k(verb_logits + (size_t)r * (size_t)ld_v, Cv, k, lane, keys, &vkey, &vidx);
    ts_top_k(noun_logits + (size_t)r * (size_t)ld_n, Cn, k, lane, keys + Cv, &nkey, &nidx);
    if (lane < k) {
      const size_t o = (size_t)r * (size_t)(2 * k) + lane;
      sel_idx[o] = vidx;
      sel_idx[o + k] = nidx;
      sel_score[o] = ts_unkey(vkey);
      sel_score[o + k] = ts_unkey(nkey);
    }
    // ---- lane p < k * k owns pair (p / k, p % k); the other lanes compute on pair 0 and store nothing
    const int p = lane < kk ? lane : 0;
    const float vs = ts_unkey(__shfl(vkey, p / k, 64)), ns = ts_unkey(__shfl(nkey, p % k, 64));
    const float A = (float)pow((double)vs, (double)a32), B = (float)pow((double)ns, (double)b32);
    const float score = __fmul_rn(A, B);
    const float w = __fdiv_rn(vs, __fadd_rn(vs, ns)), w1 = __fsub_rn(1.0f, w);
    const double ws = window_start[r / Nq];
    double s[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const double pv = cand_decode(verb_reg[2 * (size_t)r + e], tmax, window_size, ws);
      const double pn = cand_decode(noun_reg[2 * (size_t)r + e], tmax, window_size, ws);
      s[e] = cand_round3(__dadd_rn(__dmul_rn((double)w, pv), __dmul_rn((double)w1, pn)));
    }
    const bool pass = lane < kk && vs > thr && ns > thr && score > thr && __dsub_rn(s[1], s[0]) > 0.0;
    const unsigned long long m = __ballot(pass);
    if (lane < kk) {
      const size_t o = (size_t)r * (size_t)kk + lane;
      pair_score[o] = score;
      pair_seg[2 * o] = (float)s[0];
      pair_seg[2 * o + 1] = (float)s[1];
    }
    if (lane == 0) {
      pair_mask[r] = m;
      row_offsets[r + 1] = __popcll(m);
    }
  }
}

// one thread per (row, pair): the records only
__global__ __launch_bounds__(256) void ts_emit_kernel(
    const int* __restrict__ sel_idx, const float* __restrict__ pair_score, const float* __restrict__ pair_seg,
    const unsigned long long* __restrict__ pair_mask, const int* __restrict__ row_offsets, const int* __restrict__ video_index,
    int R, int Cv, int Cn, int Nq, int k, long long capacity, float* __restrict__ seg, float* __restrict__ score,
    long long* __restrict__ key, int* __restrict__ rowid) {
  const int kk = k * k;
  const long long total = (long long)R * kk, step = (long long)gridDim.x * blockDim.x;
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += step) {
    const int r = (int)(t / kk), p = (int)(t - (long long)r * kk);
    const unsigned long long m = pair_mask[r];
    if (!((m >> p) & 1ull)) continue;
    const long long end = cand_row_end(row_offsets, r, capacity);
    const long long pos = (long long)row_offsets[r] + __popcll(m & lanes_below(p));
    if (pos < 0 || pos >= end) continue;
    const int verb = sel_idx[(size_t)r * (size_t)(2 * k) + p / k], noun = sel_idx[(size_t)r * (size_t)(2 * k) + k + p % k];
    seg[2 * pos] = pair_seg[2 * t];
    seg[2 * pos + 1] = pair_seg[2 * t + 1];
    score[pos] = pair_score[t];
    key[pos] = (long long)video_index[r / Nq] * ((long long)Cv * (long long)Cn) + (long long)verb * Cn + noun;
    rowid[pos] = r;
  }
}

int ts_check_shape(int R, int Cv, int Cn, int Nq, int k) {
  if (R < 0 || Cv < 1 || Cn < 1 || Nq < 1 || R % Nq != 0 || k < 1 || k > (Cv < Cn ? Cv : Cn)) return TIMHIP_EINVAL;
  if (k > kMaxTopK || (long long)Cv + (long long)Cn > kMaxClasses) return TIMHIP_EUNSUPPORTED;
  if ((long long)R * (long long)k * (long long)k > 0x7fffffffLL) return TIMHIP_EUNSUPPORTED;   // the offsets are int32
  return TIMHIP_OK;
}

}  // namespace

extern "C" {

int timhip_ts_candidates_count(const float* verb_logits, int64_t ld_v, const float* noun_logits, int64_t ld_n,
                               const float* verb_reg, const float* noun_reg, const double* window_start, float window_size,
                               const float* max_time, int R, int Cv, int Cn, int Nq, int top_k, float score_threshold,
                               float alpha32, float beta32, int32_t* sel_idx, float* sel_score, float* pair_score,
                               float* pair_seg, uint64_t* pair_mask, int32_t* row_offsets, void* stream) {
  if (!row_offsets) return TIMHIP_EINVAL;
  const int rc = ts_check_shape(R, Cv, Cn, Nq, top_k);
  if (rc != TIMHIP_OK) return rc;
  if (ld_v < Cv || ld_n < Cn) return TIMHIP_EINVAL;
  if (R > 0 && (!verb_logits || !noun_logits || !verb_reg || !noun_reg || !window_start || !max_time || !sel_idx ||
                !sel_score || !pair_score || !pair_seg || !pair_mask))
    return TIMHIP_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  if (R > 0) {
    const size_t lds = (size_t)kWavesPerBlock * (size_t)(Cv + Cn) * sizeof(unsigned);
    hipLaunchKernelGGL(ts_select_kernel, dim3(cand_grid(R)), dim3(64 * kWavesPerBlock), lds, s, verb_logits, (long long)ld_v,
                       noun_logits, (long long)ld_n, verb_reg, noun_reg, window_start, window_size, max_time, R, Cv, Cn, Nq,
                       top_k, score_threshold, alpha32, beta32, sel_idx, sel_score, pair_score, pair_seg,
                       (unsigned long long*)pair_mask, row_offsets);
    TIM_CHECK_LAUNCH();
  }
  return cand_scan(row_offsets, R, s);
}

int timhip_ts_candidates_emit(const int32_t* sel_idx, const float* pair_score, const float* pair_seg, const uint64_t* pair_mask,
                              const int32_t* row_offsets, const int32_t* video_index, int R, int Cv, int Cn, int Nq, int top_k,
                              int64_t capacity, float* seg, float* score, int64_t* key, int32_t* row, void* stream) {
  const int rc = ts_check_shape(R, Cv, Cn, Nq, top_k);
  if (rc != TIMHIP_OK) return rc;
  if (capacity < 0) return TIMHIP_EINVAL;
  if (R == 0 || capacity == 0) return TIMHIP_OK;
  if (!sel_idx || !pair_score || !pair_seg || !pair_mask || !row_offsets || !video_index || !seg || !score || !key || !row)
    return TIMHIP_EINVAL;
  const long long total = (long long)R * top_k * top_k;
  long long blocks = (total + 255) / 256;
  if (blocks > kMaxBlocks) blocks = kMaxBlocks;
  hipLaunchKernelGGL(ts_emit_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, sel_idx, pair_score, pair_seg,
                     (const unsigned long long*)pair_mask, row_offsets, video_index, R, Cv, Cn, Nq, top_k, (long long)capacity,
                     seg, score, (long long*)key, row);
  TIM_CHECK_LAUNCH();
  return TIMHIP_OK;
}

}  // extern "C"
