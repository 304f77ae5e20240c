// Detection meter: the eleven loss averages of the reference's detection TrainMeter / InferenceMeter
// (detection/time_interval_machine/utils/meters.py:94-137, :383-423) in one small STATE BLOCK in device memory
// (include/timhip.h: TIMHIP_DET_METER_*).  Its inputs are the side statistics timhip_det_side_loss_fwd_stats leaves behind
// (losses.hip): nothing is read from the logits here, and the host reads nothing.
//
//   det_meter_kernel   one block of 64 threads: the state and the two stats blocks come into LDS with one load per thread, ONE
//                      thread updates the counters and the slots in their fixed order, sum = sum + (double)val * n with the
//                      product rounded before the add, and the block goes back with one store per thread.
// No atomics, nothing depends on a dispatch order: a replayed graph leaves the bits an eager call leaves.  Contraction is off.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 64;
static_assert(TIMHIP_DET_METER_STATE_WORDS <= 2 * kThreads && 2 * TIMHIP_DET_SIDE_STATS_WORDS <= kThreads, "one or two words per thread");

// AverageMeter.update(val, n): the product is rounded on its own, then added
__device__ __forceinline__ void det_slot(uint32_t* st, int slot, float val, long long n) {
  double* sum = (double*)(st + TIMHIP_DET_METER_SUM + 4 * slot);
  long long* count = (long long*)(st + TIMHIP_DET_METER_COUNT + 4 * slot);
  ((float*)st)[TIMHIP_DET_METER_VAL + slot] = val;
  *sum = __dadd_rn(*sum, __dmul_rn((double)val, (double)n));
  *count = *count + n;
}

__global__ __launch_bounds__(kThreads) void det_meter_kernel(uint32_t* __restrict__ st, const float* __restrict__ visual,
                                                             const float* __restrict__ audio, int nheads,
                                                             const float* __restrict__ total_loss,
                                                             const float* __restrict__ drloc_loss) {
  __shared__ __attribute__((aligned(8))) uint32_t blk[TIMHIP_DET_METER_STATE_WORDS];
  __shared__ float side[2][TIMHIP_DET_SIDE_STATS_WORDS];
  __shared__ float loss[2];
  const int tid = threadIdx.x;
  for (int i = tid; i < TIMHIP_DET_METER_STATE_WORDS; i += kThreads) blk[i] = st[i];
  if (tid < 2 * TIMHIP_DET_SIDE_STATS_WORDS) {
    const int s = tid / TIMHIP_DET_SIDE_STATS_WORDS, w = tid - s * TIMHIP_DET_SIDE_STATS_WORDS;
    const float* p = s == 0 ? visual : audio;
    side[s][w] = p ? p[w] : 0.f;
  }
  if (tid == kThreads - 1) {
    loss[0] = total_loss ? total_loss[0] : 0.f;
    loss[1] = drloc_loss ? drloc_loss[0] : 0.f;
  }
  __syncthreads();
  if (tid == 0) {
    const float* v = side[0];
    const float* a = side[1];
    int32_t* sti = (int32_t*)blk;
    long long* updates = (long long*)(blk + TIMHIP_DET_METER_UPDATES);
    *updates = *updates + 1;
    long long cnt[2][2];   // (side, valid / positives): exact floats, rows <= 2^24
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      cnt[s][0] = (long long)side[s][TIMHIP_DET_STAT_VALID];
      cnt[s][1] = (long long)side[s][TIMHIP_DET_STAT_POSITIVES];
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        sti[TIMHIP_DET_METER_LAST + 2 * s + k] = (int32_t)cnt[s][k];
        long long* run = (long long*)(blk + TIMHIP_DET_METER_RUN + 4 * s + 2 * k);
        *run = *run + cnt[s][k];
      }
      ((float*)blk)[TIMHIP_DET_METER_NORM + s] = side[s][TIMHIP_DET_STAT_NORMALISER];
    }
    const long long v_cls = cnt[0][0], v_pos = cnt[0][1], a_cls = cnt[1][0], a_pos = cnt[1][1];
    // the conditions and the order of the reference's update(): meters.py:113-137
    if (v_cls > 0) {
      det_slot(blk, TIMHIP_DET_METER_VISUAL, v[TIMHIP_DET_STAT_CLS], v_cls);
      if (nheads == 3) {
        det_slot(blk, TIMHIP_DET_METER_VERB, v[TIMHIP_DET_STAT_HEAD + 0], v_cls);
        det_slot(blk, TIMHIP_DET_METER_NOUN, v[TIMHIP_DET_STAT_HEAD + 1], v_cls);
      }
      det_slot(blk, TIMHIP_DET_METER_ACTION, nheads == 3 ? v[TIMHIP_DET_STAT_HEAD + 2] : v[TIMHIP_DET_STAT_HEAD], v_cls);
      det_slot(blk, TIMHIP_DET_METER_VISUAL_REG, v[TIMHIP_DET_STAT_REG], v_pos);
      det_slot(blk, TIMHIP_DET_METER_POSITIVE, v[TIMHIP_DET_STAT_POS], v_pos);
      det_slot(blk, TIMHIP_DET_METER_NEGATIVE, v[TIMHIP_DET_STAT_NEG], v_cls - v_pos);
    }
    if (a_cls > 0) {
      det_slot(blk, TIMHIP_DET_METER_AUDIO, a[TIMHIP_DET_STAT_CLS], a_cls);
      det_slot(blk, TIMHIP_DET_METER_AUDIO_REG, a[TIMHIP_DET_STAT_REG], a_pos);
      det_slot(blk, TIMHIP_DET_METER_POSITIVE, a[TIMHIP_DET_STAT_POS], a_pos);
      det_slot(blk, TIMHIP_DET_METER_NEGATIVE, a[TIMHIP_DET_STAT_NEG], a_cls - a_pos);
    }
    det_slot(blk, TIMHIP_DET_METER_TOTAL, loss[0], v_cls + a_cls);
    det_slot(blk, TIMHIP_DET_METER_DRLOC, loss[1], v_cls + a_cls);
  }
  __syncthreads();
  for (int i = tid; i < TIMHIP_DET_METER_STATE_WORDS; i += kThreads) st[i] = blk[i];
}

}  // namespace

extern "C" {

int timhip_det_meter_update(void* state, const float* const* sides, int nheads, const float* total_loss, const float* drloc_loss,
                            void* stream) {
  if (!state || !sides || (!sides[0] && !sides[1]) || (nheads != 1 && nheads != 3)) return TIMHIP_EINVAL;
  if (((uintptr_t)state & 7) != 0) return TIMHIP_EALIGN;
  hipLaunchKernelGGL(det_meter_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, (uint32_t*)state, sides[0], sides[1], nheads,
                     total_loss, drloc_loss);
  TIM_CHECK_LAUNCH();
  return TIMHIP_OK;
}

}  // extern "C"
