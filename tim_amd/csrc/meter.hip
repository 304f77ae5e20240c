// Training meter: the numbers a person watches while a recognition model trains - the loss averages and the
// top-1 / top-5 accuracies of the batch and of the run so far - kept in one small STATE BLOCK in device memory
// (include/timhip.h: TIMHIP_METER_*), so that a captured iteration updates them with launches only and a logger reads them with
// one copy of the block.  It restates the loss side of the reference's TrainMeter (recognition/time_interval_machine/utils/
// meters.py:13-29, :140-167: AverageMeter.update with the valid counts as weights) and adds what the reference has only at the
// end of an epoch, an accuracy: the rank of every valid row's label over that row's raw logits, rec_finalize_kernel's rank.
//
//   meter_rank_kernel     one wavefront per (head, row, segment of up to 1,024 columns): the segment's share of
//                         #{c : x_c > x_y} + #{c < y : x_c == x_y} -> work (kRowPadded: the row is padding; kRowNoRank: the label is
//                         outside [0, C) or x_y is NaN).  Every word of `work` has one writer.
//   meter_finish_kernel   one block: the valid counts nv / na from the labels, a row's rank as the sum of its segments, the
//                         counters as integer sums over the block (the order of integer adds does not matter), then ONE thread
//                         updates the block (staged in LDS: one load and one store per word): the last-batch words, the
//                         running int64 counters, and the seven loss slots in their fixed order, sum = sum + (double)val * n
//                         with the product rounded before the add.
// No floating-point atomics; nothing here depends on the dispatch order, so a replayed graph leaves the bits an eager call
// leaves.  The unit is compiled with contraction off.  Loads are one dword per lane, 256 contiguous bytes per wave instruction,
// the chunks of a segment in flight together, as in recog.hip: rows of 97 or 3,806 floats are not 16-byte aligned.
#include <math.h>

#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kWavesPerBlock = 4;
constexpr int kMaxBlocks = 2048;   // a memory-bound grid: cap it and stride over the items
constexpr int kChunk = 256;        // columns of one wave instruction row: 4 dwords per lane
constexpr int kSegChunks = 4;      // chunks of one work item: 16 dwords per lane in flight, 4 items for a 3,806-wide row
constexpr int kSeg = kChunk * kSegChunks;
constexpr int kMaxHeads = 2 * TIMHIP_METER_MAX_HEADS;
constexpr int kRowPadded = -1, kRowNoRank = -2;   // work words that are not a count
constexpr int kNoRank = 0x7fffffff;
constexpr int kFinishThreads = 1024;
constexpr int kCounters = 3 * TIMHIP_METER_HEADS + 2;   // (rows, top-1, top-5) per head, then nv, na

struct MeterHeads {
  const float* logits[kMaxHeads];
  long long ld[kMaxHeads];
  int C[kMaxHeads];
  int label_col[kMaxHeads];
  int slot[kMaxHeads];      // TIMHIP_METER_HEAD_*
  int nseg[kMaxHeads];      // work items of a row of head h
  int start[kMaxHeads];     // first work word (= first item) of head h
  int n, n_visual;          // heads in all, and how many of them are visual (they come first)
};

// (a select chain, not an indexed read: the struct is a kernel argument and stays in scalar registers this way)
template <typename T> __device__ __forceinline__ T pick(int h, const T (&a)[kMaxHeads]) {
  return h == 0 ? a[0] : (h == 1 ? a[1] : (h == 2 ? a[2] : (h == 3 ? a[3] : (h == 4 ? a[4] : a[5]))));
}

struct MeterLabels {
  const long long* v;       // [Rv, >= 3]: verb, noun, action; a visual row is valid iff its action label is not -1
  const long long* a;       // [Ra, >= 1]: a row is valid iff its class id is not -1
  long long ldv, lda;
  int Rv, Ra;
};

__global__ __launch_bounds__(64 * kWavesPerBlock) void meter_rank_kernel(MeterHeads hd, MeterLabels lb, int items,
                                                                         int* __restrict__ work) {
  const int lane = threadIdx.x & 63;
  const int wave = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  const int nwaves = gridDim.x * kWavesPerBlock;
  for (int it = wave; it < items; it += nwaves) {
    int h = 0;
#pragma unroll
    for (int k = 1; k < kMaxHeads; ++k) h += (k < hd.n && it >= hd.start[k]);
    const int nseg = pick(h, hd.nseg);
    const int local = it - pick(h, hd.start);
    const int r = local / nseg, s = local - r * nseg;
    const bool vis = h < hd.n_visual;
    const long long* lrow = vis ? lb.v + (size_t)r * (size_t)lb.ldv : lb.a + (size_t)r * (size_t)lb.lda;
    if (lrow[vis ? 2 : 0] == -1) {
      if (lane == 0) work[it] = kRowPadded;
      continue;
    }
    const int C = pick(h, hd.C);
    const long long y = lrow[pick(h, hd.label_col)];
    const float* row = pick(h, hd.logits) + (size_t)r * (size_t)pick(h, hd.ld);
    const bool has = y >= 0 && y < (long long)C;
    const float xy = has ? row[y] : 0.0f;
    if (!has || xy != xy) {
      if (lane == 0) work[it] = kRowNoRank;
      continue;
    }
    const int lab = (int)y;
    const int c0 = s * kSeg;
    float x[kSegChunks][4];
#pragma unroll
    for (int q = 0; q < kSegChunks; ++q) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int c = c0 + q * kChunk + 64 * k + lane;
        x[q][k] = c < C ? row[c] : 0.0f;
      }
    }
    int above = 0;
#pragma unroll
    for (int q = 0; q < kSegChunks; ++q) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int c = c0 + q * kChunk + 64 * k + lane;
        above += c < C && (x[q][k] > xy || (x[q][k] == xy && c < lab));
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) above += __shfl_xor(above, o, 64);
    if (lane == 0) work[it] = above;
  }
}

// the rank of row r under head h from its work words (kNoRank: no usable label); the row is known to be valid
__device__ __forceinline__ int row_rank(const MeterHeads& hd, int h, int r, const int* __restrict__ work) {
  const int nseg = pick(h, hd.nseg);
  const int* w = work + pick(h, hd.start) + (size_t)r * nseg;
  if (w[0] == kRowNoRank) return kNoRank;
  int rank = 0;
  for (int s = 0; s < nseg; ++s) rank += w[s];
  return rank;
}

// AverageMeter.update(val, n): the product is rounded on its own, then added
__device__ __forceinline__ void loss_slot(uint32_t* st, int slot, float val, long long n) {
  double* sum = (double*)(st + TIMHIP_METER_SUM + 4 * slot);
  long long* count = (long long*)(st + TIMHIP_METER_COUNT + 4 * slot);
  ((float*)st)[TIMHIP_METER_VAL + slot] = val;
  *sum = __dadd_rn(*sum, __dmul_rn((double)val, (double)n));
  *count = *count + n;
}

struct MeterLosses {
  const float* p[TIMHIP_METER_SLOTS];   // device scalars; NULL: the loss counts as 0
};

__global__ __launch_bounds__(kFinishThreads) void meter_finish_kernel(MeterHeads hd, MeterLabels lb, MeterLosses ls, int flags,
                                                                      const int* __restrict__ work,
                                                                      uint32_t* __restrict__ st) {
  __shared__ int part[kCounters][kFinishThreads / 64];
  __shared__ __attribute__((aligned(8))) uint32_t blk[TIMHIP_METER_STATE_WORDS];
  __shared__ float val[TIMHIP_METER_SLOTS];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  // the block and the loss scalars come in with one load per thread while the rows are counted: the one thread that does the
  // arithmetic then works in LDS, not through some fifty dependent round trips to memory
  if (tid < TIMHIP_METER_STATE_WORDS) blk[tid] = st[tid];
  if (tid == kFinishThreads - 1) {
#pragma unroll
    for (int i = 0; i < TIMHIP_METER_SLOTS; ++i) val[i] = ls.p[i] ? *ls.p[i] : 0.0f;
  }
  const bool ranks = (flags & TIMHIP_METER_BATCH_ACCURACY) != 0;
  int v[kCounters];
#pragma unroll
  for (int i = 0; i < kCounters; ++i) v[i] = 0;
  // (a counter index is a compile-time constant everywhere below: the array stays in registers)
  auto tally = [&](int slot, int rank) {
#pragma unroll
    for (int t = 0; t < TIMHIP_METER_HEADS; ++t) {
      v[3 * t + 0] += slot == t;
      v[3 * t + 1] += slot == t && rank < 1;
      v[3 * t + 2] += slot == t && rank < 5;
    }
  };
  for (int r = tid; r < lb.Rv; r += kFinishThreads) {
    if (lb.v[(size_t)r * (size_t)lb.ldv + 2] == -1) continue;
    v[3 * TIMHIP_METER_HEADS] += 1;
    if (!ranks) continue;
    int verb = -1, noun = -1;
#pragma unroll
    for (int h = 0; h < TIMHIP_METER_MAX_HEADS; ++h) {
      if (h >= hd.n_visual) continue;
      const int slot = pick(h, hd.slot);
      const int rank = row_rank(hd, h, r, work);
      tally(slot, rank);
      verb = slot == TIMHIP_METER_HEAD_VERB ? rank : verb;
      noun = slot == TIMHIP_METER_HEAD_NOUN ? rank : noun;
    }
    if (verb >= 0 && noun >= 0) tally(TIMHIP_METER_HEAD_MT, max(verb, noun));
  }
  for (int r = tid; r < lb.Ra; r += kFinishThreads) {
    if (lb.a[(size_t)r * (size_t)lb.lda] == -1) continue;
    v[3 * TIMHIP_METER_HEADS + 1] += 1;
    if (!ranks) continue;
#pragma unroll
    for (int k = 0; k < TIMHIP_METER_MAX_HEADS; ++k) {
      const int h = hd.n_visual + k;
      if (h >= hd.n) continue;
      tally(pick(h, hd.slot), row_rank(hd, h, r, work));
    }
  }
#pragma unroll
  for (int i = 0; i < kCounters; ++i) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[i] += __shfl_xor(v[i], o, 64);
    if (lane == 0) part[i][w] = v[i];
  }
  __syncthreads();
  if (tid == 0) {
    int tot[kCounters];
#pragma unroll
    for (int i = 0; i < kCounters; ++i) {
      int s = 0;
#pragma unroll
      for (int k = 0; k < kFinishThreads / 64; ++k) s += part[i][k];
      tot[i] = s;
    }
    int32_t* sti = (int32_t*)blk;
    long long* updates = (long long*)(blk + TIMHIP_METER_UPDATES);
    *updates = *updates + 1;
#pragma unroll
    for (int i = 0; i < 3 * TIMHIP_METER_HEADS; ++i) {
      sti[TIMHIP_METER_LAST + i] = tot[i];
      long long* run = (long long*)(blk + TIMHIP_METER_RUN + 2 * i);
      *run = *run + (long long)tot[i];
    }
    const long long nv = tot[3 * TIMHIP_METER_HEADS], na = tot[3 * TIMHIP_METER_HEADS + 1];
    sti[TIMHIP_METER_NV] = (int32_t)nv;
    sti[TIMHIP_METER_NA] = (int32_t)na;
    // the conditions of the reference's update(): meters.py:140-167
    loss_slot(blk, TIMHIP_METER_TOTAL, val[TIMHIP_METER_TOTAL], nv + na);
    loss_slot(blk, TIMHIP_METER_DRLOC, val[TIMHIP_METER_DRLOC], nv + na);
    if (nv > 0) {
      loss_slot(blk, TIMHIP_METER_VISUAL, val[TIMHIP_METER_VISUAL], nv);
      if (flags & TIMHIP_METER_VERB_NOUN) {
        loss_slot(blk, TIMHIP_METER_VERB, val[TIMHIP_METER_VERB], nv);
        loss_slot(blk, TIMHIP_METER_NOUN, val[TIMHIP_METER_NOUN], nv);
      }
      loss_slot(blk, TIMHIP_METER_ACTION, val[TIMHIP_METER_ACTION], nv);
    }
    if (na > 0) loss_slot(blk, TIMHIP_METER_AUDIO, val[TIMHIP_METER_AUDIO], na);
  }
  __syncthreads();
  if (tid < TIMHIP_METER_STATE_WORDS) st[tid] = blk[tid];
}

// checks one group's heads and appends them to the table -> 0 or an error
int add_heads(MeterHeads& hd, const TimMeterHead* heads, int n, int R, int n_labels, long long& items) {
  for (int i = 0; i < n; ++i) {
    const TimMeterHead& x = heads[i];
    if (x.C < 1 || x.ld < x.C || (R > 0 && !x.logits)) return TIMHIP_EINVAL;
    if (x.label_col < 0 || x.label_col >= n_labels || x.slot < 0 || x.slot >= TIMHIP_METER_HEADS || x.slot == TIMHIP_METER_HEAD_MT)
      return TIMHIP_EINVAL;
    const int h = hd.n++;
    hd.logits[h] = x.logits; hd.ld[h] = x.ld; hd.C[h] = x.C; hd.label_col[h] = x.label_col; hd.slot[h] = x.slot;
    hd.nseg[h] = (x.C + kSeg - 1) / kSeg;
    if (items > 0x7fffffffLL) return TIMHIP_EUNSUPPORTED;
    hd.start[h] = (int)items;
    items += (long long)R * hd.nseg[h];
  }
  return TIMHIP_OK;
}

}  // namespace

extern "C" {

size_t timhip_meter_work_words(const TimMeterHead* v_heads, int n_v, int Rv, const TimMeterHead* a_heads, int n_a, int Ra) {
  if (n_v < 0 || n_a < 0 || n_v > TIMHIP_METER_MAX_HEADS || n_a > TIMHIP_METER_MAX_HEADS || Rv < 0 || Ra < 0) return 0;
  if ((n_v > 0 && !v_heads) || (n_a > 0 && !a_heads)) return 0;
  size_t words = 0;
  for (int i = 0; i < n_v; ++i) words += (size_t)Rv * (size_t)((v_heads[i].C > 0 ? v_heads[i].C + kSeg - 1 : 0) / kSeg);
  for (int i = 0; i < n_a; ++i) words += (size_t)Ra * (size_t)((a_heads[i].C > 0 ? a_heads[i].C + kSeg - 1 : 0) / kSeg);
  return words;
}

int timhip_meter_update(const TimMeterHead* v_heads, int n_v, const int64_t* v_labels, int64_t ld_v_labels, int Rv,
                        const TimMeterHead* a_heads, int n_a, const int64_t* a_labels, int64_t ld_a_labels, int Ra,
                        const float* const* losses, int flags, void* state, int32_t* work, void* stream) {
  if (!state || !losses || n_v < 0 || n_a < 0 || n_v > TIMHIP_METER_MAX_HEADS || n_a > TIMHIP_METER_MAX_HEADS) return TIMHIP_EINVAL;
  if (Rv < 0 || Ra < 0 || (n_v > 0 && !v_heads) || (n_a > 0 && !a_heads)) return TIMHIP_EINVAL;
  if (flags & ~(TIMHIP_METER_VERB_NOUN | TIMHIP_METER_BATCH_ACCURACY)) return TIMHIP_EINVAL;
  if ((Rv > 0 && (!v_labels || ld_v_labels < 3)) || (Ra > 0 && (!a_labels || ld_a_labels < 1))) return TIMHIP_EINVAL;
  if (((uintptr_t)state & 7) != 0) return TIMHIP_EALIGN;
  MeterHeads hd = {};
  long long items = 0;
  int rc = add_heads(hd, v_heads, n_v, Rv, 3, items);
  if (rc != TIMHIP_OK) return rc;
  hd.n_visual = hd.n;
  rc = add_heads(hd, a_heads, n_a, Ra, 1, items);
  if (rc != TIMHIP_OK) return rc;
  if (items > 0x7fffffffLL) return TIMHIP_EUNSUPPORTED;
  if (Rv == 0 && Ra == 0) return TIMHIP_OK;
  const bool ranks = (flags & TIMHIP_METER_BATCH_ACCURACY) && items > 0;
  if (ranks && !work) return TIMHIP_EINVAL;
  if (!ranks) flags &= ~TIMHIP_METER_BATCH_ACCURACY;
  MeterLabels lb = {(const long long*)v_labels, (const long long*)a_labels, (long long)ld_v_labels, (long long)ld_a_labels, Rv, Ra};
  MeterLosses ls;
  for (int i = 0; i < TIMHIP_METER_SLOTS; ++i) ls.p[i] = losses[i];
  hipStream_t s = (hipStream_t)stream;
  if (ranks) {
    const long long blocks = (items + kWavesPerBlock - 1) / kWavesPerBlock;
    hipLaunchKernelGGL(meter_rank_kernel, dim3((unsigned)(blocks > kMaxBlocks ? kMaxBlocks : blocks)), dim3(64 * kWavesPerBlock), 0,
                       s, hd, lb, (int)items, work);
    TIM_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(meter_finish_kernel, dim3(1), dim3(kFinishThreads), 0, s, hd, lb, ls, flags, (const int*)work,
                     (uint32_t*)state);
  TIM_CHECK_LAUNCH();
  return TIMHIP_OK;
}

}  // extern "C"
