// Attention of query rows against cached keys and values (evaluation only): a window's feature stream never depends on the
// queries and queries never depend on each other (tim.py:161-166), so the K | V rows of the F feature tokens of every layer can be
// kept (timhip_stack_encode) and any number of query rows run against them later (timhip_stack_query).
//
// Every row is a query row: softmax over the F cached keys of window widx[g] plus the row's own key,
//   o = sum_j p_j V_j + p_self v_own.
// No dropout, no log-sum-exp store.  The arithmetic is the full forward's: both kernels here are the bodies of attention.h
// (attn_fwd_mfma_body / attn_fwd_simple_body) with QRY = true, which changes where a block finds its rows and its keys and
// nothing about what it does with them - the outputs equal timhip_attention_fwd's query rows bit for bit on equal inputs.
//
// 16-bit operands run the matrix-core body for every (head width, key blocks) pair of attn_for_shape.  Everything else - fp32,
// bf16x3, other head widths, other F - runs the fp32-arithmetic body (the exact-fp32 matrix-core kernels of attention_f32.hip
// stage K and V per pass over one LDS tile and have no row split; they are not shared here).
#include "attention.h"

namespace {

template <typename HT, int DH, int NJB>
__global__ __launch_bounds__(512) void attn_query_mfma(const HT* __restrict__ qkv_q, HT* __restrict__ o, AttnArgs a, AttnQuerySrc qs) {
  attn_fwd_mfma_body<HT, DH, NJB, false, true>(qkv_q, o, nullptr, a, qs);
}

template <typename T>
__global__ __launch_bounds__(256) void attn_query_simple(const T* __restrict__ qkv_q, T* __restrict__ o, AttnArgs a, AttnQuerySrc qs) {
  attn_fwd_simple_body<T, true>(qkv_q, o, nullptr, a, qs);
}

// (the geometry of attention_mfma.hip's launcher: at most four waves, row blocks split over workgroups when G * H leaves CUs idle)
template <typename HT, int DH, int NJB>
int launch_query(const TimDesc& d, const void* qkv_q, const AttnQuerySrc& qs, void* o, hipStream_t s) {
  const size_t lds = (size_t)2 * NJB * 32 * DH * 2;
  AttnArgs a = make_attn_args(d);
  attn_row_split(d, 0, d.B * d.H < 128 ? tim_knobs().attn_split_min : 4, a.rsplit, a.rper);
  const int waves = attn_waves(32 * a.rper, 4, true);
  (void)hipFuncSetAttribute((const void*)attn_query_mfma<HT, DH, NJB>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL((attn_query_mfma<HT, DH, NJB>), dim3(d.B * d.H * a.rsplit), dim3(64 * waves), lds, s, (const HT*)qkv_q, (HT*)o, a,
                     qs);
  return hipGetLastError() == hipSuccess ? TIMHIP_OK : TIMHIP_ELAUNCH;
}

}  // namespace

int tim_attention_query_fwd(const TimDesc& d, const void* qkv_q, const void* kv, int ldkv, int wrows, int W, const int* widx, void* o,
                            hipStream_t s) {
  if (d.B <= 0 || d.S <= 0 || d.F <= 0 || d.H <= 0 || d.E <= 0 || d.E % d.H || W <= 0) return TIMHIP_EINVAL;
  if (!valid_precision(d.precision)) return TIMHIP_EUNSUPPORTED;
  if (!qkv_q || !kv || !o || d.p_drop != 0.f) return TIMHIP_EINVAL;
  if (ldkv < 2 * d.E || wrows < d.F || (!widx && d.B != W)) return TIMHIP_EINVAL;
  const size_t ts = opsize(d.precision);
  // (the matrix-core body reads 16-byte chunks)
  const bool al16 = (d.E % 8) == 0 && (ldkv % 8) == 0 && (((uintptr_t)qkv_q | (uintptr_t)kv | (uintptr_t)o) & 15) == 0;
  if ((((uintptr_t)qkv_q | (uintptr_t)kv | (uintptr_t)o) & (ts - 1)) != 0) return TIMHIP_EALIGN;
  TimGemmScope timing(((double)d.B * d.S * d.E * 4 + (double)d.B * d.F * d.E * 2) * ts, s, 1);
  const AttnQuerySrc qs{kv, widx, ldkv, wrows, W};
  if (h16_storage(d.precision) && !(d.reserved & 1) && al16) {   // reserved bit 0: force the fp32-arithmetic kernel
    const int rc = attn_for_shape(d.E / d.H, (d.F + 31) / 32, [&](auto dh, auto njb) {
      DISPATCH_H16(d.precision, return (launch_query<HT, decltype(dh)::value, decltype(njb)::value>(d, qkv_q, qs, o, s)));
    });
    if (rc != TIMHIP_EUNSUPPORTED) return rc;
  }
  if (d.F > 64 * KPL) return TIMHIP_EUNSUPPORTED;
  const size_t lds = simple_lds(d, 1);
  if (lds > 160 * 1024) return TIMHIP_EUNSUPPORTED;
  const AttnArgs a = make_attn_args(d);
  DISPATCH_T(d.precision,
    (void)hipFuncSetAttribute((const void*)attn_query_simple<T>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(attn_query_simple<T>, dim3(d.B * d.H), dim3(256), lds, s, (const T*)qkv_q, (T*)o, a, qs));
  TIM_CHECK_LAUNCH();
  return TIMHIP_OK;
}

extern "C" int timhip_attention_query_fwd(const TimDesc* d, const void* qkv_q, const void* kv, int ldkv, int wrows, int W,
                                          const int* widx, void* o, void* stream) {
  if (!d) return TIMHIP_EINVAL;
  return tim_attention_query_fwd(*d, qkv_q, kv, ldkv, wrows, W, widx, o, (hipStream_t)stream);
}
