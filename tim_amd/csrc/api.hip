// extern "C" stage entry points: one post-norm encoder layer forward/backward
// (transformers.py:92-111), plus small utilities.  Pure launch sequencing: no
// allocation, no synchronisation, no retained state.
#include <atomic>
#include "common.h"
#include "gemm_plan.h"
#include "wgrad_plan.h"

namespace {

struct SavedLayout {
  Field qkv, o, lse, y1, st1, x1t, u, h, y2, st2, ffn_mask, attn_keep;
  size_t total;
};

SavedLayout saved_layout(const TimDesc& d) {
  const size_t M = (size_t)d.B * d.S, ts = opsize(d.precision);
  Arena a;
  SavedLayout L;
  L.qkv = a.take(M * 3 * d.E * ts);
  L.o = a.take(M * d.E * ts);
  L.lse = a.take((size_t)d.B * d.H * d.S * 4);
  L.y1 = a.take(M * d.E * 4);
  L.st1 = a.take(M * 2 * 4);
  L.x1t = a.take(M * d.E * ts);
  L.u = a.take(M * d.FF * ts);
  L.h = a.take(M * d.FF * ts);
  L.y2 = a.take(M * d.E * 4);
  L.st2 = a.take(M * 2 * 4);
  L.ffn_mask = a.take(M * d.FF / 8);   // keep-bits of the FFN dropout (FF % 64 == 0): written by norm1, read by the linear1 epilogue
  L.attn_keep = a.take((size_t)d.B * d.H * d.S * 16);   // keep-bits of the attention dropout (timhip_attn_keep_bits, TIMHIP_DESC_ATTN_KEEP_BITS)
  L.total = a.total();
  return L;
}

// gradient operands handed from the data chain to the weight-gradient part: df[M,E] | du[M,FF] | da[M,E] | dqkv[M,3E]
struct DyLayout { Field df, du, da, dqkv; size_t total; };
DyLayout dy_layout(const TimDesc& d) {
  const size_t M = (size_t)d.B * d.S, ts = opsize(d.precision);
  Arena a;
  DyLayout L;
  L.df = a.take(M * d.E * ts);
  L.du = a.take(M * d.FF * ts);
  L.da = a.take(M * d.E * ts);
  L.dqkv = a.take(M * 3 * d.E * ts);
  L.total = a.total();
  return L;
}

// The four Linear products of a layer as weight-gradient items:
//   linear2: dW2 += df^T h ; linear1: dW1 += du^T x1 ; out-proj: dWo += da^T o ; in-proj: dWin += dqkv^T x_in
// in this order (the grouped kernels walk their tiles in item order).  saved / dy: the layer's saved block and the block its data
// chain left; all of saved, dy, x_in_T, g NULL: the shapes alone (workspace sizes, kernel choice).
void layer_products(const TimDesc& d, const void* saved, const void* dy, const void* x_in_T, const TimLayerGrads* g,
                    TimWgradItem it[4]) {
  const SavedLayout L = saved_layout(d);
  const DyLayout Y = dy_layout(d);
  const int E = d.E, FF = d.FF;
  auto in = [](const void* base, const Field& f) { return base ? (const void*)f.at(base) : nullptr; };
  it[0] = TimWgradItem{in(dy, Y.df), in(saved, L.h), g ? g->l2_w : nullptr, g ? g->l2_b : nullptr, E, FF, E, FF};
  it[1] = TimWgradItem{in(dy, Y.du), in(saved, L.x1t), g ? g->l1_w : nullptr, g ? g->l1_b : nullptr, FF, E, FF, E};
  it[2] = TimWgradItem{in(dy, Y.da), in(saved, L.o), g ? g->out_w : nullptr, g ? g->out_b : nullptr, E, E, E, E};
  it[3] = TimWgradItem{in(dy, Y.dqkv), x_in_T, g ? g->in_w : nullptr, g ? g->in_b : nullptr, 3 * E, E, 3 * E, E};
}

int splitk_for(int Mout, int Nout, int Kp) {
  const int tiles = ((Mout + 127) / 128) * ((Nout + 127) / 128);
  int sk = (512 + tiles - 1) / tiles;
  const int maxk = Kp / 256 > 0 ? Kp / 256 : 1;
  if (sk > maxk) sk = maxk;
  if (sk > 8) sk = 8;
  if (sk < 1) sk = 1;
  return sk;
}

struct WgradWs { Field tA, tB, slab; size_t total; };
WgradWs wgrad_ws(int prec, int Nout, int Kout, int M) {
  const size_t Mp = round_up(M, 64), ts = opsize(prec);
  Arena a;
  WgradWs w{};
  if (h16_storage(prec)) {  // transposing-read kernel: no operand copies
    w.total = tim_wgrad_tn_ws(Nout, Kout, M);
    return w;
  }
  w.tA = a.take((size_t)Nout * Mp * ts);
  w.tB = a.take((size_t)Kout * Mp * ts);
  const int sk = splitk_for(Nout, Kout, (int)Mp);
  w.slab = a.take(sk > 1 ? (size_t)sk * Nout * Kout * 4 : 0);
  w.total = a.total();
  return w;
}

// workspace of the data chain; `wg`: the part the weight gradients run in (timhip_layer_bwd hands it on)
struct WsLayout {
  Field f32a, f32b, Tb, Tc, wg, attn, lnp;
  size_t total;
};

WsLayout ws_layout(const TimDesc& d) {
  const size_t M = (size_t)d.B * d.S, ts = opsize(d.precision);
  // the weight gradients: one product at a time (timhip_wgrad) or the grouped launch (slabs only when it splits)
  TimWgradItem it[4];
  layer_products(d, nullptr, nullptr, nullptr, nullptr, it);
  size_t wg = h16_storage(d.precision) ? tim_wgrad_group_ws(it, 4, (int)M) : 0;
  for (int i = 0; i < 4; ++i) {
    // (the out-projection is left out, as it always was: the sizes the library reports stay what they were.  Run alone - the
    //  TIMHIP_DESC_WGRAD_SEPARATE route - it asks for more than the other three at a few shapes, E = 768 / FF = 3072 among them)
    if (i == 2) continue;
    const size_t one = wgrad_ws(d.precision, it[i].Nout, it[i].Kout, (int)M).total;
    if (one > wg) wg = one;
  }
  Arena a;
  WsLayout L;
  L.f32a = a.take(M * d.E * 4);
  L.f32b = a.take(M * d.E * 4);
  L.Tb = a.take(M * d.E * ts);
  L.Tc = a.take(M * d.E * ts);
  L.wg = a.take(wg);
  L.attn = a.take(tim_attention_bwd_ws(d));
  L.lnp = a.take(tim_layernorm_bwd_ws((int)M, d.E));
  L.total = a.total();
  return L;
}

int check_layer_desc(const TimDesc& d) {
  if (d.B <= 0 || d.S <= 0 || d.F <= 0 || d.F > d.S || d.E <= 0 || d.H <= 0 || d.FF <= 0) return TIMHIP_EINVAL;
  if (d.E % 64 || d.FF % 64 || d.E % d.H) return TIMHIP_EUNSUPPORTED;
  if (!valid_precision(d.precision)) return TIMHIP_EUNSUPPORTED;
  if (d.p_drop < 0.f || d.p_drop >= 1.f) return TIMHIP_EINVAL;
  return TIMHIP_OK;
}

TimEpi epi0() {
  TimEpi e;
  e.out0 = e.out1 = nullptr; e.bias = e.res = nullptr; e.aux = nullptr;
  e.ld0 = e.ld1 = e.ldres = e.ldaux = 0; e.p_drop = 0.f; e.site = 0; e.seed = 0;
  e.mask = nullptr; e.ldmask = 0; e.reserved = 0; e.a_wrap_k = 0; e.reserved2 = 0;
  e.ln_stats = e.ln_w = e.ln_b = nullptr;
  e.acc_scale = nullptr;
  return e;
}

// dW[Nout, Kout] += dY[M, Nout]^T X[M, Kout]   (+ db[Nout] += colsum dY)
// 16-bit operands: the transposing-read kernel of wgrad.hip (tim_wgrad_tn_h16), which also knows "=" instead of "+="
// (accumulate = 0) and a device scalar multiplied into what it writes (out_scale).
// fp32 / bf16x3 operands: both are transposed into K(=M)-contiguous copies, the product runs split-K into fp32
// slabs (plain coalesced stores, no atomics) and one reduce kernel adds the slabs into dW.
int wgrad(int prec, const void* dY, int ldy, int Nout, const void* X, int ldx, int Kout, int M, float* dW, float* db,
          void* ws, size_t ws_bytes, hipStream_t s, int accumulate = 1, const float* out_scale = nullptr) {
  const int Mp = round_up(M, 64);
  const WgradWs W = wgrad_ws(prec, Nout, Kout, M);
  if (ws_bytes < W.total) return TIMHIP_EWORKSPACE;
  if (h16_storage(prec)) return tim_wgrad_tn_h16(prec, dY, ldy, Nout, X, ldx, Kout, M, dW, db, ws, ws_bytes, s, accumulate, out_scale);
  if (!accumulate || out_scale) return TIMHIP_EUNSUPPORTED;   // the fp32 / bf16x3 route accumulates into dW, unscaled
  char* w = (char*)ws;
  void* tA = W.tA.at(w); void* tB = W.tB.at(w); float* slab = (float*)W.slab.at(w);
  int rc;
  if ((rc = tim_transpose(prec, dY, M, Nout, ldy, tA, Mp, db, s))) return rc;
  if ((rc = tim_transpose(prec, X, M, Kout, ldx, tB, Mp, nullptr, s))) return rc;
  const int sk = splitk_for(Nout, Kout, Mp);
  TimEpi e = epi0();
  if (sk == 1 || (Kout % 4) != 0) {
    e.out0 = dW; e.ld0 = Kout;
    return tim_gemm_nt(prec, TIMHIP_EPI_ATOMIC_F32, tA, Mp, tB, Mp, Nout, Kout, Mp, e, sk, s);
  }
  e.out0 = slab; e.ld0 = Kout;
  if ((rc = tim_gemm_nt(prec, TIMHIP_EPI_STORE_F32, tA, Mp, tB, Mp, Nout, Kout, Mp, e, sk, s))) return rc;
  return tim_slab_reduce(slab, (long long)Nout * Kout, sk, dW, s);
}

// What a pass over a layer takes from the descriptor's flags rather than from its shape.
struct LayerPass {
  // fp16: the gradient OPERANDS (df, du, da, Tb, Tc, dqkv, the 16-bit parts of the stream and the attention scratch) carry the
  // factor S = grad_scale[0]; it enters with the T copies LayerNorm-backward writes (gs_in) and leaves where a product joins
  // fp32 values (gs_out = &grad_scale[1], 1 / S).  NULL both: no scale
  const float* gs_in;
  const float* gs_out;
  int accumulate;   // weight gradients: 1 "+=", 0 "=" (TIMHIP_DESC_WGRAD_OVERWRITE: the buffers are neither zero-filled nor read)
  const unsigned long long* akeep;   // the attention dropout's keep-bits (TIMHIP_DESC_ATTN_KEEP_BITS), NULL: the kernels draw their own
};
LayerPass layer_pass(const TimDesc& d, const unsigned long long* keep_bits = nullptr) {   // keep_bits: where the saved block has them
  LayerPass P;
  P.gs_in = (d.precision == TIMHIP_PREC_F16 && d.grad_scale) ? d.grad_scale : nullptr;
  P.gs_out = P.gs_in ? P.gs_in + 1 : nullptr;
  P.accumulate = (d.reserved & TIMHIP_DESC_WGRAD_OVERWRITE) ? 0 : 1;
  P.akeep = ((d.reserved & TIMHIP_DESC_ATTN_KEEP_BITS) && d.p_drop > 0.f) ? keep_bits : nullptr;
  return P;
}

// whether the grouped weight-gradient launches take this layer (else: one timhip_wgrad per product).  Their other condition, four
// products of a multiple of 4 elements each, holds for every descriptor check_layer_desc lets through (E % 64 == 0)
bool wgrad_grouped(const TimDesc& d) { return h16_storage(d.precision) && !(d.reserved & TIMHIP_DESC_WGRAD_SEPARATE); }

// One forward Linear: epilogue `epi` of A[M, K] W[N, K]^T.  split: W is a split copy [hi | lo | ..] with row stride 3 K (the
// descriptor's *_SPLIT flags); the product runs over 2 K with the activation operand read twice (TimEpi.a_wrap_k) - the weight
// to ~22 bits
int linear_fwd(int prec, int epi, const void* A, const void* W, int M, int N, int K, bool split, TimEpi e, hipStream_t s) {
  if (!split) return tim_gemm_nt(prec, epi, A, K, W, K, M, N, K, e, 1, s);
  e.a_wrap_k = K; e.reserved = 2;
  return tim_gemm_nt(prec, epi, A, K, W, 3 * K, M, N, 2 * K, e, 1, s);
}

}  // namespace

const unsigned long long* tim_salt_ptr = nullptr;

// ---- environment knobs, cached (common.h: TimKnobs) ----------------------------------------------------------------
namespace {
TimKnobs g_knobs;
std::atomic<int> g_knobs_state{0};   // 0: not read, 1: valid
int env_int(const char* name, int dflt) { const char* v = getenv(name); return (v && v[0]) ? atoi(v) : dflt; }
void read_knobs(TimKnobs& k) {
  k.gemm_pp = env_int("TIMHIP_GEMM_PP", k.gemm_pp); k.gemm_ld = env_int("TIMHIP_GEMM_LD", k.gemm_ld); k.gemm_pf = env_int("TIMHIP_GEMM_PF", k.gemm_pf);
  k.gemm_pf_mode = env_int("TIMHIP_GEMM_PF_MODE", k.gemm_pf_mode); k.gemm_pf_mr = env_int("TIMHIP_GEMM_PF_MR", k.gemm_pf_mr);
  k.gemm_ldp = env_int("TIMHIP_GEMM_LDP", k.gemm_ldp); k.gemm_ld1 = env_int("TIMHIP_GEMM_LD1", k.gemm_ld1); k.gemm_pt = env_int("TIMHIP_GEMM_PT", k.gemm_pt);
  k.gemm_dg = env_int("TIMHIP_GEMM_DG", k.gemm_dg); k.gemm_dg_offset = env_int("TIMHIP_GEMM_DG_OFFSET", k.gemm_dg_offset);
  k.fuse_ln = env_int("TIMHIP_FUSE_LN", k.fuse_ln); k.fuse_ln_spin = env_int("TIMHIP_FUSE_LN_SPIN", k.fuse_ln_spin);
  k.wgrad_pp = env_int("TIMHIP_WGRAD_PP", k.wgrad_pp); k.wgrad_ld = env_int("TIMHIP_WGRAD_LD", k.wgrad_ld); k.wgrad_pf = env_int("TIMHIP_WGRAD_PF", k.wgrad_pf);
  k.wgrad_p8 = env_int("TIMHIP_WGRAD_P8", k.wgrad_p8); k.wgrad_p8_ph = env_int("TIMHIP_WGRAD_P8_PH", k.wgrad_p8_ph);
  k.attn_waves = env_int("TIMHIP_ATTN_WAVES", k.attn_waves); k.attn_fused = env_int("TIMHIP_ATTN_FUSED", k.attn_fused);
  k.ln_rpb = env_int("TIMHIP_LN_RPB", k.ln_rpb);
  k.gemm_tmw = env_int("TIMHIP_GEMM_TMW", k.gemm_tmw);
  k.ln_rpb_small = env_int("TIMHIP_LN_RPB_SMALL", k.ln_rpb_small); k.ln_fwd_rpb = env_int("TIMHIP_LN_FWD_RPB", k.ln_fwd_rpb);
  k.gemm_small_nst = env_int("TIMHIP_GEMM_SMALL_NST", k.gemm_small_nst); k.gemm_small_w8 = env_int("TIMHIP_GEMM_SMALL_W8", k.gemm_small_w8); k.gemm_p8_ph = env_int("TIMHIP_GEMM_P8_PH", k.gemm_p8_ph);
  k.gemm_pp_min = env_int("TIMHIP_GEMM_PP_MIN_TILES", k.gemm_pp_min);
  k.attn_ks = env_int("TIMHIP_ATTN_KS", k.attn_ks);
  k.attn_bwd_co = env_int("TIMHIP_ATTN_BWD_CO", k.attn_bwd_co);
  k.gemm_p8 = env_int("TIMHIP_GEMM_P8", k.gemm_p8);
  k.ln_pair = env_int("TIMHIP_LN_PAIR", k.ln_pair);
  k.epi_pair = env_int("TIMHIP_EPI_PAIR", k.epi_pair);
  k.epi_g2_pk = env_int("TIMHIP_EPI_G2_PK", k.epi_g2_pk);
  k.epi_wt = env_int("TIMHIP_EPI_WT", k.epi_wt);
  k.attn_split_min = env_int("TIMHIP_ATTN_SPLIT_MIN", k.attn_split_min);
  if (k.attn_split_min < 1) k.attn_split_min = 1;
}
}  // namespace
const TimKnobs& tim_knobs() {
  if (g_knobs_state.load(std::memory_order_acquire) == 0) {   // (a benign race reads the same environment twice)
    TimKnobs k;
    read_knobs(k);
    g_knobs = k;
    g_knobs_state.store(1, std::memory_order_release);
  }
  return g_knobs;
}

extern "C" {

int timhip_version(void) { return TIMHIP_VERSION; }
void timhip_reload_env(void) { g_knobs_state.store(0, std::memory_order_release); (void)tim_knobs(); }
int timhip_gemm_p8_choice(int epi, int M, int N, int K) { return gemm_p8_tm(tim_knobs(), epi, M, N, K, 0); }
int timhip_build_flags(void) {
#ifdef TIMHIP_TUNING
  return 1;
#else
  return 0;
#endif
}

int timhip_dropout_salt(const unsigned long long* dev_salt) {
  tim_salt_ptr = dev_salt;
  return TIMHIP_OK;
}

const char* timhip_strerror(int code) {
  switch (code) {
    case TIMHIP_OK: return "ok";
    case TIMHIP_EINVAL: return "invalid argument (null pointer or bad descriptor field)";
    case TIMHIP_EUNSUPPORTED: return "shape or precision not supported by the gfx950 kernels";
    case TIMHIP_EWORKSPACE: return "workspace too small";
    case TIMHIP_ELAUNCH: return "HIP kernel launch failed";
    case TIMHIP_EALIGN: return "pointer or leading dimension not aligned";
    default: return "unknown timhip error";
  }
}

int timhip_attn_keep_bits(const TimDesc* d, int nlayers, void* const* saved, void* stream) {
  if (!d || !saved || nlayers <= 0) return TIMHIP_EINVAL;
  // (the geometry whose kernels read them: 128-wide heads, 97 .. 128 feature keys - attn_fwd_mfma<.., 128, 4, true> and the fused
  //  key-split backward; every other shape draws its masks in the kernels)
  if (!h16_storage(d->precision) || !(d->p_drop > 0.f) || d->B <= 0 || d->S <= 0 || d->H <= 0 || d->E / d->H != 128 ||
      (d->F + 31) / 32 != 4)
    return TIMHIP_EUNSUPPORTED;
  const SavedLayout L = saved_layout(*d);
  for (int l0 = 0; l0 < nlayers; l0 += 8) {
    unsigned long long* out[8] = {};
    const int n = nlayers - l0 < 8 ? nlayers - l0 : 8;
    for (int i = 0; i < n; ++i) {
      if (!saved[l0 + i]) return TIMHIP_EINVAL;
      out[i] = reinterpret_cast<unsigned long long*>(L.attn_keep.at(saved[l0 + i]));
    }
    const int rc = tim_attn_keep_bits(*d, l0, n, out, (hipStream_t)stream);
    if (rc) return rc;
  }
  return TIMHIP_OK;
}

size_t timhip_layer_saved_bytes(const TimDesc* d) { return d ? saved_layout(*d).total : 0; }

// test hook: where a field of the (otherwise opaque) saved block lives
int timhip_layer_saved_field(const TimDesc* d, int field, size_t* offset, size_t* bytes) {
  if (!d || !offset || !bytes) return TIMHIP_EINVAL;
  const SavedLayout L = saved_layout(*d);
  const Field* f;
  switch (field) {
    case TIMHIP_SAVED_QKV: f = &L.qkv; break;
    case TIMHIP_SAVED_O: f = &L.o; break;
    case TIMHIP_SAVED_Y1: f = &L.y1; break;
    case TIMHIP_SAVED_X1T: f = &L.x1t; break;
    case TIMHIP_SAVED_H: f = &L.h; break;
    case TIMHIP_SAVED_Y2: f = &L.y2; break;
    case TIMHIP_SAVED_FFN_KEEP_BITS: f = &L.ffn_mask; break;
    case TIMHIP_SAVED_ATTN_KEEP_BITS: f = &L.attn_keep; break;
    default: return TIMHIP_EINVAL;
  }
  *offset = f->off; *bytes = f->bytes;
  return TIMHIP_OK;
}

int timhip_gemm_nt(int precision, int epi, const void* A, int lda, const void* B, int ldb, int M, int N, int K,
                   const TimEpi* e, int splitk, void* stream) {
  if (!e) return TIMHIP_EINVAL;
  return tim_gemm_nt(precision, epi, A, lda, B, ldb, M, N, K, *e, splitk, (hipStream_t)stream);
}

size_t timhip_wgrad_workspace_bytes(int precision, int Nout, int Kout, int M) {
  return wgrad_ws(precision, Nout, Kout, M).total;
}

int timhip_gemm_nt_group(int precision, int epi, const TimGemmItem* items, int n, void* stream) {
  return tim_gemm_nt_group(precision, epi, items, n, (hipStream_t)stream);
}

size_t timhip_wgrad_group_workspace_bytes(int precision, const TimWgradItem* items, int n, int M) {
  return (h16_storage(precision) && items && n > 0) ? tim_wgrad_group_ws(items, n, M) : 0;
}

int timhip_wgrad_group(int precision, const TimWgradItem* items, int n, int M, int accumulate, void* workspace,
                       size_t workspace_bytes, const float* out_scale, void* stream) {
  return tim_wgrad_group_h16(precision, items, n, M, accumulate, workspace, workspace_bytes, out_scale, (hipStream_t)stream);
}

int timhip_wgrad(int precision, const void* dY, int ldy, int Nout, const void* X, int ldx, int Kout, int M,
                 float* dW, float* db, void* workspace, size_t workspace_bytes, const float* out_scale, void* stream) {
  if (!dY || !X || !dW || !workspace) return TIMHIP_EINVAL;
  return wgrad(precision, dY, ldy, Nout, X, ldx, Kout, M, dW, db, workspace, workspace_bytes, (hipStream_t)stream, 1, out_scale);
}

// The fp32 residual stream is only ever READ by the "+ residual" epilogues, and each of them can normalise on the fly
// (TimEpi.ln_*): a layer's input rows are LayerNorm-2 of the previous layer's y2, its inner residual LayerNorm-1 of its own
// y1.  So the normalised fp32 rows are written only where someone else needs them (x_out of the last layer -> feats);
// LayerNorm writes its bf16 operand copy and the statistics, 60 instead of 100 MB per launch.
// One layer body for training and evaluation, parameterised by WHERE the intermediates live and WHICH stores exist:
//   u == NULL      linear1 writes h only (TIMHIP_EPI_GELU_T) - nobody multiplies with gelu' in an evaluation forward
//   lse == NULL    attention skips its log-sum-exp store
//   s0 > 0         "tail": everything behind the in-projection runs on the token rows s0 .. S - 1 of every window only, compactly
//                  (B (S - s0) rows: o, y1, x1t, h, y2, the outputs - and the residual rows the caller hands in)
//   kv != NULL     every row is a query row of one of d.B groups: its keys and values are the K | V rows of window widx[g] of a
//                  cache (timhip_stack_query; tim_attention_query_fwd) plus its own.  d.F: the cached keys per window (may exceed d.S)
struct LayerBufs {
  void* qkv; void* o; float* lse; float* y1; float* st1; void* x1t; void* u; void* h; float* y2; float* st2;
  uint8_t* ffn_mask; const unsigned long long* attn_keep;
  const void* kv; int ldkv, wrows, W; const int* widx;
};

static LayerBufs saved_bufs(const TimDesc& d, void* saved) {
  const SavedLayout L = saved_layout(d);
  return LayerBufs{L.qkv.at(saved), L.o.at(saved), (float*)L.lse.at(saved), (float*)L.y1.at(saved), (float*)L.st1.at(saved),
                   L.x1t.at(saved), L.u.at(saved), L.h.at(saved), (float*)L.y2.at(saved), (float*)L.st2.at(saved),
                   (uint8_t*)L.ffn_mask.at(saved), reinterpret_cast<const unsigned long long*>(L.attn_keep.at(saved)),
                   nullptr, 0, 0, 0, nullptr};
}

static int layer_fwd_body(const TimDesc& d, const TimLayerParams* w, const float* x_in, const float* x_in_prenorm,
                          const float* x_in_stats, const float* x_in_lnw, const float* x_in_lnb, const void* x_in_T,
                          float* x_out, void* x_out_T, const LayerBufs& bufs, int s0, hipStream_t s) {
  int rc;
  const int Mall = d.B * d.S, M = d.B * (d.S - s0), E = d.E, FF = d.FF, prec = d.precision;
  void* qkv = bufs.qkv; void* o = bufs.o; float* y1 = bufs.y1; float* st1 = bufs.st1; void* x1t = bufs.x1t;
  void* u = bufs.u; void* h = bufs.h; float* y2 = bufs.y2; float* st2 = bufs.st2;

  // 1. packed in-projection (F._in_projection_packed)
  // (a *_SPLIT flag: that weight pointer is a split copy, see linear_fwd)
  auto split = [&](int flag) { return (d.reserved & flag) != 0 && h16_storage(prec); };
  TimEpi e = epi0();
  e.out0 = qkv; e.ld0 = 3 * E; e.bias = w->in_b;
  if ((rc = linear_fwd(prec, TIMHIP_EPI_STORE_T, x_in_T, w->in_w, Mall, 3 * E, E, split(TIMHIP_DESC_INPROJ_SPLIT), e, s))) return rc;
  // 2. structured attention (keys and values of all rows; the rows from s0 on)
  if (bufs.kv) {
    if ((rc = tim_attention_query_fwd(d, qkv, bufs.kv, bufs.ldkv, bufs.wrows, bufs.W, bufs.widx, o, s))) return rc;
  } else if ((rc = tim_attention_fwd(d, qkv, o, bufs.lse, s, layer_pass(d, bufs.attn_keep).akeep, s0))) return rc;
  // 3. out-projection + dropout1 + residual
  e = epi0();
  e.out0 = y1; e.ld0 = E; e.bias = w->out_b; e.ldres = E;
  if (x_in) {
    e.res = x_in;
  } else {   // the input rows as LayerNorm-2 of the previous layer's y2
    e.res = x_in_prenorm; e.ln_stats = x_in_stats; e.ln_w = x_in_lnw; e.ln_b = x_in_lnb;
  }
  e.p_drop = d.p_drop; e.seed = d.seed; e.site = layer_site(d.layer, SITE_L_DROP1);
  uint8_t* fmask = d.p_drop > 0.f ? bufs.ffn_mask : nullptr;
  // TIMHIP_FUSE_LN=1 (round 3, opt-in): the LayerNorm that follows the out-projection / linear2 inside the GEMM's epilogue
  // (gemm_nt_ldln_kernel: the column tiles of a row panel exchange row statistics); the stand-alone LayerNorm stays behind it as
  // a launch that exits at once unless a tile's wait timed out.  Falls back to the two kernels wherever the shape does not fit.
  const bool fuse_ln = tim_knobs().fuse_ln == 1;
  const uint32_t* ln_run_if = nullptr;
  bool fused1 = false;
  if (fuse_ln && h16_storage(prec) && !split(TIMHIP_DESC_OUTPROJ_SPLIT)) {
    TimLnFuse lf{x1t, E, nullptr, 0, st1, w->n1_w, w->n1_b, fmask, FF, d.p_drop, d.seed, layer_site(d.layer, SITE_L_FFN)};
    rc = tim_gemm_nt_fuse_ln(prec, o, E, w->out_w, E, M, E, E, e, lf, &ln_run_if, s);
    if (rc == TIMHIP_OK) fused1 = true;
    else if (rc != TIMHIP_EUNSUPPORTED) return rc;
  }
  if (!fused1 && (rc = linear_fwd(prec, TIMHIP_EPI_DROP_RES_F32, o, w->out_w, M, E, E, split(TIMHIP_DESC_OUTPROJ_SPLIT), e, s))) return rc;
  // 4. norm1.  The kernel is HBM-bound with idle VALU: it also draws the keep-bits of the FFN dropout (same Philox
  //    stream as the epilogues would use), which the linear1 epilogue and, in the backward, the gelu' epilogue read
  if ((rc = tim_layernorm_fwd(prec, y1, M, E, E, 0, w->n1_w, w->n1_b, nullptr, 0, x1t, E, st1, s, fmask, FF, d.p_drop, d.seed,
                              layer_site(d.layer, SITE_L_FFN), fused1 ? ln_run_if : nullptr))) return rc;
  // 5. linear1 + GELU(erf) + dropout
  e = epi0();
  e.out0 = h; e.ld0 = FF; e.bias = w->l1_b;
  // (out1 = `u` holds dropmask * gelu'(linear1 output): the factor the backward multiplies with - it never needs the
  //  pre-activations themselves, so its epilogue is a plain multiply; no `u`: no backward, h alone)
  const int epi1 = u ? TIMHIP_EPI_GELU_DROP_G2 : TIMHIP_EPI_GELU_T;
  if (u) {
    e.out1 = u; e.ld1 = FF;
    e.p_drop = d.p_drop; e.seed = d.seed; e.site = layer_site(d.layer, SITE_L_FFN);
    e.mask = fmask; e.ldmask = FF / 8;
  }
  if ((rc = linear_fwd(prec, epi1, x1t, w->l1_w, M, FF, E, split(TIMHIP_DESC_L1_SPLIT), e, s))) return rc;
  // 6. linear2 + dropout2 + residual
  e = epi0();
  e.out0 = y2; e.ld0 = E; e.bias = w->l2_b; e.ldres = E;
  e.res = y1; e.ln_stats = st1; e.ln_w = w->n1_w; e.ln_b = w->n1_b;   // residual = norm1(y1), normalised by the epilogue
  e.p_drop = d.p_drop; e.seed = d.seed; e.site = layer_site(d.layer, SITE_L_DROP2);
  bool fused2 = false;
  if (fuse_ln && h16_storage(prec) && !split(TIMHIP_DESC_L2_SPLIT)) {
    TimLnFuse lf{x_out_T, E, x_out, E, st2, w->n2_w, w->n2_b, nullptr, 0, 0.f, 0, 0};
    rc = tim_gemm_nt_fuse_ln(prec, h, FF, w->l2_w, FF, M, E, FF, e, lf, &ln_run_if, s);
    if (rc == TIMHIP_OK) fused2 = true;
    else if (rc != TIMHIP_EUNSUPPORTED) return rc;
  }
  if (!fused2 && (rc = linear_fwd(prec, TIMHIP_EPI_DROP_RES_F32, h, w->l2_w, M, E, FF, split(TIMHIP_DESC_L2_SPLIT), e, s))) return rc;
  // 7. norm2 (x_out == NULL: only the operand copy and the statistics)
  return tim_layernorm_fwd(prec, y2, M, E, E, 0, w->n2_w, w->n2_b, x_out, E, x_out_T, E, st2, s, nullptr, 0, 0.f, 0, 0,
                           fused2 ? ln_run_if : nullptr);
}

int timhip_layer_fwd(const TimDesc* dp, const TimLayerParams* w, const float* x_in, const void* x_in_T, float* x_out,
                     void* x_out_T, void* saved, void* workspace, size_t workspace_bytes, void* stream) {
  (void)workspace; (void)workspace_bytes;   // kept in the signature: earlier versions staged norm1's fp32 rows there
  if (!dp || !w || !x_in || !x_in_T || !x_out_T || !saved) return TIMHIP_EINVAL;
  int rc = check_layer_desc(*dp);
  if (rc) return rc;
  return layer_fwd_body(*dp, w, x_in, nullptr, nullptr, nullptr, nullptr, x_in_T, x_out, x_out_T, saved_bufs(*dp, saved), 0,
                        (hipStream_t)stream);
}

int timhip_layer_fwd_chained(const TimDesc* dp, const TimLayerParams* w, const TimLayerParams* prev_w, const void* prev_saved,
                             const void* x_in_T, float* x_out, void* x_out_T, void* saved, void* stream) {
  if (!dp || !w || !prev_w || !prev_saved || !x_in_T || !x_out_T || !saved) return TIMHIP_EINVAL;
  int rc = check_layer_desc(*dp);
  if (rc) return rc;
  const SavedLayout L = saved_layout(*dp);   // the previous layer has the same shape
  return layer_fwd_body(*dp, w, nullptr, (const float*)L.y2.at(prev_saved), (const float*)L.st2.at(prev_saved), prev_w->n2_w,
                        prev_w->n2_b, x_in_T, x_out, x_out_T, saved_bufs(*dp, saved), 0, (hipStream_t)stream);
}

// ---- evaluation forward of the whole stack out of one arena (timhip_stack_infer) ---------------------------------------------
// The arena holds ONE layer's intermediates - the fields of a saved block a forward itself reads (no lse, no u, no keep-bits) -
// plus the operand-dtype rows between two layers and, for the query-row tail, the gathered residual rows.  One copy is enough:
// a layer reads the previous layer's y2 / st2 (its residual, normalised by the out-projection epilogue) before its own linear2
// rewrites them, and the previous layer's operand rows (its in-projection) before its own norm2 rewrites those.
struct InferLayout { Field qkv, o, y1, st1, x1t, h, y2, st2, xt, resg, stg; size_t total; };
static InferLayout infer_layout(const TimDesc& d, int tail_only) {
  const size_t M = (size_t)d.B * d.S, Mt = (size_t)d.B * (d.S - d.F), ts = opsize(d.precision);
  Arena a;
  InferLayout L;
  L.qkv = a.take(M * 3 * d.E * ts);
  L.o = a.take(M * d.E * ts);
  L.y1 = a.take(M * d.E * 4);
  L.st1 = a.take(M * 2 * 4);
  L.x1t = a.take(M * d.E * ts);
  L.h = a.take(M * d.FF * ts);
  L.y2 = a.take(M * d.E * 4);
  L.st2 = a.take(M * 2 * 4);
  L.xt = a.take(M * d.E * ts);
  L.resg = a.take(tail_only ? Mt * d.E * 4 : 0);   // fp32 residual rows of the tail's query rows (pre-norm, or x_in's own)
  L.stg = a.take(tail_only ? Mt * 2 * 4 : 0);      // their LayerNorm statistics
  L.total = a.total();
  return L;
}

size_t timhip_stack_infer_workspace_bytes(const TimDesc* d, int nlayers, int tail_only) {
  (void)nlayers;   // (in the signature for the caller's sake: the arena is one layer's, whatever the depth)
  return (d && check_layer_desc(*d) == TIMHIP_OK) ? infer_layout(*d, tail_only).total : 0;
}

// The one body of timhip_stack_infer and timhip_stack_infer_maps.  maps (HOST array of nlayers device pointers, or NULL): behind
// layer l's launches - its qkv is live in the arena until layer l + 1's in-projection - the weights kernel writes maps[l].
static int stack_infer_body(const TimDesc* dp, int nlayers, const TimLayerParams* layers, const float* x_in, const void* x_in_T,
                            float* x_out, void* x_out_T, int tail_only, float* const* maps, int maps_s0, int ld,
                            void* workspace, size_t workspace_bytes, void* stream, void* kv_cache = nullptr) {
  if (!dp || !layers || nlayers <= 0 || !x_in || !x_in_T || (!x_out_T && !kv_cache) || !workspace) return TIMHIP_EINVAL;
  TimDesc d = *dp;
  int rc = check_layer_desc(d);
  if (rc) return rc;
  if (d.p_drop != 0.f || (tail_only && d.S == d.F)) return TIMHIP_EINVAL;
  if (maps) {   // refused before the first launch, like everything above
    if (maps_s0 < 0 || maps_s0 >= d.S || ld < d.F + 1) return TIMHIP_EINVAL;
    if (d.F > 192) return TIMHIP_EUNSUPPORTED;
    for (int l = 0; l < nlayers; ++l)
      if (((uintptr_t)maps[l] & 3) != 0) return TIMHIP_EALIGN;
  }
  const InferLayout L = infer_layout(d, tail_only);
  if (workspace_bytes < L.total) return TIMHIP_EWORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  void* ws = workspace;
  const LayerBufs bufs{L.qkv.at(ws), L.o.at(ws), nullptr, (float*)L.y1.at(ws), (float*)L.st1.at(ws), L.x1t.at(ws), nullptr,
                       L.h.at(ws), (float*)L.y2.at(ws), (float*)L.st2.at(ws), nullptr, nullptr, nullptr, 0, 0, 0, nullptr};
  d.reserved &= ~TIMHIP_DESC_ATTN_KEEP_BITS;
  for (int l = 0; l < nlayers; ++l) {
    const bool last = l == nlayers - 1;
    const int s0 = (last && tail_only) ? d.F : 0;
    d.layer = l;
    // the residual of the out-projection: the caller's fp32 rows (first layer), LayerNorm-2 of the previous layer's y2 otherwise
    const float* res = l == 0 ? x_in : nullptr;
    const float* pre = l == 0 ? nullptr : bufs.y2;
    const float* pst = l == 0 ? nullptr : bufs.st2;
    if (s0) {   // the tail reads them by compact row index: gather the query rows (fp32; pre-norm rows with their statistics)
      float* resg = (float*)L.resg.at(ws); float* stg = (float*)L.stg.at(ws);
      if ((rc = timhip_gather_rows(TIMHIP_PREC_FP32, l == 0 ? x_in : pre, d.B, d.S, d.E, s0, d.S - s0, resg, stream))) return rc;
      if (l > 0 && (rc = timhip_gather_rows(TIMHIP_PREC_FP32, pst, d.B, d.S, 2, s0, d.S - s0, stg, stream))) return rc;
      if (l == 0) res = resg; else { pre = resg; pst = stg; }
    }
    const void* in_T = l == 0 ? x_in_T : (const void*)L.xt.at(ws);
    if ((rc = layer_fwd_body(d, &layers[l], res, pre, pst, l ? layers[l - 1].n2_w : nullptr, l ? layers[l - 1].n2_b : nullptr, in_T,
                             last ? x_out : nullptr, (last && x_out_T) ? x_out_T : (void*)L.xt.at(ws), bufs, s0, s))) return rc;
    if (maps && maps[l] && (rc = tim_attention_weights(d, bufs.qkv, maps_s0, 0, maps[l], ld, s))) return rc;
    // kv_cache (timhip_stack_encode: S == F, every row a feature row): the K | V columns of the layer's qkv - live in the arena until
    // the next in-projection - as rows of 2 E elements into block l of the cache; one pitched device copy, 2/3 of qkv read and written
    if (kv_cache) {
      const size_t ts = opsize(d.precision), rowb = (size_t)2 * d.E * ts, rows = (size_t)d.B * d.S;
      if (hipMemcpy2DAsync((char*)kv_cache + (size_t)l * rows * rowb, rowb, (const char*)bufs.qkv + (size_t)d.E * ts, (size_t)3 * d.E * ts,
                           rowb, rows, hipMemcpyDeviceToDevice, s) != hipSuccess) return TIMHIP_ELAUNCH;
    }
  }
  return TIMHIP_OK;
}

int timhip_stack_infer(const TimDesc* dp, int nlayers, const TimLayerParams* layers, const float* x_in, const void* x_in_T,
                       float* x_out, void* x_out_T, int tail_only, void* workspace, size_t workspace_bytes, void* stream) {
  return stack_infer_body(dp, nlayers, layers, x_in, x_in_T, x_out, x_out_T, tail_only, nullptr, 0, 0, workspace, workspace_bytes,
                          stream);
}

// (the maps are the caller's buffers: the arena is timhip_stack_infer's)
size_t timhip_stack_infer_maps_workspace_bytes(const TimDesc* d, int nlayers, int tail_only) {
  return timhip_stack_infer_workspace_bytes(d, nlayers, tail_only);
}

int timhip_stack_infer_maps(const TimDesc* dp, int nlayers, const TimLayerParams* layers, const float* x_in, const void* x_in_T,
                            float* x_out, void* x_out_T, int tail_only, float* const* maps, int maps_s0, int ld,
                            void* workspace, size_t workspace_bytes, void* stream) {
  if (!maps) return TIMHIP_EINVAL;
  return stack_infer_body(dp, nlayers, layers, x_in, x_in_T, x_out, x_out_T, tail_only, maps, maps_s0, ld, workspace,
                          workspace_bytes, stream);
}

// ---- encode a window once, query it many times (timhip_stack_encode / timhip_stack_query) -----------------------------------------
// The feature rows of a window never read a query row, and a query row reads the feature rows' keys and values and itself: the
// stack on the feature rows alone (S == F) is the feature stream of a full forward, and its per-layer K | V columns are all a later
// pass over query rows needs.  cache: [nlayers][W F][2 E] in the operand dtype.
size_t timhip_window_cache_bytes(const TimDesc* d, int nlayers) {
  if (!d || nlayers <= 0 || check_layer_desc(*d) != TIMHIP_OK || d->S != d->F) return 0;
  return (size_t)nlayers * d->B * d->F * 2 * d->E * opsize(d->precision);
}

int timhip_stack_encode(const TimDesc* dp, int nlayers, const TimLayerParams* layers, const float* x_in, const void* x_in_T,
                        float* feats_out, void* cache, void* workspace, size_t workspace_bytes, void* stream) {
  if (!dp || !cache || dp->S != dp->F) return TIMHIP_EINVAL;
  if (((uintptr_t)cache & 15) != 0) return TIMHIP_EALIGN;
  return stack_infer_body(dp, nlayers, layers, x_in, x_in_T, feats_out, nullptr, 0, nullptr, 0, 0, workspace, workspace_bytes, stream,
                          cache);
}

// a query descriptor: B = groups, S = query rows per group, F = cached keys per window (no relation to S)
static int check_query_desc(const TimDesc& d) {
  if (d.F <= 0) return TIMHIP_EINVAL;
  TimDesc c = d;
  c.F = 1;
  return check_layer_desc(c);
}

size_t timhip_stack_query_workspace_bytes(const TimDesc* d, int nlayers) {
  (void)nlayers;   // (one layer's arena, as timhip_stack_infer_workspace_bytes)
  return (d && check_query_desc(*d) == TIMHIP_OK) ? infer_layout(*d, 0).total : 0;
}

// The one body of timhip_stack_query and timhip_stack_query_maps.  maps (HOST array of nlayers device pointers, or NULL): behind
// layer l's launches - the in-projection of the query rows is live in the arena until layer l + 1's - the weights kernel writes
// maps[l] from those rows and the K columns of cache block l.
static int stack_query_body(const TimDesc* dp, int nlayers, const TimLayerParams* layers, const void* cache, int W, const int* widx,
                            const float* xq_in, const void* xq_in_T, float* xq_out, void* xq_out_T, float* const* maps,
                            int per_head, int ld, void* workspace, size_t workspace_bytes, void* stream) {
  if (!dp || !layers || nlayers <= 0 || !cache || !xq_in || !xq_in_T || !xq_out_T || !workspace) return TIMHIP_EINVAL;
  TimDesc d = *dp;
  int rc = check_query_desc(d);
  if (rc) return rc;
  if (d.p_drop != 0.f || W <= 0 || (!widx && d.B != W)) return TIMHIP_EINVAL;
  if (d.F > 192) return TIMHIP_EUNSUPPORTED;   // (the attention kernels' key limit; refused here, before the first launch)
  if (((uintptr_t)cache & 15) != 0) return TIMHIP_EALIGN;
  if (maps) {   // refused before the first launch, like everything above
    if (ld < d.F + 1) return TIMHIP_EINVAL;
    for (int l = 0; l < nlayers; ++l)
      if (((uintptr_t)maps[l] & 3) != 0) return TIMHIP_EALIGN;
  }
  const InferLayout L = infer_layout(d, 0);
  if (workspace_bytes < L.total) return TIMHIP_EWORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  void* ws = workspace;
  LayerBufs bufs{L.qkv.at(ws), L.o.at(ws), nullptr, (float*)L.y1.at(ws), (float*)L.st1.at(ws), L.x1t.at(ws), nullptr,
                 L.h.at(ws), (float*)L.y2.at(ws), (float*)L.st2.at(ws), nullptr, nullptr, nullptr, 2 * d.E, d.F, W, widx};
  d.reserved &= ~TIMHIP_DESC_ATTN_KEEP_BITS;
  const size_t layer_bytes = (size_t)W * d.F * 2 * d.E * opsize(d.precision);
  for (int l = 0; l < nlayers; ++l) {
    const bool last = l == nlayers - 1;
    d.layer = l;
    bufs.kv = (const char*)cache + (size_t)l * layer_bytes;
    if ((rc = layer_fwd_body(d, &layers[l], l == 0 ? xq_in : nullptr, l == 0 ? nullptr : bufs.y2, l == 0 ? nullptr : bufs.st2,
                             l ? layers[l - 1].n2_w : nullptr, l ? layers[l - 1].n2_b : nullptr,
                             l == 0 ? xq_in_T : (const void*)L.xt.at(ws), last ? xq_out : nullptr,
                             last ? xq_out_T : (void*)L.xt.at(ws), bufs, 0, s))) return rc;
    if (maps && maps[l] &&
        (rc = tim_attention_query_weights(d, bufs.qkv, bufs.kv, bufs.ldkv, bufs.wrows, W, widx, per_head, maps[l], ld, s))) return rc;
  }
  return TIMHIP_OK;
}

int timhip_stack_query(const TimDesc* dp, int nlayers, const TimLayerParams* layers, const void* cache, int W, const int* widx,
                       const float* xq_in, const void* xq_in_T, float* xq_out, void* xq_out_T, void* workspace,
                       size_t workspace_bytes, void* stream) {
  return stack_query_body(dp, nlayers, layers, cache, W, widx, xq_in, xq_in_T, xq_out, xq_out_T, nullptr, 0, 0, workspace,
                          workspace_bytes, stream);
}

// (the maps are the caller's buffers: the arena is timhip_stack_query's)
size_t timhip_stack_query_maps_workspace_bytes(const TimDesc* d, int nlayers) { return timhip_stack_query_workspace_bytes(d, nlayers); }

int timhip_stack_query_maps(const TimDesc* dp, int nlayers, const TimLayerParams* layers, const void* cache, int W, const int* widx,
                            const float* xq_in, const void* xq_in_T, float* xq_out, void* xq_out_T, float* const* maps,
                            int per_head, int ld, void* workspace, size_t workspace_bytes, void* stream) {
  if (!maps) return TIMHIP_EINVAL;
  return stack_query_body(dp, nlayers, layers, cache, W, widx, xq_in, xq_in_T, xq_out, xq_out_T, maps, per_head, ld, workspace,
                          workspace_bytes, stream);
}

size_t timhip_layer_ln_partial_bytes(const TimDesc* d) { return d ? 2 * tim_layernorm_bwd_ws(d->B * d->S, d->E) : 0; }
size_t timhip_layer_dy_bytes(const TimDesc* d) { return d ? dy_layout(*d).total : 0; }
size_t timhip_layer_workspace_bytes(const TimDesc* d) { return d ? ws_layout(*d).total + dy_layout(*d).total : 0; }
size_t timhip_layer_data_workspace_bytes(const TimDesc* d) { return d ? ws_layout(*d).total : 0; }
size_t timhip_layer_wgrad_workspace_bytes(const TimDesc* d) { return d ? ws_layout(*d).wg.bytes : 0; }

// The data chain.  dx_out_add / dx_in_add (both optional): the SPLIT form of the gradient stream between layers - the
// gradient of a layer boundary travels as an fp32 part (what LayerNorm-backward wrote) plus a 16-bit part (the input-gradient
// product of the GEMM in front of it, still carrying the fp16 gradient scale), and the next LayerNorm-backward adds the two
// as it reads them.  The two "+ residual" input-gradient GEMMs of a layer then store 20 MB instead of reading 40 and writing
// 40 (C2a), and the fp32 sum is never written: 360 instead of 440 MB of gradient-stream traffic per layer.
static int layer_bwd_data_impl(const TimDesc& d, const TimLayerParams* w, const void* saved, const float* dx_out,
                               const void* dx_out_add, float* dx_in, void* dx_in_add, void* dy, const TimLayerGrads* g,
                               void* workspace, size_t workspace_bytes, hipStream_t s) {
  int rc = check_layer_desc(d);
  if (rc) return rc;
  const WsLayout W = ws_layout(d);
  if (workspace_bytes < W.total) return TIMHIP_EWORKSPACE;
  const int M = d.B * d.S, E = d.E, FF = d.FF, prec = d.precision;
  const SavedLayout L = saved_layout(d);
  const DyLayout Y = dy_layout(d);
  const void* qkv = L.qkv.at(saved); const void* o = L.o.at(saved); const float* lse = (const float*)L.lse.at(saved);
  const float* y1 = (const float*)L.y1.at(saved); const float* st1 = (const float*)L.st1.at(saved);
  const void* u = L.u.at(saved);
  const float* y2 = (const float*)L.y2.at(saved); const float* st2 = (const float*)L.st2.at(saved);
  void* ws = workspace;
  float* f32a = (float*)W.f32a.at(ws); float* f32b = (float*)W.f32b.at(ws); float* lnp = (float*)W.lnp.at(ws);
  void* Tb = W.Tb.at(ws); void* Tc = W.Tc.at(ws);
  void* df = Y.df.at(dy); void* du = Y.du.at(dy); void* da = Y.da.at(dy); void* dqkv = Y.dqkv.at(dy);
  const LayerPass P = layer_pass(d, reinterpret_cast<const unsigned long long*>(L.attn_keep.at(saved)));
  const float* gs_in = P.gs_in; const float* gs_out = P.gs_out;

  // the residual part of the stream as 16-bit (TIMHIP_DESC_STREAM16*, fp16 mode only: same scale as the gradient operands)
  const bool s16 = gs_in != nullptr && (d.reserved & TIMHIP_DESC_STREAM16) != 0;
  const bool s16_in = s16 && (d.reserved & TIMHIP_DESC_STREAM16_IN) != 0;
  const bool s16_out = s16 && (d.reserved & TIMHIP_DESC_STREAM16_OUT) != 0;
  if (((d.reserved & (TIMHIP_DESC_STREAM16_IN | TIMHIP_DESC_STREAM16_OUT)) != 0 && !s16) || (s16_out && !dx_in_add)) return TIMHIP_EINVAL;
  // norm2 backward -> dy2 (fp32; STREAM16: T times S, in f32a's space) and df = dropout2-mask * dy2 (T)
  if ((rc = tim_layernorm_bwd(prec, dx_out, E, y2, E, st2, M, E, 0, w->n2_w, f32a, E, df, E, d.p_drop, d.seed,
                              layer_site(d.layer, SITE_L_DROP2), g->n2_w, g->n2_b,
                              g->ln_partials ? g->ln_partials : lnp, s, g->ln_partials != nullptr, gs_in,
                              dx_out_add, E, gs_out, (s16_in ? 1 : 0) | (s16 ? 2 : 0)))) return rc;
  // du = (df W2) * [dropout-mask * gelu'(pre-activation)]
  TimEpi e = epi0();
  e.out0 = du; e.ld0 = FF; e.aux = u; e.ldaux = FF;   // u = dropmask * gelu'(pre-activation), written by the forward
  if ((rc = tim_gemm_nt(prec, TIMHIP_EPI_MULAUX_T, df, E, w->l2_wt, E, M, FF, E, e, 1, s))) return rc;
  // the FFN branch's input gradient du W1 as an operand-dtype product; norm1 backward adds it to dy2 (the residual branch) as it
  // reads.  fp16 (11 bits under the gradient scale) and the fp32-storage modes (nothing is rounded) take this form; plain bf16
  // would round the branch to 8 bits per layer, so there the product joins the fp32 stream directly (dy2 += du W1, fp32)
  const bool branch_split = prec != TIMHIP_PREC_BF16;
  e = epi0();
  if (branch_split) {
    e.out0 = Tb; e.ld0 = E;
    if ((rc = tim_gemm_nt(prec, TIMHIP_EPI_STORE_T, du, FF, w->l1_wt, FF, M, E, FF, e, 1, s))) return rc;
  } else {
    e.out0 = f32b; e.ld0 = E; e.res = f32a; e.ldres = E;
    if ((rc = tim_gemm_nt(prec, TIMHIP_EPI_ADD_F32, du, FF, w->l1_wt, FF, M, E, FF, e, 1, s))) return rc;
  }
  const float* ln1_in = branch_split ? f32a : f32b;
  // norm1 backward -> dy1 (fp32) and da = dropout1-mask * dy1 (T)
  float* dy1 = dx_in_add ? dx_in : (branch_split ? f32b : f32a);
  if ((rc = tim_layernorm_bwd(prec, ln1_in, E, y1, E, st1, M, E, 0, w->n1_w, dy1, E, da, E, d.p_drop, d.seed,
                              layer_site(d.layer, SITE_L_DROP1), g->n1_w, g->n1_b,
                              g->ln_partials ? g->ln_partials + tim_layernorm_bwd_ws(M, E) / sizeof(float) : lnp, s,
                              g->ln_partials != nullptr, gs_in, branch_split ? Tb : nullptr, E, gs_out,
                              (s16 ? 1 : 0) | (s16_out ? 2 : 0)))) return rc;
  // do = da Wo
  e = epi0();
  e.out0 = Tc; e.ld0 = E;
  if ((rc = tim_gemm_nt(prec, TIMHIP_EPI_STORE_T, da, E, w->out_wt, E, M, E, E, e, 1, s))) return rc;
  // attention backward -> dqkv
  if ((rc = tim_attention_bwd(d, qkv, o, lse, Tc, dqkv, W.attn.at(ws), W.attn.bytes, s, P.akeep))) return rc;
  e = epi0();
  if (dx_in_add) {   // split form: the product stays 16-bit (and scaled); dy1 is already in dx_in
    e.out0 = dx_in_add; e.ld0 = E;
    return tim_gemm_nt(prec, TIMHIP_EPI_STORE_T, dqkv, 3 * E, w->in_wt, 3 * E, M, E, 3 * E, e, 1, s);
  }
  // dx_in = dqkv Win + dy1: the complete fp32 gradient (first layer of the stack, or a caller that wants one tensor)
  e.out0 = dx_in; e.ld0 = E; e.res = dy1; e.ldres = E; e.acc_scale = gs_out;
  return tim_gemm_nt(prec, TIMHIP_EPI_ADD_F32, dqkv, 3 * E, w->in_wt, 3 * E, M, E, 3 * E, e, 1, s);
}

int timhip_layer_bwd_data(const TimDesc* dp, const TimLayerParams* w, const void* saved, float* dx_out, float* dx_in,
                          void* dy, const TimLayerGrads* g, void* workspace, size_t workspace_bytes, void* stream) {
  if (!dp || !w || !saved || !dx_out || !dx_in || !dy || !g || !workspace) return TIMHIP_EINVAL;
  return layer_bwd_data_impl(*dp, w, saved, dx_out, nullptr, dx_in, nullptr, dy, g, workspace, workspace_bytes, (hipStream_t)stream);
}

int timhip_layer_bwd_data_split(const TimDesc* dp, const TimLayerParams* w, const void* saved, const float* dx_out,
                                const void* dx_out_add, float* dx_in, void* dx_in_add, void* dy, const TimLayerGrads* g,
                                void* workspace, size_t workspace_bytes, void* stream) {
  if (!dp || !w || !saved || !dx_out || !dx_in || !dy || !g || !workspace) return TIMHIP_EINVAL;
  return layer_bwd_data_impl(*dp, w, saved, dx_out, dx_out_add, dx_in, dx_in_add, dy, g, workspace, workspace_bytes,
                             (hipStream_t)stream);
}

int timhip_layer_bwd_weights(const TimDesc* dp, const void* x_in_T, const void* saved, const void* dy,
                             const TimLayerGrads* g, void* workspace, size_t workspace_bytes, void* stream) {
  if (!dp || !x_in_T || !saved || !dy || !g || !workspace) return TIMHIP_EINVAL;
  const TimDesc& d = *dp;
  int rc = check_layer_desc(d);
  if (rc) return rc;
  const int M = d.B * d.S;
  hipStream_t s = (hipStream_t)stream;
  const LayerPass P = layer_pass(d);
  TimWgradItem it[4];
  layer_products(d, saved, dy, x_in_T, g, it);
  // one grouped launch (wgrad.hip): 12 E^2 / 128^2 tiles with FF = 2E, i.e. 512 at E = 1024 - the contraction is not split
  if (wgrad_grouped(d)) return tim_wgrad_group_h16(d.precision, it, 4, M, P.accumulate, workspace, workspace_bytes, P.gs_out, s);
  for (const TimWgradItem& p : it)
    if ((rc = wgrad(d.precision, p.dY, p.ldy, p.Nout, p.X, p.ldx, p.Kout, M, p.dW, p.db, workspace, workspace_bytes, s, P.accumulate,
                    P.gs_out))) return rc;
  return TIMHIP_OK;
}

// The weight gradients of TWO layers in one grouped launch (round 6): at production batch sizes the eight products are 256 tiles of
// 256 x 256 for the eight-phase kernel (wgrad_pp.hip: wgrad_p8_kernel), one per CU; any other shape takes the grouped kernels the
// single-layer call takes (then as two rounds).  a / b: the arguments of timhip_layer_bwd_weights for the two layers (same
// descriptor but for `layer`, which only names the dropout sites and is not read here).
int timhip_layer_bwd_weights_pair(const TimDesc* dp, const void* x_in_T_a, const void* saved_a, const void* dy_a, const TimLayerGrads* ga,
                                  const void* x_in_T_b, const void* saved_b, const void* dy_b, const TimLayerGrads* gb,
                                  void* workspace, size_t workspace_bytes, void* stream) {
  if (!dp || !x_in_T_a || !saved_a || !dy_a || !ga || !x_in_T_b || !saved_b || !dy_b || !gb || !workspace) return TIMHIP_EINVAL;
  const TimDesc& d = *dp;
  int rc = check_layer_desc(d);
  if (rc) return rc;
  if (!wgrad_grouped(d)) return TIMHIP_EUNSUPPORTED;
  const LayerPass P = layer_pass(d);
  TimWgradItem it[8];
  layer_products(d, saved_a, dy_a, x_in_T_a, ga, it);
  layer_products(d, saved_b, dy_b, x_in_T_b, gb, it + 4);
  return tim_wgrad_group_h16(d.precision, it, 8, d.B * d.S, P.accumulate, workspace, workspace_bytes, P.gs_out, (hipStream_t)stream);
}

// 1: timhip_layer_bwd_weights_pair runs this descriptor's two layers as ONE round of eight-phase tiles (hosts defer a layer's
// weight gradients to its neighbour's only then); 0: no gain from pairing
int timhip_layer_wgrad_pair_wins(const TimDesc* dp) {
  if (!dp || check_layer_desc(*dp)) return 0;
  const TimDesc& d = *dp;
  if (!wgrad_grouped(d)) return 0;
  TimWgradItem it[8];
  layer_products(d, nullptr, nullptr, nullptr, nullptr, it);
  layer_products(d, nullptr, nullptr, nullptr, nullptr, it + 4);
  return wgrad_group_plan(tim_knobs(), it, 8, d.B * d.S).family == WGRAD_P8 ? 1 : 0;   // what the pair launch takes
}

// single-stream form: the data chain followed by the weight gradients, `dy` behind the data chain's workspace
static int layer_bwd_impl(const TimDesc* dp, const TimLayerParams* w, const void* x_in_T, const void* saved, const float* dx_out,
                          const void* dx_out_add, float* dx_in, void* dx_in_add, const TimLayerGrads* g, void* workspace,
                          size_t workspace_bytes, void* stream) {
  const WsLayout W = ws_layout(*dp);
  if (workspace_bytes < W.total + dy_layout(*dp).total) return TIMHIP_EWORKSPACE;
  char* ws = (char*)workspace;
  void* dy = ws + W.total;
  int rc = timhip_layer_bwd_data_split(dp, w, saved, dx_out, dx_out_add, dx_in, dx_in_add, dy, g, ws, W.total, stream);
  if (rc) return rc;
  return timhip_layer_bwd_weights(dp, x_in_T, saved, dy, g, W.wg.at(ws), W.wg.bytes, stream);
}

int timhip_layer_bwd(const TimDesc* dp, const TimLayerParams* w, const void* x_in_T, const void* saved, float* dx_out,
                     float* dx_in, const TimLayerGrads* g, void* workspace, size_t workspace_bytes, void* stream) {
  if (!dp) return TIMHIP_EINVAL;
  return layer_bwd_impl(dp, w, x_in_T, saved, dx_out, nullptr, dx_in, nullptr, g, workspace, workspace_bytes, stream);
}

int timhip_layer_bwd_split(const TimDesc* dp, const TimLayerParams* w, const void* x_in_T, const void* saved, const float* dx_out,
                           const void* dx_out_add, float* dx_in, void* dx_in_add, const TimLayerGrads* g, void* workspace,
                           size_t workspace_bytes, void* stream) {
  if (!dp) return TIMHIP_EINVAL;
  return layer_bwd_impl(dp, w, x_in_T, saved, dx_out, dx_out_add, dx_in, dx_in_add, g, workspace, workspace_bytes, stream);
}

}  // extern "C"
