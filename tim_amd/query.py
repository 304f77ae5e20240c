"""Encode a window once, query it many times (evaluation only).

Under TIM's mask the feature stream of a window never depends on the queries and queries never depend on each
other.  `encode_windows` runs the stack on the feature rows alone and keeps every layer's K | V columns in a `WindowCache`
(timhip_stack_encode); `query_windows` runs all layers on query rows only, against that cache (timhip_stack_query).  Both are
methods of the two models (`tim_amd.tim.TIM`, `tim_amd.detection.TIM`); this module holds what they share.  `model.eval()` and
no-grad only: there is no autograd node, no backward through a cache.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib as L
from . import functional as Fn


class WindowCache:
    """Opaque result of `encode_windows`: kv [L, W F, 2E] (operand dtype; per layer the K | V columns of the feature rows), the
    shape it was computed for, `feats` ([W, F, E] fp32, or None) and the (data_ptr, _version) of every parameter it was computed
    from - the pair the runtime's operand copies go by.  `query_windows` refuses a cache whose versions are not the model's."""
    __slots__ = ("kv", "W", "F", "E", "nlayers", "precision", "feats", "versions")

    def __init__(self, kv, W, F, E, nlayers, precision, feats, versions):
        self.kv, self.W, self.F, self.E, self.nlayers = kv, int(W), int(F), int(E), int(nlayers)
        self.precision, self.feats, self.versions = precision, feats, tuple(versions)

    @property
    def nbytes(self):
        return self.nlayers * self.W * self.F * 2 * self.E * (2 if self.precision in ("fp16", "bf16") else 4)


class QueryPlan:
    """The kind-1 rows of the full `EncoderPlan` for (nv, na), as a plan of their own: token row i = query row F + i of the full
    sequence, time rows counted from the first query's, head slices relative to the first query row."""

    def __init__(self, cfg, nv, na):
        full = Fn.EncoderPlan(cfg, cfg.F + nv + na, nv, na)
        F = full.F
        self.full = full
        self.rows = [(k, src, te - F, mod) for (k, src, te, mod) in full.rows if k == 1]
        assert len(self.rows) == full.S - F and all(r[2] >= 0 for r in self.rows)
        self.S, self.F, self.T = len(self.rows), F, nv + na
        self.cls_names, self.mod_names, self.embedders = full.cls_names, full.mod_names, []
        self.heads = [(slot, pname, s0 - F, n) for (slot, pname, s0, n) in full.heads]
        self.reg = [(slot, pname, s0 - F, n) for (slot, pname, s0, n) in full.reg]
        self._table = {}

    table = Fn.EncoderPlan.table


def _query_plan(model, nv, na):
    key = ("query", nv, na)
    p = model._plans.get(key)
    if p is None:
        p = model._plans[key] = QueryPlan(model.cfg, nv, na)
    return p


def cache_params(model):
    """every parameter a cache depends on: the encoder's, the time MLP's where the model computes the feature time encodings
    itself (detection), the pooling pre-step's"""
    ps = list(model._encoder_param_list())
    if model.cfg.variant == "detection":
        ps += list(model.time_mlp.parameters())
    if model.pool is not None:
        ps += list(model.pool.parameters())
    return ps


def param_versions(model):
    return tuple((p.data_ptr(), p._version) for p in cache_params(model))


def _need_eval(model, what):
    if model.training:
        raise ValueError("%s is an evaluation call: model.eval() first (no dropout, no backward through a window cache)" % what)


def resolve_window_index(window_index, G, W, dev, validate=True):
    """-> None (identity) or a CUDA int32 tensor of G window numbers.  Host-side values (list, numpy array, CPU tensor) are
    range-checked here; a CUDA tensor with one reduction and a sync unless validate is False (captured graphs: the caller owns the
    range, the kernel's NaN guard is the backstop)."""
    if window_index is None:
        if G != W:
            raise ValueError("%d query groups for a cache of %d windows: pass window_index (one window number per group)" % (G, W))
        return None
    if isinstance(window_index, torch.Tensor) and window_index.is_cuda:
        if window_index.dtype != torch.int32 or window_index.dim() != 1 or not window_index.is_contiguous():
            raise ValueError("a CUDA window_index must be a contiguous 1-D int32 tensor")
        if window_index.numel() != G:
            raise ValueError("window_index has %d entries for %d query groups" % (window_index.numel(), G))
        if validate and bool(((window_index < 0) | (window_index >= W)).any().item()):   # one reduction, one sync
            raise ValueError("window_index holds a window outside [0, %d)" % W)
        return window_index
    idx = np.asarray(window_index.numpy() if isinstance(window_index, torch.Tensor) else window_index)
    if idx.ndim != 1 or idx.shape[0] != G:
        raise ValueError("window_index must hold one window number per query group (%d), got shape %s" % (G, tuple(idx.shape)))
    if idx.size and (not np.issubdtype(idx.dtype, np.integer) or idx.min() < 0 or idx.max() >= W):
        raise ValueError("window_index holds a window outside [0, %d) (or is not integral)" % W)
    return torch.as_tensor(idx.astype(np.int32)).to(dev)


def check_cache(model, cache):
    """a cache this model can answer from: same shape and precision (ValueError), same parameter contents (RuntimeError)"""
    cfg, rt = model.cfg, model.rt
    if not isinstance(cache, WindowCache):
        raise ValueError("query_windows needs the WindowCache encode_windows returned, got %s" % type(cache).__name__)
    if cache.precision != rt.precision_name:
        raise ValueError("the cache holds %s keys and values, the model runs %s" % (cache.precision, rt.precision_name))
    if cache.F != cfg.F or cache.E != cfg.E or cache.nlayers != cfg.num_layers:
        raise ValueError("the cache was encoded for F = %d, E = %d, %d layers; the model has F = %d, E = %d, %d layers"
                         % (cache.F, cache.E, cache.nlayers, cfg.F, cfg.E, cfg.num_layers))
    if cache.versions != param_versions(model):
        raise RuntimeError("stale WindowCache: the model's parameters changed since encode_windows (an optimizer step, "
                           "load_state_dict, or a cache of another model) - encode the windows again")


def encode(model, visual, audio, te, want_feats=False):
    """feature rows of W windows through the stack -> WindowCache.  te: [W, >= F, d] time encodings, the first F rows are used"""
    _need_eval(model, "encode_windows")
    cfg, rt = model.cfg, model.rt
    if te.dim() != 3 or te.shape[2] != cfg.d_model:
        raise ValueError("time encodings must be [W, >= %d, d_model = %d], got %s" % (cfg.F, cfg.d_model, tuple(te.shape)))
    if te.shape[1] < cfg.F:
        raise ValueError("time encodings have %d rows per window, the %d feature tokens need %d" % (te.shape[1], cfg.F, cfg.F))
    Fn._require_gpu(te, "encode_windows")
    with torch.no_grad():
        W, T, _ = te.shape
        q = Fn._Pass(model, model._plan(cfg.F, 0, 0), te.device, W, T, False, 0)   # (T: the row pitch of te; the plan reads rows < F)
        P = dict(zip(q.names, model._encoder_param_list()))
        versions = param_versions(model)
        _, e_bufs = Fn._embedders_fwd(q, P, visual, audio)
        x0_f, x0_t = Fn._assemble_fwd(q, P, e_bufs, Fn._f32c(te))
        Lyr = cfg.num_layers
        desc = L.TimDesc(W, q.F, q.F, q.d, q.E, cfg.nhead, cfg.FF, rt.prec, 0.0, 0, 0, rt.layer_split_flags(q.E, cfg.FF), None)
        lparams = [model._layer_params(rt, P, "%s.layers.%d." % (model._stack_prefix, l)) for l in range(Lyr)]
        layers = (L.TimLayerParams * Lyr)(*[lp[0] for lp in lparams])
        kv = torch.empty((Lyr, W * q.F, 2 * q.E), dtype=rt.op_dtype, device=q.dev)
        assert L.load().timhip_window_cache_bytes(C.byref(desc), Lyr) == kv.numel() * kv.element_size()
        feats = torch.empty((W * q.F, q.E), dtype=torch.float32, device=q.dev) if want_feats else None
        ws_bytes = L.load().timhip_stack_infer_workspace_bytes(C.byref(desc), Lyr, 0)
        ws = model._workspace(ws_bytes, q.dev, slot="infer")
        L.call("timhip_stack_encode", C.byref(desc), Lyr, layers, L.ptr(x0_f), L.ptr(x0_t), L.ptr(feats), L.ptr(kv), L.ptr(ws), ws_bytes,
               q.st)
        return WindowCache(kv, W, q.F, q.E, Lyr, rt.precision_name, None if feats is None else feats.view(W, q.F, q.E), versions)


def check_query_encodings(model, te_q, nv, na):
    cfg = model.cfg
    if te_q.dim() != 3 or te_q.shape[2] != cfg.d_model:
        raise ValueError("query time encodings must be [G, num_v_queries + num_a_queries, d_model = %d], got %s"
                         % (cfg.d_model, tuple(te_q.shape)))
    if te_q.shape[1] != nv + na or nv + na == 0:
        raise ValueError("query time encodings hold %d rows per group, num_v_queries + num_a_queries = %d"
                         % (te_q.shape[1], nv + na))


def query(model, cache, te_q, nv, na, window_index=None, validate=True, maps=None):
    """all layers on the query rows of G groups against `cache` -> the encoder's outputs by slot (dict; no `feats`).
    te_q: [G, nv + na, d] time encodings of the queries, visual first.  maps (an attn_maps.QueryMapRequest:
    `model.query_attention_maps`): the same walk through timhip_stack_query_maps, which also writes the requested layers' maps."""
    _need_eval(model, "query_windows")
    check_cache(model, cache)
    check_query_encodings(model, te_q, nv, na)
    plan = _query_plan(model, nv, na)       # (raises ValueError where the counts do not fit the model's modalities)
    G = te_q.shape[0]
    widx = resolve_window_index(window_index, G, cache.W, te_q.device, validate)
    Fn._require_gpu(te_q, "query_windows")
    if cache.kv.device != te_q.device:
        raise ValueError("the cache lives on %s, the queries on %s" % (cache.kv.device, te_q.device))
    cfg, rt = model.cfg, model.rt
    with torch.no_grad():
        q = Fn._Pass(model, plan, te_q.device, G, nv + na, False, 0)
        P = dict(zip(q.names, model._encoder_param_list()))
        x0_f, x0_t = Fn._assemble_fwd(q, P, [None, None], Fn._f32c(te_q))
        Lyr = cfg.num_layers
        desc = L.TimDesc(G, q.S, cache.F, q.d, q.E, cfg.nhead, cfg.FF, rt.prec, 0.0, 0, 0, rt.layer_split_flags(q.E, cfg.FF), None)
        lparams = [model._layer_params(rt, P, "%s.layers.%d." % (model._stack_prefix, l)) for l in range(Lyr)]
        layers = (L.TimLayerParams * Lyr)(*[lp[0] for lp in lparams])
        xL_f = torch.empty((q.M, q.E), dtype=torch.float32, device=q.dev)
        xL_t = torch.empty((q.M, q.E), dtype=rt.op_dtype, device=q.dev)
        ws_bytes = L.load().timhip_stack_query_workspace_bytes(C.byref(desc), Lyr)
        ws = model._workspace(ws_bytes, q.dev, slot="query")
        if maps is not None:
            maps.run(model, q, plan, desc, Lyr, layers, cache, widx, x0_f, x0_t, xL_f, xL_t, ws, ws_bytes)
        else:
            L.call("timhip_stack_query", C.byref(desc), Lyr, layers, L.ptr(cache.kv), cache.W, L.ptr(widx), L.ptr(x0_f), L.ptr(x0_t),
                   L.ptr(xL_f), L.ptr(xL_t), L.ptr(ws), ws_bytes, q.st)
        outs = {}
        Fn._heads_fwd(q, P, xL_f, xL_t, outs)
        Fn._reg_heads_fwd(q, P, xL_t, outs)
        return outs
