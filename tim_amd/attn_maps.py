"""Query attention maps: the per-layer attention weights of the encoder's evaluation forward.

The reference's `TransformerEncoder.forward` returns `(output, attn_weights)` (transformers.py:45-48): the head-averaged softmax
weights of `nn.MultiheadAttention`, [B, S, S] - which feature tokens, at which times, a query reads.  TIM's mask (tim.py:161-166)
leaves a row F + 1 non-zeros at most - the F feature tokens and the token itself - so the maps are kept as [B, S - s0, F + 1]:
columns 0 .. F - 1 the feature tokens, column F the token's own key (exact 0 for feature rows, whose own key is one of the F).
`model.attention_maps(...)` runs the evaluation forward through `timhip_stack_infer_maps`: the same stack walk as
`model(inputs, "encoder", ...)` under `eval()` / `no_grad()` - bit-identical outputs - with one weights kernel per requested layer
(csrc/attn_maps.hip) while that layer's qkv is live in the arena.
`model.query_attention_maps(cache, ...)` is the same for a `query.WindowCache`: `query_windows`' walk over the query rows alone
through `timhip_stack_query_maps`, the weights kernel reading layer l's keys from the cache through the window index - the maps'
first axis is then the query group, their feature columns those of the group's own window."""
import ctypes as C

import torch

from ._lib import call, ptr


def resolve_layers(layers, num_layers):
    """"last" | "all" | an iterable of layer indices (negative: from the end) -> ascending list of distinct indices"""
    if isinstance(layers, str):
        if layers == "last":
            return [num_layers - 1]
        if layers == "all":
            return list(range(num_layers))
        raise ValueError('layers: "last", "all" or a list of layer indices, not %r' % (layers,))
    try:
        idx = list(layers)
    except TypeError:
        raise ValueError('layers: "last", "all" or a list of layer indices, not %r' % (layers,)) from None
    if not idx:
        raise ValueError("layers: the list of layer indices is empty")
    out = []
    for i in idx:
        if isinstance(i, bool) or not isinstance(i, int):
            raise ValueError("layers: %r is not a layer index" % (i,))
        if not -num_layers <= i < num_layers:
            raise ValueError("layers: index %d outside the model's %d layers" % (i, num_layers))
        out.append(i % num_layers)
    if len(set(out)) != len(out):
        raise ValueError("layers: a layer is named twice in %r" % (idx,))
    return sorted(out)


def resolve_rows(rows, F):
    """"queries" (the query tokens: s0 = F) | "all" (s0 = 0) -> s0"""
    if rows == "queries":
        return F
    if rows == "all":
        return 0
    raise ValueError('rows: "queries" or "all", not %r' % (rows,))


class AttentionMaps:
    """The maps of one call.  `layers`: the layer indices, ascending; `weights[l]`: fp32 [B, S - s0, F + 1]; `F`, `S`, `s0`: the
    layout (row i = token s0 + i).  Maps of a `WindowCache` (`query_attention_maps`): B = the query groups, s0 = F, S = F + the
    queries per group; with per_head=True there `weights[l]` is [G, H, S - s0, F + 1] and every view keeps the head axis."""

    def __init__(self, layers, weights, F, S, s0, heads=(), num_feats=None):
        self.layers = list(layers)
        self.weights = dict(zip(self.layers, weights))
        self.F, self.S, self.s0 = int(F), int(S), int(s0)
        self._heads = {h[0]: (h[2], h[3]) for h in heads}     # output slot -> (first token row, rows): EncoderPlan.heads
        self._nf = num_feats                                  # feature tokens per modality of an audio-visual model, or None
        for w in self.weights.values():
            if w.dim() not in (3, 4) or w.shape[-2] != self.S - self.s0 or w.shape[-1] != self.F + 1:
                raise ValueError("a map is [B, S - s0, F + 1] = [B, %d, %d], not %s" % (self.S - self.s0, self.F + 1, tuple(w.shape)))
        self.per_head = any(w.dim() == 4 for w in self.weights.values())

    def _w(self, layer):
        if layer is None:
            layer = self.layers[-1]
        if layer not in self.weights:
            raise KeyError("layer %r was not asked for (layers: %r)" % (layer, self.layers))
        return self.weights[layer]

    def to_dense(self, layer=None):
        """[B, S - s0, S] as the reference lays its rows out: feature columns copied, the self column on the diagonal, zeros
        elsewhere"""
        w = self._w(layer)
        n, F, S, s0 = self.S - self.s0, self.F, self.S, self.s0
        dense = w.new_zeros(tuple(w.shape[:-2]) + (n, S))
        dense[..., :F] = w[..., :F]
        first = max(F, s0)                                    # query rows: token s sits in row s - s0 and owns column s
        if first < S:
            tok = torch.arange(first, S, device=w.device)
            dense[..., tok - s0, tok] = w[..., first - s0:, F]
        return dense

    def for_head(self, name, layer=None):
        """[B, Nq, F + 1]: the rows of the queries one head reads (name: "verb", "noun", "action" or "audio")"""
        if name not in self._heads:
            raise KeyError("this model has no %r head (heads: %r)" % (name, sorted(self._heads)))
        start, n = self._heads[name]
        if start < self.s0:
            raise ValueError("rows of head %r start at token %d, the maps at token %d" % (name, start, self.s0))
        return self._w(layer)[..., start - self.s0:start - self.s0 + n, :]

    def split_modalities(self, layer=None):
        """(visual, audio): the two halves of the feature columns of an audio-visual model, [B, S - s0, num_feats] each"""
        if self._nf is None:
            raise ValueError("split_modalities: the model has one input modality")
        w = self._w(layer)
        return w[..., :self._nf], w[..., self._nf:self.F]


class MapRequest:
    """What one `attention_maps` call asks of the evaluation forward (`functional._infer_forward`), and its result"""

    def __init__(self, model, layers, rows, out=None):
        if model.training:
            raise ValueError("attention_maps needs model.eval(): under .train() the reference returns the attention weights after "
                             "dropout - a dropout mask over the weights, not a map - and this model does not compute those")
        cfg = model.cfg
        self.layers = resolve_layers(layers, cfg.num_layers)
        self.s0 = resolve_rows(rows, cfg.F)
        self.out = out
        self.result = None

    def _buffers(self, B, S, F, dev):
        n, shape = len(self.layers), (B, S - self.s0, F + 1)
        out = self.out
        if out is None:
            return list(torch.empty((n,) + shape, dtype=torch.float32, device=dev).unbind(0))
        if isinstance(out, AttentionMaps):
            if out.layers != self.layers:
                raise ValueError("out: maps of layers %r, this call asks for %r" % (out.layers, self.layers))
            out = [out.weights[l] for l in self.layers]
        bufs = list(out)
        if len(bufs) != n:
            raise ValueError("out: %d buffers for %d layers" % (len(bufs), n))
        for t in bufs:
            if tuple(t.shape) != shape or t.dtype != torch.float32 or t.device != dev or not t.is_contiguous():
                raise ValueError("out: every buffer is a contiguous fp32 %s tensor on %s" % (shape, dev))
        return bufs

    def run(self, model, q, desc, nlayers, layers, x0_f, x0_t, xL_f, xL_t, tail, ws, ws_bytes):
        """timhip_stack_infer with the maps of the requested layers (NULL for every other layer)"""
        if q.S == q.F and self.s0 == q.F:
            raise ValueError('attention_maps: this call has no query tokens; ask for rows="all"')
        bufs = self._buffers(q.B, q.S, q.F, q.dev)
        by_layer = dict(zip(self.layers, bufs))
        maps = (C.c_void_p * nlayers)(*[ptr(by_layer[l]) if l in by_layer else None for l in range(nlayers)])
        call("timhip_stack_infer_maps", C.byref(desc), nlayers, layers, ptr(x0_f), ptr(x0_t), ptr(xL_f), ptr(xL_t), int(tail), maps,
             self.s0, q.F + 1, ptr(ws), ws_bytes, q.st)
        cfg = model.cfg
        nf = cfg.num_feats if cfg.input_modality == "audio_visual" else None
        self.result = AttentionMaps(self.layers, bufs, q.F, q.S, self.s0, heads=q.plan.heads, num_feats=nf)


class QueryMapRequest:
    """What one `query_attention_maps` call asks of `query.query`, and its result: the maps of the query rows of G groups against
    a `WindowCache`, [G, Q, F + 1] (per_head: [G, H, Q, F + 1]) for every layer asked for"""

    def __init__(self, model, layers, per_head=False, out=None):
        if model.training:
            raise ValueError("query_attention_maps is an evaluation call: model.eval() first (no dropout, no backward through a "
                             "window cache)")
        self.layers = resolve_layers(layers, model.cfg.num_layers)
        self.per_head = bool(per_head)
        self.out = out
        self.result = None

    def _buffers(self, G, Q, F, H, dev):
        n, shape = len(self.layers), ((G, H, Q, F + 1) if self.per_head else (G, Q, F + 1))
        out = self.out
        if out is None:
            return list(torch.empty((n,) + shape, dtype=torch.float32, device=dev).unbind(0))
        if isinstance(out, AttentionMaps):
            if out.layers != self.layers:
                raise ValueError("out: maps of layers %r, this call asks for %r" % (out.layers, self.layers))
            out = [out.weights[l] for l in self.layers]
        bufs = list(out)
        if len(bufs) != n:
            raise ValueError("out: %d buffers for %d layers" % (len(bufs), n))
        for t in bufs:
            if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or t.dtype != torch.float32 or t.device != dev \
                    or not t.is_contiguous():
                raise ValueError("out: every buffer is a contiguous fp32 %s tensor on %s" % (shape, dev))
        return bufs

    def run(self, model, q, plan, desc, nlayers, layers, cache, widx, x0_f, x0_t, xL_f, xL_t, ws, ws_bytes):
        """timhip_stack_query with the maps of the requested layers (NULL for every other layer)"""
        cfg = model.cfg
        bufs = self._buffers(q.B, q.S, cache.F, cfg.nhead, q.dev)
        by_layer = dict(zip(self.layers, bufs))
        maps = (C.c_void_p * nlayers)(*[ptr(by_layer[l]) if l in by_layer else None for l in range(nlayers)])
        call("timhip_stack_query_maps", C.byref(desc), nlayers, layers, ptr(cache.kv), cache.W, ptr(widx), ptr(x0_f), ptr(x0_t),
             ptr(xL_f), ptr(xL_t), maps, int(self.per_head), cache.F + 1, ptr(ws), ws_bytes, q.st)
        nf = cfg.num_feats if cfg.input_modality == "audio_visual" else None
        self.result = AttentionMaps(self.layers, bufs, cache.F, cache.F + q.S, cache.F, heads=plan.full.heads, num_feats=nf)
