"""The transform-then-aggregate GAT layers behind hip_ops: node scores, the fused softmax-aggregate and
its backward (GATAggregate), GATv2 (GATv2Aggregate), the attention read-backs and per-destination
top-k, and the whole-layer ``GATLayer`` autograd function with its fused dx / weight-gradient
paths, the producer hand-off and the side-stream weight gradients.

``_SIDE_STREAMS`` and ``_PENDING_JOINS`` are this module's state.  The kink tap lives in
ops_graph (the aggregate-then-transform layer records into it too).
"""
from __future__ import annotations

import os
import weakref
from typing import Optional

import torch

from . import _launch, _lib, ops_graph
from .ops_gemm import att_proj, gemm_tn, join_rows, mm_nn, project, project_supported, rank_update_, weight_grads
from .ops_graph import (CSRGraph, Schedule, _check_dev, _csr2csc, _require, _tap_kinks, edge_terms, seed_buffer,
                        stage_edge_attr)
from .ops_xgat import XViews, gat_layer_x, xgat_forward, xgat_supported


# ---------------------------------------------------------------------------
# node scores / fused forward / fused backward
# ---------------------------------------------------------------------------
def node_scores(h: torch.Tensor, att_src: torch.Tensor, att_dst: torch.Tensor, heads: int, channels: int):
    N = h.size(0)
    _check_dev("h", h, torch.float32)
    _check_dev("att_src", att_src, torch.float32, h.device)
    _check_dev("att_dst", att_dst, torch.float32, h.device)
    _require(h.numel() == N * heads * channels, "h must be [N, heads*channels]")
    _require(att_src.numel() == heads * channels and att_dst.numel() == heads * channels, "att must be [H, C]")
    s_src = torch.empty(N, heads, dtype=torch.float32, device=h.device)
    s_dst = torch.empty(N, heads, dtype=torch.float32, device=h.device)
    _launch.node_scores(h, att_src, att_dst, heads, channels, s_src, s_dst)
    return s_src, s_dst


def gat_fwd(g: CSRGraph, h, s_src, s_dst, bias, heads: int, channels: int, mode: int, slope: float,
            dropout_p: float, seed: int, want_agg: bool, seed_buf: Optional[torch.Tensor] = None, edge_term=None):
    N = g.n_nodes
    dev = h.device
    _require(h.size(0) == N, f"x has {h.size(0)} rows but the graph has {N} nodes")
    out, m, inv_l, agg = _fwd_outputs(N, heads, channels, want_agg, dev)
    _fwd_rows(g, g.fwd_sched, 0, N, h, s_src, s_dst, bias, heads, channels, mode, slope, dropout_p, seed, seed_buf,
              out, m, inv_l, agg, edge_term)
    return out, m, inv_l, agg


def _fwd_outputs(N: int, heads: int, channels: int, want_agg: bool, dev):
    out = torch.empty(N, channels, dtype=torch.float32, device=dev)
    m = torch.empty(N, heads, dtype=torch.float32, device=dev)
    inv_l = torch.empty(N, heads, dtype=torch.float32, device=dev)
    agg = torch.empty(N, heads, channels, dtype=torch.float32, device=dev) if want_agg else None
    return out, m, inv_l, agg


def _fwd_rows(g: CSRGraph, sched: Schedule, r0: int, n: int, h, s_src, s_dst, bias, heads: int, channels: int,
              mode: int, slope: float, dropout_p: float, seed: int, seed_buf, out, m, inv_l, agg, edge_term=None):
    """The forward over the destination rows [r0, r0 + n) of ``sched`` (row ids relative to
    r0; edge slots and source rows absolute): destination-indexed pointers are offset by r0."""
    _launch.fwd(sched, g.col, g.csr_eid, g.n_edges, r0, n, h, s_src, s_dst, bias, heads, channels, mode, slope,
                dropout_p, seed, seed_buf, out, m, inv_l, agg, edge_term)


def gat_bwd(g: CSRGraph, h, s_src, s_dst, att_src, att_dst, bias, out, agg, m, inv_l, grad_out, heads: int,
            channels: int, mode: int, slope: float, dropout_p: float, seed: int, want_bias_grad: bool = False,
            seed_buf: Optional[torch.Tensor] = None):
    N = g.n_nodes
    dev = h.device
    _check_dev("grad_out", grad_out, torch.float32, dev)
    grad_h = torch.empty(N, heads * channels, dtype=torch.float32, device=dev)
    datt_src = torch.empty(heads, channels, dtype=torch.float32, device=dev)
    datt_dst = torch.empty(heads, channels, dtype=torch.float32, device=dev)
    dbias = torch.empty(channels, dtype=torch.float32, device=dev) if want_bias_grad else None
    _launch.bwd(g, h, s_src, s_dst, att_src, att_dst, bias, out, agg, m, inv_l, grad_out, heads, channels, mode, slope,
                dropout_p, seed, seed_buf, grad_h, datt_src, datt_dst, dbias)
    return grad_h, datt_src, datt_dst, dbias


class GATAggregate(torch.autograd.Function):
    """h [N, H*C] -> out [N, C]: node scores + fused softmax-aggregate (fwd) and the
    atomic-free backward.  The projection ``h = lin(x)`` stays outside, in autograd."""

    @staticmethod
    def forward(ctx, h, att_src, att_dst, bias, graph: CSRGraph, heads: int, channels: int, mode: int,
                slope: float, dropout_p: float, seed: int):
        h = h.contiguous()
        att_src_c = att_src.detach().contiguous().view(heads, channels)
        att_dst_c = att_dst.detach().contiguous().view(heads, channels)
        bias_c = bias.detach().contiguous() if bias is not None else None
        s_src, s_dst = node_scores(h, att_src_c, att_dst_c, heads, channels)
        need_grad = any(ctx.needs_input_grad[:4])
        ctx.seed_buf = seed_buffer(dropout_p, h.device) if need_grad else None
        out, m, inv_l, agg = gat_fwd(graph, h, s_src, s_dst, bias_c, heads, channels, mode, slope, dropout_p, seed,
                                     want_agg=need_grad and heads > 1, seed_buf=ctx.seed_buf)
        if need_grad:
            ctx.save_for_backward(h, att_src_c, att_dst_c, s_src, s_dst, out, m, inv_l,
                                  agg if agg is not None else torch.empty(0, device=h.device),
                                  bias_c if bias_c is not None else torch.empty(0, device=h.device))
        ctx.graph = graph
        ctx.meta = (heads, channels, mode, slope, dropout_p, seed, bias is not None, agg is not None)
        ctx.att_shapes = (att_src.shape, att_dst.shape)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        h, att_src, att_dst, s_src, s_dst, out, m, inv_l, agg, bias = ctx.saved_tensors
        heads, channels, mode, slope, p, seed, has_bias, has_agg = ctx.meta
        grad_out = grad_out.contiguous()
        want_db = has_bias and ctx.needs_input_grad[3]
        grad_h, datt_src, datt_dst, dbias = gat_bwd(ctx.graph, h, s_src, s_dst, att_src, att_dst,
                                                    bias if has_bias else None, out, agg if has_agg else None, m,
                                                    inv_l, grad_out, heads, channels, mode, slope, p, seed,
                                                    want_bias_grad=want_db, seed_buf=ctx.seed_buf)
        return (grad_h, datt_src.view(ctx.att_shapes[0]), datt_dst.view(ctx.att_shapes[1]), dbias,
                None, None, None, None, None, None, None)


def gat_aggregate(h, att_src, att_dst, bias, graph, heads, channels, mode, slope, dropout_p=0.0, seed=0):
    return GATAggregate.apply(h, att_src, att_dst, bias, graph, heads, channels, mode, slope, dropout_p, seed)


# ---------------------------------------------------------------------------
# GATv2 dynamic attention (ppgat_dynatt_*)
# ---------------------------------------------------------------------------
def gatv2_supported(heads: int, channels: int) -> bool:
    """ppgat_dynatt_supported: the (heads, channels) the fused GATv2 kernels are built for."""
    return _launch.dynatt_supported(heads, channels)


def _gatv2_require_shape(heads: int, channels: int):
    if not gatv2_supported(heads, channels):
        raise NotImplementedError(f"GATv2 (heads={heads}, channels={channels}) not implemented: (H, C) in "
                                  "(1,32) (1,64) (1,128) (2,64) (2,128) (4,64) (4,128)")


class GATv2Aggregate(torch.autograd.Function):
    """x_l, x_r [N, H*C] -> out [N, C]: the fused dynamic-attention softmax-aggregate and its
    atomic-free backward (a D sweep, one pass by source for dx_l, one by destination for dx_r, datt).
    ``x_r`` may be ``x_l`` itself (share_weights): autograd then adds the two row gradients."""

    @staticmethod
    def forward(ctx, xl, xr, att, bias, graph: CSRGraph, heads: int, channels: int, slope: float, dropout_p: float,
                seed: int):
        N, dev = graph.n_nodes, xl.device
        shared = xr is xl or (xr.data_ptr() == xl.data_ptr() and xr.stride() == xl.stride())
        xl = xl.contiguous()
        xr = xl if shared else xr.contiguous()
        att_c = att.detach().contiguous().view(heads, channels)
        bias_c = bias.detach().contiguous() if bias is not None else None
        need_grad = any(ctx.needs_input_grad[:4])
        ctx.seed_buf = seed_buffer(dropout_p, dev)
        out, m, inv_l, _ = _fwd_outputs(N, heads, channels, False, dev)
        _launch.dynatt_fwd(graph, xl, xr, att_c, bias_c, heads, channels, slope, dropout_p, seed, ctx.seed_buf, out, m,
                           inv_l)
        if need_grad:
            ctx.save_for_backward(xl, xr, att_c, m, inv_l)
        ctx.graph = graph
        ctx.meta = (heads, channels, slope, dropout_p, bias is not None)
        ctx.att_shape = att.shape
        return out

    @staticmethod
    def backward(ctx, grad_out):
        xl, xr, att, m, inv_l = ctx.saved_tensors
        heads, channels, slope, p, has_bias = ctx.meta
        grad_out = grad_out.contiguous()
        _check_dev("grad_out", grad_out, torch.float32, xl.device)
        dxl, dxr = torch.empty_like(xl), torch.empty_like(xl)
        datt = torch.empty(heads, channels, dtype=torch.float32, device=xl.device)
        dbias = torch.empty(channels, dtype=torch.float32, device=xl.device) \
            if has_bias and ctx.needs_input_grad[3] else None
        _launch.dynatt_bwd(ctx.graph, xl, xr, att, m, inv_l, grad_out, heads, channels, slope, p, ctx.seed_buf, dxl, dxr,
                           datt, dbias)
        return dxl, dxr, datt.view(ctx.att_shape), dbias, None, None, None, None, None, None


def gatv2_aggregate(xl, xr, att, bias, graph, heads, channels, slope, dropout_p=0.0, seed=0):
    """GATv2Conv after its projections: ``out_i = mean_h sum_j alpha_ij x_l[j] + bias`` with
    ``alpha = softmax_i(att . leaky_relu(x_l[j] + x_r[i]))`` (include/ppgat.h ppgat_dynatt_fwd)."""
    heads, channels = int(heads), int(channels)
    for name, t in (("xl", xl), ("xr", xr), ("att", att)) + ((("bias", bias),) if bias is not None else ()):
        _require(isinstance(t, torch.Tensor), f"{name}: expected a tensor")
        _require(t.is_cuda, f"{name}: ppgat runs on ROCm devices only (got {t.device}); there is no CPU path")
        _require(t.dtype == torch.float32, f"{name}: expected torch.float32, got {t.dtype}")
        _require(t.device == xl.device, f"{name}: on {t.device}, expected {xl.device}")
    _gatv2_require_shape(heads, channels)
    N = graph.n_nodes
    _require(xl.dim() == 2 and tuple(xl.shape) == (N, heads * channels),
             f"xl must be [{N}, {heads * channels}], got {tuple(xl.shape)}")
    _require(tuple(xr.shape) == tuple(xl.shape), "xr must have xl's shape")
    _require(att.numel() == heads * channels, "att must be [H, C]")
    _require(bias is None or bias.numel() == channels, "bias must be [C]")
    _require(0.0 <= float(dropout_p) < 1.0, "dropout p must be in [0, 1)")
    return GATv2Aggregate.apply(xl, xr, att, bias, graph, heads, channels, float(slope), float(dropout_p), int(seed))


# ---------------------------------------------------------------------------
# attention weights (ppgat_attention, ppgat_dynatt_attention, ppgat_attention_topk)
# ---------------------------------------------------------------------------
_ORDERS = {"slot": 0, "edge": 1}


def _attention_out(graph: CSRGraph, heads: int, order: str, dev):
    _require(order in _ORDERS, f"order: expected 'edge' (edge_index column order) or 'slot' (CSR slot order), "
                               f"got {order!r}")
    return _ORDERS[order], torch.empty(graph.n_edges, heads, dtype=torch.float32, device=dev)


def _check_state(graph: CSRGraph, heads: int, dev, **named):
    for name, t in named.items():
        _check_dev(name, t, torch.float32, dev)
        _require(t.numel() == graph.n_nodes * heads, f"{name} must be [{graph.n_nodes}, {heads}]")


def attention_weights(graph: CSRGraph, s_src, s_dst, m, inv_l, heads: int, mode: int, slope: float, edge_term=None,
                      order: str = "edge") -> torch.Tensor:
    """alpha [E, H] of a v1 layer (GATConv, SimpleGATLayer, the aggregate-then-transform layer):
    the softmax weight of every edge and head BEFORE the dropout mask, recomputed from the node
    scores and the softmax state (m, inv_l) a forward over those scores left (gat_fwd,
    xgat_forward).  ``edge_term`` [E, H] in CSR slot order (edge_terms): the edge-feature logit
    term.  ``order``: "edge" -- row k belongs to column k of the edge_index the graph was built
    from -- or "slot" (CSR slot order, what attention_topk reads).  No gradient."""
    heads = int(heads)
    _check_dev("s_src", s_src, torch.float32)
    dev = s_src.device
    _require(1 <= heads <= 8, "heads must be in [1, 8]")
    _require(s_src.numel() == graph.n_nodes * heads, f"s_src must be [{graph.n_nodes}, {heads}]")
    _check_state(graph, heads, dev, s_dst=s_dst, m=m, inv_l=inv_l)
    if edge_term is not None:
        _check_dev("edge_term", edge_term, torch.float32, dev)
        _require(edge_term.numel() >= graph.n_edges * heads, f"edge_term must be [{graph.n_edges}, {heads}]")
    code, alpha = _attention_out(graph, heads, order, dev)
    with torch.cuda.device(dev):
        _launch.attention(graph, s_src, s_dst, m, inv_l, heads, int(mode), slope, code, alpha, edge_term)
    return alpha


def gatv2_attention_weights(graph: CSRGraph, xl, xr, att, m, inv_l, heads: int, channels: int, slope: float,
                            order: str = "edge") -> torch.Tensor:
    """alpha [E, H] of a GATv2 layer before the dropout mask, from the projections x_l, x_r
    [N, H * C] and the state (m, inv_l) _launch.dynatt_fwd left for them; ``order`` as in
    attention_weights.  No gradient."""
    heads, channels = int(heads), int(channels)
    _gatv2_require_shape(heads, channels)
    _check_dev("xl", xl, torch.float32)
    dev = xl.device
    _check_dev("xr", xr, torch.float32, dev)
    _check_dev("att", att, torch.float32, dev)
    _require(tuple(xl.shape) == (graph.n_nodes, heads * channels),
             f"xl must be [{graph.n_nodes}, {heads * channels}], got {tuple(xl.shape)}")
    _require(tuple(xr.shape) == tuple(xl.shape), "xr must have xl's shape")
    _require(att.numel() == heads * channels, "att must be [H, C]")
    _check_state(graph, heads, dev, m=m, inv_l=inv_l)
    code, alpha = _attention_out(graph, heads, order, dev)
    with torch.cuda.device(dev):
        _launch.dynatt_attention(graph, xl, xr, att, m, inv_l, heads, channels, slope, code, alpha)
    return alpha


def attention_topk(graph: CSRGraph, val_slot_order: torch.Tensor, k: int):
    """(eid [N, k] int32, val [N, k], cnt [N] int32): per destination the k (1..32) in-edges with the
    largest head mean of ``val_slot_order`` [E, H] (CSR slot order: attention_weights(...,
    order="slot")), ranked exactly under (value descending, original edge id ascending); eid are
    edge_index column ids, -1 (value 0) past the in-degree; cnt = min(k, in-degree)."""
    _check_dev("val_slot_order", val_slot_order, torch.float32)
    dev = val_slot_order.device
    E, N = graph.n_edges, graph.n_nodes
    _require(val_slot_order.dim() == 2 and val_slot_order.size(0) == E and 1 <= val_slot_order.size(1) <= 8,
             f"val_slot_order must be [{E}, H <= 8], got {tuple(val_slot_order.shape)}")
    _require(isinstance(k, int) and 1 <= k <= 32, "k must be an int in [1, 32]")
    _require(graph.rowptr.device == dev, f"val_slot_order: on {dev}, the graph on {graph.rowptr.device}")
    eid = torch.empty(N, k, dtype=torch.int32, device=dev)
    val = torch.empty(N, k, dtype=torch.float32, device=dev)
    cnt = torch.empty(N, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _launch.attention_topk(graph, val_slot_order, val_slot_order.size(1), k, eid, val, cnt)
    return eid, val, cnt


def _bwd_edges_src(g: CSRGraph, sched: Schedule, r0: int, h, s_src, nstate, grad_out, D, S, dz, heads, channels,
                   mode, slope, p, seed, seed_buf=None, edge_term=None):
    """Pass B over the source rows of ``sched`` (row ids relative to r0; edge slots and
    destination rows absolute) into D, S[:, :H] and dz -- dz in CSC order (dz_slot NULL: one
    contiguous store per edge instead of a 4-B scatter to its CSR slot)."""
    _launch.bwd_edges(sched, g.row, g.csc_eid, None, g.n_edges, r0, h, s_src, nstate, grad_out, heads, channels, mode,
                      slope, p, seed, seed_buf, D, S, dz, edge_term)


def _bwd_dst_sum(g: CSRGraph, dz, S, heads):
    _launch.bwd_dst_sum(g.fwd_sched, g.n_nodes, g.n_edges, heads, dz, _csr2csc(g) if g.n_edges else None,
                        S[:, heads:], csc=True)


def _bwd_edges_dst(g: CSRGraph, h, s_src, nstate, grad_out, D, S, heads, channels, mode, slope, p, seed,
                   seed_buf=None, edge_term=None):
    """Pass B into D [N, HC] (dh_msg) and S[:, :H] (ds_src); the destination sum into
    S[:, H:2H] (ds_dst).  S [N, 2H] is compact (its scattered per-node writes stay in L2)
    and D keeps whole 512-B rows for the GEMMs that read it.  Returns dz [E, H] (CSC order)."""
    dz = torch.empty(max(g.n_edges, 1) * heads, dtype=torch.float32, device=h.device)
    _bwd_edges_src(g, g.bwd_sched, 0, h, s_src, nstate, grad_out, D, S, dz, heads, channels, mode, slope, p, seed,
                   seed_buf, edge_term)
    _bwd_dst_sum(g, dz, S, heads)
    return dz


# ---------------------------------------------------------------------------
# weight gradients on a side stream
# ---------------------------------------------------------------------------
# A layer's dW = D^T x (+ S^T x) is independent of everything the backward does after it
# (dx, the next layer's edge passes), so it can run on a second HIP stream, overlapping the
# memory-bound edge kernels of the layer below.  Off by default (PPGAT_ASYNC_WGRAD=1 turns it
# on): at config 2 the persistent GEMM grid holds whole CUs the edge kernels then lack, and
# the step measured 2.47 ms against 2.42 ms in order (profiles/r01/v10_async_wgrad_bench.log).
# The main stream waits for it
# in a callback queued on the autograd engine, which runs once the whole backward pass has
# been enqueued -- before anything (optimizer, host reads) can consume the gradients.  Only
# used when the parameters' .grad are None and carry no hooks: accumulating into an existing
# .grad, or a hook, would read the gradient on the main stream before it exists.
_SIDE_STREAMS = {}
_PENDING_JOINS = []


def _fused_dxw_enabled() -> bool:
    """dx and the weight-gradient products in one pass (ppgat_project_bwd_fused); PPGAT_FUSED_DXW=0
    selects the two-kernel path (ppgat_project_bwd_input + ppgat_gemm_tn), e.g. to compare
    against the side-stream weight gradients bit for bit."""
    return os.environ.get("PPGAT_FUSED_DXW", "1") != "0"


def _async_wgrad_enabled() -> bool:
    return os.environ.get("PPGAT_ASYNC_WGRAD", "0") == "1"


def _grad_free(params) -> bool:
    for p in params:
        if p is None:
            continue
        if p.grad is not None or getattr(p, "_backward_hooks", None) or \
                getattr(p, "_post_accumulate_grad_hooks", None):
            return False
    return True


def _join_side_streams():
    while _PENDING_JOINS:
        main, ev = _PENDING_JOINS.pop()
        main.wait_event(ev)


def _side_stream(dev) -> torch.cuda.Stream:
    s = _SIDE_STREAMS.get(dev.index)
    if s is None:
        s = torch.cuda.Stream(device=dev)
        _SIDE_STREAMS[dev.index] = s
    return s


def _run_on_side(dev, inputs, fn):
    """fn() on the side stream after the main stream's work so far; returns fn's tensors,
    registered for use on the main stream, with the join queued on the autograd engine."""
    main = torch.cuda.current_stream(dev)
    side = _side_stream(dev)
    side.wait_stream(main)
    for t in inputs:
        if t is not None and t.numel() > 0:
            t.record_stream(side)
    with torch.cuda.stream(side):
        outs = fn()
    for t in outs:
        if t is not None:
            t.record_stream(main)
    ev = torch.cuda.Event()
    ev.record(side)
    if not _PENDING_JOINS:
        torch.autograd.Variable._execution_engine.queue_callback(_join_side_streams)
    _PENDING_JOINS.append((main, ev))
    return outs


def _producer_fusion_enabled() -> bool:
    """The producer layer's backward prologue inside this layer's dx kernel
    (ppgat_project_bwd_fused_producer); PPGAT_PRODUCER_PROLOGUE=0 runs it separately."""
    return _fused_dxw_enabled() and os.environ.get("PPGAT_PRODUCER_PROLOGUE", "1") != "0"


def _producer_of(x: torch.Tensor, N: int, C: int = 128):
    """The backward node of the GATLayer whose output x is -- nothing in between, x unmodified
    since -- when that layer (heads = 1, no replicated rows) can hand its backward prologue to
    the consumer's backward (its dx kernel, or the loss backward); else None."""
    node = x.grad_fn
    if node is None or not isinstance(node, GATLayer._backward_cls):
        return None
    if getattr(node, "pro_state", None) is None or x.dim() != 2 or x.size(0) != N or x.size(1) != C:
        return None
    if getattr(node, "out_version", None) != x._version:
        return None
    return node


class GATLayer(torch.autograd.Function):
    """One whole GAT layer x -> out with the projection inside:
    forward  h = x W^T with the node scores fused (ppgat_project; BLAS + ppgat_node_scores
             outside the fused shapes), then the fused softmax-aggregate;
    backward prologue, pass B and the destination sum write D = dh_msg [N, HC] and the
             compact S = [ds_src | ds_dst] [N, 2H]; dx = D W + S [A_src; A_dst]
             (ppgat_project_bwd_input: the attention terms as a rank-2 epilogue; BLAS outside
             the fused shapes), D^T x and S^T x (ppgat_gemm_tn with V) and
             ppgat_weight_grads give dW and datt.
    ``x_items`` (optional): the input rows [x.size(0), N) as a second tensor, so the model's
    node features cat(user_emb, item_proj(feats)) are never concatenated."""

    @staticmethod
    def forward(ctx, x, weight, att_src, att_dst, bias, graph: CSRGraph, heads: int, channels: int, mode: int,
                slope: float, dropout_p: float, seed: int, x_items=None, rep=None, edge_v=None, edge_staged=None):
        x_arg = x
        x = x.contiguous()
        x_items = x_items.contiguous() if x_items is not None else None
        W = weight.detach().contiguous()
        a_s = att_src.detach().reshape(heads, channels).contiguous()
        a_d = att_dst.detach().reshape(heads, channels).contiguous()
        b = bias.detach().contiguous() if bias is not None else None
        K = x.size(1)
        had_items = x_items is not None
        split = x.size(0)
        fused = heads == 1 and project_supported(K, heads * channels) and (x_items is None or x_items.size(1) == K)
        if fused:
            h, s_src, s_dst = project(x, W, att_src=a_s, att_dst=a_d, x_items=x_items)
            s_src, s_dst = s_src.view(-1, 1), s_dst.view(-1, 1)
        else:
            if x_items is not None:
                x = torch.cat([x, x_items], 0)
                x_items = None
            h = mm_nn(x, W, 1, heads * channels)  # ppgat_gemm_nn (zero-padded where the shape needs it)
            s_src, s_dst = node_scores(h, a_s, a_d, heads, channels)
        need = any(ctx.needs_input_grad[:5]) or (had_items and ctx.needs_input_grad[12])
        t_csr = t_csc = None
        if edge_v is not None:
            # edge features: the per-slot logit terms of this step, in both slot orders when a backward follows
            # a no-grad forward (eval, export) allocates nothing for a backward: needs_input_grad
            # does not know about the grad mode, so gat_layer passes it along
            need = (need or ctx.needs_input_grad[14]) and edge_staged[2]
            ev = edge_v.detach().reshape(heads, -1).contiguous()
            t_csr, t_csc = edge_terms(graph, edge_staged[:2], ev, heads, want_csc=need)
        else:
            _tap_kinks(graph.rowptr, graph.col, graph.csr_eid, s_src, s_dst, heads)
        ctx.seed_buf = seed_buffer(dropout_p, x.device) if need else None
        want_agg = (need or rep is not None) and heads > 1
        if rep is not None and graph.fwd_split is not None and rep.async_capable():
            # replicated item rows over RCCL: the item destinations first, their merge on the
            # communication stream, the user destinations meanwhile on this one
            RU, sched_u, sched_i = graph.fwd_split
            N = graph.n_nodes
            _require(h.size(0) == N, f"x has {h.size(0)} rows but the graph has {N} nodes")
            out, m, inv_l, agg = _fwd_outputs(N, heads, channels, want_agg, x.device)
            fa = (h, s_src, s_dst, b, heads, channels, mode, slope, dropout_p, seed, ctx.seed_buf, out, m, inv_l, agg)
            _fwd_rows(graph, sched_i, RU, N - RU, *fa)
            pending = rep.merge_fwd_async(out, m, inv_l, agg, b, heads, channels)
            _fwd_rows(graph, sched_u, 0, RU, *fa)
            rep.wait(pending)
        else:
            out, m, inv_l, agg = gat_fwd(graph, h, s_src, s_dst, b, heads, channels, mode, slope, dropout_p, seed,
                                         want_agg=want_agg, seed_buf=ctx.seed_buf, edge_term=t_csr)
            if rep is not None:  # replicated item rows (dist.py): merge their softmax over the ranks
                rep.merge_fwd(out, m, inv_l, agg, b, heads, channels)
        if need:
            empty = torch.empty(0, device=x.device)
            ctx.save_for_backward(x, x_items if x_items is not None else empty, W, h, a_s, a_d, s_src, s_dst, out, m,
                                  inv_l, agg if agg is not None else empty, b if b is not None else empty,
                                  t_csc if t_csc is not None else empty)
        ctx.edge = (edge_staged[1], tuple(edge_v.shape)) if edge_v is not None else None
        ctx.graph = graph
        ctx.rep = rep
        ctx.params = (weight, att_src, att_dst)
        ctx.meta = (heads, channels, mode, slope, dropout_p, seed, bias is not None, agg is not None, fused,
                    x_items is not None, had_items, split)
        ctx.att_shapes = (att_src.shape, att_dst.shape)
        # x straight from another heads = 1 layer (the stacked convs, train_gat_pyg.py:86-87): this
        # layer's dx kernel also does that layer's backward prologue (_producer_of)
        ctx.producer = _producer_of(x_arg, N=h.size(0)) if (need and fused and rep is None and x_items is None
                                                            and _producer_fusion_enabled()) else None
        ctx.pro_state = (b, s_dst, m, inv_l) if (need and heads == 1 and rep is None and agg is None) else None
        ctx.pro_result = None
        ctx.out_version = out._version
        return out

    @staticmethod
    def backward(ctx, g_out):
        x, xi, W, h, a_s, a_d, s_src, s_dst, out, m, inv_l, agg, b, t_csc = ctx.saved_tensors
        heads, C, mode, slope, p, seed, has_bias, has_agg, fused, seg, had_items, split = ctx.meta
        g = ctx.graph
        et = t_csc if ctx.edge is not None else None
        dev = x.device
        g_arg = g_out
        g_out = g_out.contiguous()
        N = g.n_nodes
        K = x.size(1)
        HC = heads * C
        rep = ctx.rep
        # replicated items over RCCL on a bipartite graph: the item rows' all_reduce runs on the
        # communication stream while the item sources' edge pass (user destinations only) runs
        overlap = rep is not None and g.bwd_split is not None and rep.async_capable()
        pending = None
        if rep is not None:  # item rows of grad_out: per-rank partial sums -> the full gradient
            if overlap:
                pending = rep.reduce_grad_async(g_out)
            else:
                rep.reduce_grad(g_out)
        # prologue: packed per-node state (+ dbias)
        want_db = has_bias and ctx.needs_input_grad[4]
        nstate = torch.empty(N, heads, 4, dtype=torch.float32, device=dev)
        dbias = torch.empty(C, dtype=torch.float32, device=dev) if want_db else None

        def prologue(r0, r1, db):
            _launch.bwd_prologue(r0, r1 - r0, g_out, out, agg if has_agg else None, b if has_bias else None, s_dst, m,
                                 inv_l, heads, C, mode, nstate, db)

        D = torch.empty(N, HC, dtype=torch.float32, device=dev)
        S = torch.empty(N, 2 * heads, dtype=torch.float32, device=dev)
        # the hand-off applies only to the very tensor the consumer produced (the object, not an
        # address a later allocation could reuse), unmodified since; a stale result is dropped here
        pre, ctx.pro_result = ctx.pro_result, None
        if (rep is None and pre is not None and pre[0]() is g_arg and pre[1] == g_arg._version
                and (not want_db or pre[3] is not None)):
            # the consumer layer's dx kernel already did this prologue (ppgat_project_bwd_fused_producer)
            nstate = pre[2]
            dbias = pre[3] if want_db else None
            dz = _bwd_edges_dst(g, h, s_src, nstate, g_out, D, S, heads, C, mode, slope, p, seed, ctx.seed_buf, et)
        elif rep is None:
            prologue(0, N, dbias)
            dz = _bwd_edges_dst(g, h, s_src, nstate, g_out, D, S, heads, C, mode, slope, p, seed, ctx.seed_buf, et)
        else:  # the replicated item rows enter dbias on one rank only
            RU = rep.RU
            db_i = torch.empty(C, dtype=torch.float32, device=dev) if (want_db and rep.rank == 0) else None
            prologue(0, RU, dbias)
            if overlap:
                RUs, sched_u, sched_i = g.bwd_split
                dz = torch.empty(max(g.n_edges, 1) * heads, dtype=torch.float32, device=dev)
                _bwd_edges_src(g, sched_i, RU, h, s_src, nstate, g_out, D, S, dz, heads, C, mode, slope, p, seed,
                               ctx.seed_buf)
                rep.wait(pending)
                prologue(RU, N, db_i)
                _bwd_edges_src(g, sched_u, 0, h, s_src, nstate, g_out, D, S, dz, heads, C, mode, slope, p, seed,
                               ctx.seed_buf)
                _bwd_dst_sum(g, dz, S, heads)
            else:
                prologue(RU, N, db_i)
                _bwd_edges_dst(g, h, s_src, nstate, g_out, D, S, heads, C, mode, slope, p, seed, ctx.seed_buf)
            if db_i is not None:
                dbias = dbias + db_i
        dv = None
        if ctx.edge is not None and ctx.needs_input_grad[14]:
            # dv[h, d] = sum_k dz[k, h] attr_csc[k, d]: the caller's autograd turns it into
            # the lin_edge.weight and att_edge gradients
            attr_csc, v_shape = ctx.edge
            dv = torch.empty(heads, attr_csc.size(1), dtype=torch.float32, device=dev)
            _launch.edge_dv(dz, attr_csc, g.n_edges, heads, attr_csc.size(1), dv)
            dv = dv.view(v_shape)
        need_dx = ctx.needs_input_grad[0] or (had_items and ctx.needs_input_grad[12])
        dx = None
        if (heads == 1 and HC == K and _launch.project_bwd_fused_supported(K) and _fused_dxw_enabled()
                and not (_async_wgrad_enabled() and _grad_free(ctx.params))):
            # dx and D^T x, S^T x in one pass over D and x (ppgat_project_bwd_fused)
            dx = torch.empty(N, K, dtype=torch.float32, device=dev) if need_dx else None
            G = torch.empty(HC, K, dtype=torch.float32, device=dev)
            GV = torch.empty(2, K, dtype=torch.float32, device=dev)
            ws, nbytes = _launch.project_bwd_fused_workspace(N, dev)
            x0, x1, sp = (x, xi, split) if seg else (x, None, N)
            if seg and split == 0:  # no user rows: every row from the item segment
                x0, x1, sp = xi, None, N
            prod = ctx.producer
            if prod is not None and dx is not None and prod.pro_state is not None:
                # also the producer layer's prologue: its nstate and dbias from dx (= its grad_out)
                pb, ps_dst, pm, pinv_l = prod.pro_state
                p_nstate = torch.empty(N, 1, 4, dtype=torch.float32, device=dev)
                p_dbias = torch.empty(K, dtype=torch.float32, device=dev) if pb is not None else None
                _launch.project_bwd_fused(D, S, x0, x1, sp, N, W, a_s, a_d, dx, G, GV, ws, nbytes,
                                          producer=(pb, ps_dst, pm, pinv_l, p_nstate, p_dbias))
                prod.pro_result = (weakref.ref(dx), dx._version, p_nstate, p_dbias)
            else:
                _launch.project_bwd_fused(D, S, x0, x1, sp, N, W, a_s, a_d, dx, G, GV, ws, nbytes)
            dW, datt_src, datt_dst = weight_grads(G, GV, W, a_s, a_d, heads, C)
            dx_u = dx[:split] if (dx is not None and had_items) else dx
            dx_i = dx[split:] if (dx is not None and had_items) else None
            return (dx_u, dW, datt_src.view(ctx.att_shapes[0]), datt_dst.view(ctx.att_shapes[1]), dbias,
                    None, None, None, None, None, None, None, dx_i, None, dv, None)
        if need_dx:
            if heads == 1 and project_supported(HC, K):  # reduction over HC, K output columns
                dx = torch.empty(N, K, dtype=torch.float32, device=dev)
                _launch.project_bwd_input(D, N, W, a_s, a_d, S, dx)
            else:
                # dx = D W + S [A_src; A_dst] with A_v[hd] = sum_c att_v[hd, c] W[hd*C + c, :]:
                # ppgat_gemm_nn, then the rank-2H attention terms in place (ppgat_rows_rank_update)
                dx = mm_nn(D, W, 0, K)
                if K % 4 == 0:
                    rank_update_(dx, S, att_proj(W, a_s, a_d, heads, C))
                else:  # odd widths: the rank-2H terms through the padded GEMM as well
                    dx += mm_nn(S, att_proj(W, a_s, a_d, heads, C), 0, K)
        def wgrad():
            G, _, GV = gemm_tn(D, x, V=S, B_items=xi if seg else None)
            return weight_grads(G, GV, W, a_s, a_d, heads, C)

        if _async_wgrad_enabled() and _grad_free(ctx.params):
            dW, datt_src, datt_dst = _run_on_side(dev, (D, S, x, xi, W, a_s, a_d), wgrad)
        else:
            dW, datt_src, datt_dst = wgrad()
        dx_u = dx[:split] if (dx is not None and had_items) else dx
        dx_i = dx[split:] if (dx is not None and had_items) else None
        return (dx_u, dW, datt_src.view(ctx.att_shapes[0]), datt_dst.view(ctx.att_shapes[1]), dbias,
                None, None, None, None, None, None, None, dx_i, None, dv, None)


def gat_layer(x, weight, att_src, att_dst, bias, graph, heads, channels, mode, slope, dropout_p=0.0, seed=0,
              x_items=None, rep=None, edge_v=None, edge_attr=None):
    """x [N, F] -> out [N, C]: lin + the fused GAT aggregation, with the fused backward.
    With ``x_items``, the input rows are cat(x, x_items) (never materialised on the fused path).
    With ``edge_v`` [H, D] (differentiable) and ``edge_attr`` [E, D] (an input; staged once per
    graph, stage_edge_attr), the logit of edge k gains <edge_attr[k], edge_v[h]> -- GATConv's
    edge_dim term with lin_edge and att_edge collapsed to edge_v; transform-then-aggregate only."""
    _require(x.is_cuda, "gat_layer: ppgat runs on ROCm devices only; there is no CPU path")
    if x.dtype != torch.float32 or x.dim() != 2:
        raise NotImplementedError("ppgat gat_layer: fp32 2-D input only")
    if x_items is not None:
        _require(x_items.is_cuda and x_items.dtype == torch.float32 and x_items.dim() == 2
                 and x_items.size(1) == x.size(1), "gat_layer: x_items must match x in dtype/device/width")
    if (edge_v is None) != (edge_attr is None):
        raise ValueError("gat_layer: edge_v and edge_attr go together")
    if edge_v is not None:
        if rep is not None:
            raise NotImplementedError("gat_layer: edge features on the replicated (sharded) layer are not implemented")
        if mode != _lib.MODE_PYG:
            raise NotImplementedError("gat_layer: edge features are GATConv's (PyG mode) only")
        staged = stage_edge_attr(graph, edge_attr)
        D = staged[0].size(1)
        if not (isinstance(edge_v, torch.Tensor) and edge_v.dtype == torch.float32 and edge_v.device == x.device
                and edge_v.numel() == heads * D):
            raise ValueError(f"edge_v: expected an fp32 [{heads}, {D}] tensor on {x.device}")
        return GATLayer.apply(x, weight, att_src, att_dst, bias, graph, heads, channels, mode, slope, dropout_p, seed,
                              x_items, None, edge_v, staged + (torch.is_grad_enabled(),))
    if (mode == _lib.MODE_PYG and heads > 1 and heads * channels > x.size(1) and rep is None
            and xgat_supported(x.size(1), heads, channels)):
        # multi-head layers wider than their input: aggregate x, then transform (config 5)
        xx = join_rows(x, x_items) if x_items is not None else x
        return gat_layer_x(xx, weight, att_src, att_dst, bias, XViews.of_graph(graph), heads, channels, slope,
                           dropout_p, seed)
    return GATLayer.apply(x, weight, att_src, att_dst, bias, graph, heads, channels, mode, slope, dropout_p, seed,
                          x_items, rep)


def gat_layer_attention(x, weight, att_src, att_dst, graph, heads, channels, mode, slope, x_items=None, edge_v=None,
                        edge_attr=None, order: str = "edge") -> torch.Tensor:
    """alpha [E, H] of gat_layer(x, ...) on the same arguments, before the dropout mask: a
    no-grad forward of its own over the unfused primitives (projection and node scores, the
    edge terms, gat_fwd -- xgat_forward where gat_layer takes the aggregate-then-transform
    path) whose scores and softmax state go to attention_weights.  Costs a second forward."""
    _require(x.is_cuda, "gat_layer_attention: ppgat runs on ROCm devices only; there is no CPU path")
    if x.dtype != torch.float32 or x.dim() != 2:
        raise NotImplementedError("ppgat gat_layer_attention: fp32 2-D input only")
    if (edge_v is None) != (edge_attr is None):
        raise ValueError("gat_layer_attention: edge_v and edge_attr go together")
    if edge_v is not None and mode != _lib.MODE_PYG:
        raise NotImplementedError("gat_layer_attention: edge features are GATConv's (PyG mode) only")
    heads, channels = int(heads), int(channels)
    with torch.no_grad(), torch.cuda.device(x.device):
        x = x.detach().contiguous()
        x_items = x_items.detach().contiguous() if x_items is not None else None
        W = weight.detach().contiguous()
        a_s = att_src.detach().reshape(heads, channels).contiguous()
        a_d = att_dst.detach().reshape(heads, channels).contiguous()
        K = x.size(1)
        if (edge_v is None and mode == _lib.MODE_PYG and heads > 1 and heads * channels > K
                and xgat_supported(K, heads, channels)):
            xx = join_rows(x, x_items) if x_items is not None else x
            # the instrumentation records the layer's own forward only
            tap, ops_graph.KINK_TAP = ops_graph.KINK_TAP, None
            try:
                _, st = xgat_forward(xx, W, a_s, a_d, None, XViews.of_graph(graph), heads, channels, slope, 0.0, 0,
                                     keep_agg=False)
            finally:
                ops_graph.KINK_TAP = tap
            return attention_weights(graph, st["s_src"], st["s_dst"], st["m"], st["inv_l"], heads, mode, slope,
                                     order=order)
        if heads == 1 and project_supported(K, channels) and (x_items is None or x_items.size(1) == K):
            h, s_src, s_dst = project(x, W, att_src=a_s, att_dst=a_d, x_items=x_items)
            s_src, s_dst = s_src.view(-1, 1), s_dst.view(-1, 1)
        else:
            if x_items is not None:
                x = torch.cat([x, x_items], 0)
            h = mm_nn(x, W, 1, heads * channels)
            s_src, s_dst = node_scores(h, a_s, a_d, heads, channels)
        t_csr = None
        if edge_v is not None:
            staged = stage_edge_attr(graph, edge_attr)
            t_csr, _ = edge_terms(graph, staged, edge_v.detach().reshape(heads, -1).contiguous(), heads, want_csc=False)
        _, m, inv_l, _ = gat_fwd(graph, h, s_src, s_dst, None, heads, channels, mode, slope, 0.0, 0, want_agg=False,
                                 edge_term=t_csr)
        return attention_weights(graph, s_src, s_dst, m, inv_l, heads, mode, slope, edge_term=t_csr, order=order)


def gatv2_layer_attention(xl, xr, att, graph, heads, channels, slope, order: str = "edge") -> torch.Tensor:
    """alpha [E, H] of gatv2_aggregate(xl, xr, att, ...) before the dropout mask: a no-grad
    aggregate of its own (_launch.dynatt_fwd) whose state goes to gatv2_attention_weights."""
    heads, channels = int(heads), int(channels)
    _gatv2_require_shape(heads, channels)
    _require(xl.is_cuda, "gatv2_layer_attention: ppgat runs on ROCm devices only; there is no CPU path")
    with torch.no_grad(), torch.cuda.device(xl.device):
        shared = xr is xl or (xr.data_ptr() == xl.data_ptr() and xr.stride() == xl.stride())
        xl = xl.detach().contiguous()
        xr = xl if shared else xr.detach().contiguous()
        att_c = att.detach().contiguous().view(heads, channels)
        out, m, inv_l, _ = _fwd_outputs(graph.n_nodes, heads, channels, False, xl.device)
        _launch.dynatt_fwd(graph, xl, xr, att_c, None, heads, channels, slope, 0.0, 0, None, out, m, inv_l)
        return gatv2_attention_weights(graph, xl, xr, att_c, m, inv_l, heads, channels, slope, order=order)
