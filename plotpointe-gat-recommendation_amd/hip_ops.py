"""Torch-facing wrappers over the C ABI (include/ppgat.h): the import surface.

PyTorch is plumbing here: it owns device memory (caching allocator), the current
HIP stream and autograd.  All message-passing arithmetic runs in libppgat.so.
Every function raises if the library is absent or a tensor is not a contiguous
fp32/int64 ROCm tensor of the expected shape -- there is no CPU fallback.

The code lives by subject in ops_graph (checks, CSR / CSC views, schedules, edge-attribute
staging), ops_gemm (projections and GEMMs), ops_xgat (the aggregate-then-transform layer),
ops_gat (the GAT / GATv2 layers and attention read-backs) and ops_loss (the losses), imported
in that order, each from the ones before it; the kernels themselves are launched from
_launch.py.  This module re-exports their functions, classes and constants, and holds
``HipStages``.  Module state that is rebound or counted (ops_graph.KINK_TAP and
EDGE_STAGE_COUNT, ops_gat._PENDING_JOINS and _SIDE_STREAMS, ops_gemm._CONST_BOUNDS) is not
re-exported: a copy here would be stale.  Read and set it on its own module, and patch a
function on the module whose code looks it up.
"""
from __future__ import annotations

import torch

from . import _launch
from .ops_gat import (GATAggregate, GATLayer, GATv2Aggregate, _ORDERS, _async_wgrad_enabled,  # noqa: F401
                      _attention_out, _bwd_dst_sum, _bwd_edges_dst, _bwd_edges_src, _check_state, _fused_dxw_enabled,
                      _fwd_outputs, _fwd_rows, _gatv2_require_shape, _grad_free, _join_side_streams,
                      _producer_fusion_enabled, _producer_of, _run_on_side, _side_stream, attention_topk,
                      attention_weights, gat_aggregate, gat_bwd, gat_fwd, gat_layer, gat_layer_attention,
                      gatv2_aggregate, gatv2_attention_weights, gatv2_layer_attention, gatv2_supported, node_scores)
from .ops_gemm import (_EmbeddingRows, _JoinRows, _Linear, _aligned_rows, _const_colmax, _pad_cols4,  # noqa: F401
                       att_proj, colmax_abs, colsum, embedding_rows, gemm_nn, gemm_nn_supported, gemm_tn, gemm_tn_big,
                       gemm_tn_big_supported, join_rows, linear, mm_nn, project, project_supported, rank_update_,
                       rows_adjacent, weight_grads)
from .ops_graph import (EDGE_MAX_DIM, MAX_EDGES_PER_ITEM, CSRGraph, Schedule, _check_dev, _check_rows,  # noqa: F401
                        _csr2csc, _GraphCache, _require, _tap_kinks, check_edge_attr, csr_build, debug_validate_graph,
                        edge_terms, graph_cache, schedule_build, seed_buffer, stage_edge_attr)
from .ops_loss import (LOSS_KINDS, BprPrepared, _BadIndex, _BPRLoss, _check_correction, _SharedSoftmaxLoss,  # noqa: F401
                       _SoftmaxLoss, _track_correction, bpr_loss, bpr_loss_mapped, bpr_prepare, check_bpr_indices,
                       shared_softmax_loss, shared_softmax_loss_corrected, softmax_loss)
from .ops_xgat import (GATLayerX, XPhase, XViews, _xgat_backward_deferred_d, _xgat_bytes, _xgat_dst_sum,  # noqa: F401
                       _xgat_gather_mode, _xgat_keep_agg, _xgat_weight_grads, _xgat_weight_grads_from_G, gat_layer_x,
                       xgat_att_proj, xgat_backward, xgat_forward, xgat_scores_rows, xgat_supported)


# ---------------------------------------------------------------------------
# staged kernels for the row-sharded path (dist.py); one object so tests can swap in
# a CPU restatement of the same stages
# ---------------------------------------------------------------------------
class HipStages:
    """The GAT layer as the stages of include/ppgat.h, over explicit (possibly sliced)
    CSR/CSC views: see dist.LocalView for the fields used."""

    def linear(self, x, weight, bias, out=None):
        return linear(x, weight, bias, out=out)

    def seed_buffer(self, p, device):
        return seed_buffer(p, device)

    def supports_x(self, conv) -> bool:
        """Whether the aggregate-then-transform kernels take this layer (dist.HaloPyGGAT)."""
        return conv.heads > 1 and xgat_supported(conv.in_channels, conv.heads, conv.out_channels)

    def gather_rows(self, t, idx):
        """t[idx] (the all_to_all send buffer) through ppgat_rows_gather."""
        _check_dev("rows", t, torch.float32)
        _check_dev("idx", idx, torch.int64, t.device)
        out = torch.empty((idx.numel(),) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
        cols = t[0].numel() if t.size(0) else (out[0].numel() if idx.numel() else 0)
        _launch.rows_gather(t, idx, cols, out)
        return out

    def return_add(self, dst, ret, ptr, pos):
        """dst[o] += ret[pos[ptr[o]:ptr[o+1]]] in order (ppgat_rows_return_add), in place."""
        _check_dev("dst", dst, torch.float32)
        cols = dst[0].numel() if dst.size(0) else 0
        _launch.rows_return_add(dst, ret, ptr, pos, cols)
        return dst

    bpr_grad_rows = True  # bpr() takes grad_rows (dist.halo_bpr_loss)

    def bpr(self, Z, n_users, n_items, row_map, u, i, j, loss, grad_rows: int = 0, grad_buf=None):
        return bpr_loss_mapped(Z, n_users, n_items, row_map, u, i, j, loss, grad_rows=grad_rows, grad_buf=grad_buf)

    def scores(self, h, att_src, att_dst, heads, channels):
        return node_scores(h, att_src, att_dst, heads, channels)

    def fwd(self, v, h_full, s_src_full, s_dst, bias, heads, channels, mode, slope, p, seed, want_agg, seed_buf=None):
        dev = h_full.device
        _tap_kinks(v.rowptr, v.col, v.csr_eid, s_src_full, s_dst, heads)
        R = v.n_rows
        out, m, inv_l, agg = _fwd_outputs(R, heads, channels, want_agg, dev)
        _launch.fwd(v.fwd_sched, v.col, v.csr_eid, v.n_fwd_edges, 0, R, h_full, s_src_full, s_dst, bias, heads,
                    channels, mode, slope, p, seed, seed_buf, out, m, inv_l, agg)
        return out, m, inv_l, agg

    def bwd_prologue(self, grad_out, out, agg, bias, s_dst, m, inv_l, heads, channels, mode, want_bias_grad):
        dev = grad_out.device
        R = grad_out.size(0)
        nstate = torch.empty(R, heads, 4, dtype=torch.float32, device=dev)
        dbias = torch.empty(channels, dtype=torch.float32, device=dev) if want_bias_grad else None
        _launch.bwd_prologue(0, R, grad_out, out, agg, bias, s_dst, m, inv_l, heads, channels, mode, nstate, dbias)
        return nstate, dbias

    def bwd_edges(self, v, h, s_src, nstate_full, grad_out_full, dz, heads, channels, mode, slope, p, seed,
                  seed_buf=None):
        dev = h.device
        R = v.n_rows
        grad_h = torch.empty(R, heads * channels, dtype=torch.float32, device=dev)
        ds_src = torch.empty(R, heads, dtype=torch.float32, device=dev)
        _launch.bwd_edges(v.bwd_sched, v.row, v.csc_eid, v.dz_slot, v.n_bwd_edges, 0, h, s_src, nstate_full,
                          grad_out_full, heads, channels, mode, slope, p, seed, seed_buf, grad_h, ds_src, dz)
        return grad_h, ds_src

    def bwd_epilogue(self, v, h, att_src, att_dst, ds_src, dz, grad_h, heads, channels):
        dev = h.device
        R = v.n_rows
        datt_src = torch.empty(heads, channels, dtype=torch.float32, device=dev)
        datt_dst = torch.empty(heads, channels, dtype=torch.float32, device=dev)
        _launch.bwd_epilogue(v.rowptr, R, heads, channels, h, att_src, att_dst, ds_src, dz, grad_h, datt_src, datt_dst)
        return datt_src, datt_dst
