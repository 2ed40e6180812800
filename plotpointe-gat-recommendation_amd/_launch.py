"""The GAT layers' kernel launches (include/ppgat.h), one function per ABI entry.

hip_ops.py and dist.py decide what runs, in which order and into which tensors; here those
tensors are handed to libppgat.so on the current stream: workspace, schedule struct (a fresh one
per call), NULL edge arrays of an edge-less view, 64-bit seed, row offsets (``r0`` / ``base``: a
row of the tensor, made an address and a leading dimension by _lib.row_ptr), return-code check.
"""
from __future__ import annotations

import ctypes

import torch

from ._lib import check, edge_ptrs, load, ptr, row_ptr, seed64, stream_handle, workspace


def _at(t, row: int = 0):
    return row_ptr(t, row)[0]


def _sched(sched, all_long: bool = False):
    cs = sched.cstruct()
    if all_long:  # hip_ops._xgat_dst_sum decides
        cs.n_long_items = -1
    return ctypes.byref(cs)


def _f32(n: int, dev):
    return torch.empty(n, dtype=torch.float32, device=dev)


def node_scores(h, att_src, att_dst, heads: int, channels: int, s_src, s_dst):
    check(load().ppgat_node_scores(ptr(h), ptr(att_src), ptr(att_dst), h.size(0), heads, channels, ptr(s_src),
                                   ptr(s_dst), stream_handle(h.device)), "node_scores")


def fwd(sched, col, csr_eid, n_edges: int, r0: int, n: int, h, s_src, s_dst, bias, heads: int, channels: int,
        mode: int, slope, p, seed, seed_buf, out, m, inv_l, agg, edge_term=None):
    """The destination rows [r0, r0 + n) of ``sched`` (row ids relative to r0; edge slots and
    source rows absolute): the destination-indexed tensors start at row r0.  ``edge_term`` [E, H]
    in CSR slot order: the edge-feature logit term (ppgat_edge_fwd)."""
    lib, dev = load(), h.device
    ws, nbytes = workspace(lib.ppgat_fwd_workspace_bytes, sched.n_hub_items, heads, channels, device=dev)
    tail = (n, n_edges, heads, channels, ptr(h), ptr(s_src), _at(s_dst, r0), ptr(bias), mode, float(slope), float(p),
            seed64(seed), ptr(seed_buf), _at(out, r0), _at(m, r0), _at(inv_l, r0), _at(agg, r0), ptr(ws), nbytes,
            stream_handle(dev))
    if edge_term is None:
        check(lib.ppgat_fwd(_sched(sched), *edge_ptrs(n_edges, col, csr_eid), *tail), "gat_fwd")
    else:
        check(lib.ppgat_edge_fwd(_sched(sched), *edge_ptrs(n_edges, col, csr_eid, edge_term), *tail), "edge_fwd")


def bwd_prologue(r0: int, n: int, grad_out, out, agg, bias, s_dst, m, inv_l, heads: int, channels: int, mode: int,
                 nstate, dbias):
    """The packed per-node state of the rows [r0, r0 + n) (and their dbias, when given)."""
    lib, dev = load(), grad_out.device
    part = _f32(max(int(lib.ppgat_bwd_partial_rows(n)), 1) * channels, dev) if dbias is not None else None
    check(lib.ppgat_bwd_prologue(_at(grad_out, r0), _at(out, r0), _at(agg, r0), ptr(bias), _at(s_dst, r0), _at(m, r0),
                                 _at(inv_l, r0), n, heads, channels, mode, _at(nstate, r0), ptr(dbias), ptr(part),
                                 stream_handle(dev)), "bwd_prologue")


def bwd_edges(sched, row, csc_eid, dz_slot, n_edges: int, r0: int, h, s_src, nstate, grad_out, heads: int,
              channels: int, mode: int, slope, p, seed, seed_buf, D, S, dz, edge_term=None):
    """Pass B over the source rows of ``sched`` (row ids relative to r0; edge slots and destination
    rows absolute): D and S from row r0 on, each with its own row stride; ``dz_slot`` None: dz in CSC order.
    ``edge_term`` [E, H] in CSC slot order: the edge-feature logit term (ppgat_edge_bwd_edges)."""
    lib, dev = load(), h.device
    ws, nbytes = workspace(lib.ppgat_fwd_workspace_bytes, sched.n_hub_items, heads, channels, device=dev)
    tail = (n_edges, heads, channels, _at(h, r0), _at(s_src, r0), ptr(nstate), ptr(grad_out), mode, float(slope),
            float(p), seed64(seed), ptr(seed_buf), *row_ptr(D, r0), *row_ptr(S, r0), ptr(dz), ptr(ws), nbytes,
            stream_handle(dev))
    if edge_term is None:
        check(lib.ppgat_bwd_edges(_sched(sched), *edge_ptrs(n_edges, row, csc_eid, dz_slot), *tail), "bwd_edges")
    else:
        check(lib.ppgat_edge_bwd_edges(_sched(sched), *edge_ptrs(n_edges, row, csc_eid, dz_slot, edge_term), *tail),
              "edge_bwd_edges")


def edge_attr_permute(edge_attr, slot_eid, n_edges: int, out):
    """out [E, D] = edge_attr[slot_eid] (the staging of an attribute tensor into a view's slot order)."""
    check(load().ppgat_edge_attr_permute(*edge_ptrs(n_edges, edge_attr, slot_eid), n_edges, edge_attr.size(1),
                                         ptr(out), stream_handle(out.device)), "edge_attr_permute")


def edge_terms(attr_csr, attr_csc, v, n_edges: int, heads: int, t_csr, t_csc):
    """t_csr (and t_csc, when given) [E, H] from the staged attribute tables and v [H, D]."""
    check(load().ppgat_edge_terms(*edge_ptrs(n_edges, attr_csr, attr_csc), ptr(v), n_edges, v.size(1), heads,
                                  ptr(t_csr), ptr(t_csc), stream_handle(v.device)), "edge_terms")


def edge_dv(dz, attr_csc, n_edges: int, heads: int, edge_dim: int, dv):
    """dv [H, D] = dz^T attr_csc over the CSC slots (ordered block partials, no atomics)."""
    lib, dev = load(), dv.device
    part = _f32(max(int(lib.ppgat_edge_dv_partial_rows(n_edges)), 1) * heads * edge_dim, dev)
    check(lib.ppgat_edge_dv(*edge_ptrs(n_edges, dz, attr_csc), n_edges, heads, edge_dim, ptr(dv), ptr(part),
                            stream_handle(dev)), "edge_dv")


def bwd_dst_sum(sched, n_dst: int, n_edges: int, heads: int, dz, csr2csc, out, csc: bool, all_long: bool = False):
    """Per-destination sums of dz into ``out`` [n_dst, heads] (a column view such as S[:, H:] is fine).
    ``csc``: dz lies in CSC order, read through csr2csc (ppgat_bwd_dst_sum_csc); else by CSR slot."""
    lib, dev = load(), dz.device
    dws = _f32(max(sched.n_hub_items * heads, 1), dev)
    tail = (*row_ptr(out), ptr(dws), dws.numel() * 4, stream_handle(dev))
    if csc:
        check(lib.ppgat_bwd_dst_sum_csc(_sched(sched, all_long), n_dst, n_edges, heads, ptr(dz),
                                        *edge_ptrs(n_edges, csr2csc), *tail), "bwd_dst_sum_csc")
    else:
        check(lib.ppgat_bwd_dst_sum(_sched(sched, all_long), n_dst, heads, ptr(dz), *tail), "bwd_dst_sum")


def bwd_epilogue(rowptr, n_rows: int, heads: int, channels: int, h, att_src, att_dst, ds_src, dz, grad_h, datt_src,
                 datt_dst):
    lib, dev = load(), h.device
    part = _f32(max(int(lib.ppgat_bwd_partial_rows(n_rows)), 1) * 2 * heads * channels, dev)
    check(lib.ppgat_bwd_epilogue(ptr(rowptr), n_rows, heads, channels, ptr(h), ptr(att_src), ptr(att_dst),
                                 ptr(ds_src), ptr(dz), ptr(grad_h), ptr(datt_src), ptr(datt_dst), ptr(part),
                                 stream_handle(dev)), "bwd_epilogue")


def rep_merge(stage: int, rowptr, r0: int, n: int, heads: int, channels: int, out, agg, bias, m, inv_l, mx, pack):
    """Stage 0 / 1 / 2 of the replicated rows' softmax merge over the rows [r0, r0 + n)."""
    check(load().ppgat_rep_merge(stage, _at(rowptr, r0), n, heads, channels, _at(out, r0), _at(agg, r0), ptr(bias),
                                 _at(m, r0), _at(inv_l, r0), ptr(mx), ptr(pack), stream_handle(out.device)),
          "rep_merge")


def rows_gather(t, idx, cols: int, out):
    check(load().ppgat_rows_gather(ptr(t), cols, ptr(idx), idx.numel(), cols, ptr(out), cols,
                                   stream_handle(t.device)), "rows_gather")


def rows_return_add(dst, ret, ret_ptr, pos, cols: int):
    check(load().ppgat_rows_return_add(ptr(dst), cols, ptr(ret) if ret.numel() else None, cols, ptr(ret_ptr),
                                       ptr(pos) if pos.numel() else None, dst.size(0), cols,
                                       stream_handle(dst.device)), "rows_return_add")


# the GATv2 dynamic-attention layer (ppgat_dynatt_*); ``g``: a hip_ops.CSRGraph
def dynatt_supported(heads: int, channels: int) -> bool:
    return bool(load().ppgat_dynatt_supported(int(heads), int(channels)))


def dynatt_workspace(g, heads: int, channels: int, backward: bool, dev):
    return workspace(load().ppgat_dynatt_workspace_bytes, g.n_nodes, g.fwd_sched.n_hub_items,
                     g.bwd_sched.n_hub_items, heads, channels, 1 if backward else 0, device=dev, floor=1)


def dynatt_fwd(g, xl, xr, att, bias, heads: int, channels: int, slope, p, seed, seed_buf, out, m, inv_l):
    lib, dev, E = load(), xl.device, g.n_edges
    ws, nbytes = dynatt_workspace(g, heads, channels, False, dev)
    check(lib.ppgat_dynatt_fwd(_sched(g.fwd_sched), *edge_ptrs(E, g.col, g.csr_eid), g.n_nodes, E, heads, channels,
                               ptr(xl), ptr(xr), ptr(att), ptr(bias), float(slope), float(p), seed64(seed),
                               ptr(seed_buf), ptr(out), ptr(m), ptr(inv_l), ptr(ws), nbytes, stream_handle(dev)),
          "gatv2_fwd")


def dynatt_bwd(g, xl, xr, att, m, inv_l, grad_out, heads: int, channels: int, slope, p, seed_buf, dxl, dxr, datt,
               dbias):
    lib, dev, E = load(), xl.device, g.n_edges
    ws, nbytes = dynatt_workspace(g, heads, channels, True, dev)
    check(lib.ppgat_dynatt_bwd(_sched(g.bwd_sched), _sched(g.fwd_sched), *edge_ptrs(E, g.row, g.csc_eid, g.col,
                                                                                    g.csr_eid),
                               g.n_nodes, E, heads, channels, ptr(xl), ptr(xr), ptr(att), ptr(m), ptr(inv_l),
                               ptr(grad_out), float(slope), float(p), ptr(seed_buf), ptr(dxl), ptr(dxr), ptr(datt),
                               ptr(dbias), ptr(ws), nbytes, stream_handle(dev)),
          "gatv2_bwd")


# attention weights from a forward's final state (``order`` 0: CSR slot order, 1: edge_index
# column order) and the per-destination selection; ``g``: a hip_ops.CSRGraph
def attention(g, s_src, s_dst, m, inv_l, heads: int, mode: int, slope, order: int, alpha, edge_term=None):
    E = g.n_edges
    check(load().ppgat_attention(_sched(g.fwd_sched), *edge_ptrs(E, g.col, g.csr_eid, edge_term), g.n_nodes, E,
                                 heads, ptr(s_src), ptr(s_dst), ptr(m), ptr(inv_l), mode, float(slope), order,
                                 ptr(alpha), stream_handle(alpha.device)), "attention")


def dynatt_attention(g, xl, xr, att, m, inv_l, heads: int, channels: int, slope, order: int, alpha):
    E = g.n_edges
    check(load().ppgat_dynatt_attention(_sched(g.fwd_sched), *edge_ptrs(E, g.col, g.csr_eid), g.n_nodes, E, heads,
                                        channels, ptr(xl), ptr(xr), ptr(att), ptr(m), ptr(inv_l), float(slope),
                                        order, ptr(alpha), stream_handle(alpha.device)), "gatv2_attention")


def attention_topk(g, val, heads: int, k: int, out_eid, out_val, out_cnt):
    E = g.n_edges
    check(load().ppgat_attention_topk(ptr(g.rowptr), *edge_ptrs(E, g.csr_eid, val), g.n_nodes, E, heads, k,
                                      ptr(out_eid), ptr(out_val), ptr(out_cnt), stream_handle(out_eid.device)),
          "attention_topk")


# fan-out neighbour sampling (ppgat_neighbor_*); ``g``: the parent hip_ops.CSRGraph.  The three
# run in this order on one stream and share ``ws`` (neighbor_workspace), untouched in between.
def neighbor_workspace(n_nodes: int, n_edges: int, dev):
    return workspace(load().ppgat_neighbor_sample_workspace_bytes, n_nodes, n_edges, device=dev, floor=1)


def neighbor_count(g, fanout: int, fanout_of, rowptr_s, info, ws, nbytes: int):
    """rowptr_s [N + 1] and info [2] int32 = (E', bad) for the caps ``fanout`` / ``fanout_of``."""
    check(load().ppgat_neighbor_count(ptr(g.rowptr), g.n_nodes, g.n_edges, int(fanout), ptr(fanout_of),
                                      ptr(rowptr_s), ptr(info), ptr(ws), nbytes, stream_handle(rowptr_s.device)),
          "neighbor_count")


def neighbor_sample(g, edge_index, seed, rowptr_s, n_kept: int, col_s, csr_eid_s, edge_index_s, eid, ws, nbytes: int):
    """The pick and the renumbering: the sampled CSR side, edge_index_s [2, E'] and eid [E'].
    ``g.csr2csc`` must be there (hip_ops.csr_build leaves it; hip_ops._csr2csc makes it)."""
    E = g.n_edges
    check(load().ppgat_neighbor_sample(ptr(g.rowptr), *edge_ptrs(E, g.col, g.csr_eid, g.csr2csc, edge_index), g.n_nodes,
                                       E,
                                       seed64(seed), ptr(rowptr_s),
                                       n_kept, *edge_ptrs(n_kept, col_s, csr_eid_s, edge_index_s, eid), ptr(ws), nbytes,
                                       stream_handle(rowptr_s.device)), "neighbor_sample")


def neighbor_derive(g, n_kept: int, colptr_s, row_s, csc_eid_s, csc2csr_s, csr2csc_s, ws, nbytes: int):
    """The sampled CSC side and the slot maps between the two."""
    E = g.n_edges
    check(load().ppgat_neighbor_derive(ptr(g.colptr), *edge_ptrs(E, g.row, g.csc_eid, g.csc2csr), g.n_nodes, E, n_kept,
                                       ptr(colptr_s), *edge_ptrs(n_kept, row_s, csc_eid_s, csc2csr_s, csr2csc_s),
                                       ptr(ws), nbytes, stream_handle(colptr_s.device)), "neighbor_derive")


# seed-subgraph sampling (ppgat_subgraph_*); ``g``: the parent hip_ops.CSRGraph.  seed, expand per
# hop, plan, then neighbor_count / _sample / _derive under the plan's cap table, then relabel: one
# stream, ``ws`` (subgraph_workspace) untouched in between.  ``info`` [4] int32.
def subgraph_workspace(n_nodes: int, dev):
    return workspace(load().ppgat_subgraph_workspace_bytes, n_nodes, device=dev, floor=1)


def subgraph_seed(seeds, n_nodes: int, info, ws, nbytes: int):
    T = seeds.numel()
    check(load().ppgat_subgraph_seed(ptr(seeds) if T else None, T, n_nodes, ptr(info), ptr(ws), nbytes,
                                     stream_handle(info.device)), "subgraph_seed")


def subgraph_expand(g, hop: int, fanout: int, fanout_of, seed, ws, nbytes: int):
    check(load().ppgat_subgraph_expand(ptr(g.rowptr), *edge_ptrs(g.n_edges, g.col), g.n_nodes, g.n_edges, int(hop),
                                       int(fanout), ptr(fanout_of), seed64(seed), ptr(ws), nbytes,
                                       stream_handle(g.rowptr.device)), "subgraph_expand")


def subgraph_plan(n_nodes: int, n_users: int, hops: int, fanout: int, fanout_of, cap, info, ws, nbytes: int):
    """cap [N] int32 (0 outside the expanded nodes) and info[0:2] = (N_s, n_users_s), info[3] = bad fanout_of."""
    check(load().ppgat_subgraph_plan(n_nodes, int(n_users), int(hops), int(fanout), ptr(fanout_of),
                                     ptr(cap) if n_nodes else None, ptr(info), ptr(ws), nbytes,
                                     stream_handle(info.device)), "subgraph_plan")


def subgraph_relabel(n_nodes: int, n_sub: int, n_kept: int, seeds, rowptr_p, colptr_p, n_id, depth, rowptr_s,
                     colptr_s, col_s, row_s, edge_index_s, seed_local, ws, nbytes: int):
    """The node side compacted, the edge side relabelled in place (col_s, row_s, edge_index_s)."""
    T = seeds.numel()
    check(load().ppgat_subgraph_relabel(n_nodes, n_sub, n_kept, ptr(seeds) if T else None, T, ptr(rowptr_p),
                                        ptr(colptr_p), *edge_ptrs(n_sub, n_id, depth), ptr(rowptr_s), ptr(colptr_s),
                                        *edge_ptrs(n_kept, col_s, row_s, edge_index_s),
                                        ptr(seed_local) if T else None, ptr(ws), nbytes,
                                        stream_handle(rowptr_s.device)), "subgraph_relabel")


# the aggregate-then-transform layer (ppgat_xgat_*); ``v``: a hip_ops.XViews
def xgat_weights(W, a_s, a_d, H: int, C: int, A=None, Wt=None, Wg=None):
    """Whichever of A [2, H, K] (needs a_s, a_d), Wt [H * K, C] and Wg [C, H * K] are given."""
    check(load().ppgat_xgat_weights(ptr(W), ptr(a_s), ptr(a_d), H, C, W.size(1), ptr(A), ptr(Wt), ptr(Wg),
                                    stream_handle(W.device)), "xgat_weights")


def xgat_scores(x, r0: int, n: int, A, s_src, s_dst=None):
    """s_src of the rows [r0, r0 + n) of x under A [2, H, K]; with ``s_dst`` (r0 = 0) theirs too."""
    px, ldx = row_ptr(x, r0)
    check(load().ppgat_xgat_scores(px, ldx, n, n if s_dst is not None else 0, x.size(1), A.size(1), ptr(A),
                                   _at(s_src, r0), ptr(s_dst), stream_handle(x.device)), "xgat_scores")


def xgat_fwd_colmax(sched, v, d0: int, nd: int, x, s_src, s_dst, slope, p, seed, seed_buf, agg, m, inv_l, xbits):
    """The destination rows [d0, d0 + nd) of ``sched`` (rows relative to d0); column maxima into xbits."""
    lib, dev, E = load(), x.device, v.n_edges
    K, H = x.size(1), s_src.size(1)
    ws, nbytes = workspace(lib.ppgat_xgat_fwd_workspace_bytes, sched.n_hub_items, H, K, device=dev)
    check(lib.ppgat_xgat_fwd_colmax(_sched(sched), *edge_ptrs(E, v.col, v.csr_eid), nd, E, K, H, *row_ptr(x),
                                    ptr(s_src), _at(s_dst, d0), float(slope), float(p), seed64(seed), ptr(seed_buf),
                                    _at(agg, d0), _at(m, d0), _at(inv_l, d0), ptr(xbits), ptr(ws), nbytes,
                                    stream_handle(dev)), "xgat_fwd_colmax")


def xgat_bwd_prologue(gt, agg, s_dst, m, inv_l, n_dst: int, K: int, H: int, nstate):
    check(load().ppgat_xgat_bwd_prologue(ptr(gt), ptr(agg), ptr(s_dst), ptr(m), ptr(inv_l), n_dst, K, H, ptr(nstate),
                                         stream_handle(gt.device)), "xgat_bwd_prologue")


def xgat_bwd_edges(sched, v, base: int, x, s_src, nstate, gt, A, S, dz, dx, H: int, slope, p, seed, seed_buf):
    """The gt-gathering edge pass over one source schedule whose rows start at ``base``."""
    lib, dev, E = load(), x.device, v.n_edges
    K = x.size(1)
    ws, nbytes = workspace(lib.ppgat_xgat_bwd_workspace_bytes, sched.n_hub_items, K, device=dev)
    check(lib.ppgat_xgat_bwd_edges(_sched(sched), *edge_ptrs(E, v.row, v.csc_eid, v.dz_slot), E, K, H,
                                   *row_ptr(x, base), _at(s_src, base), ptr(nstate), ptr(gt), ptr(A), float(slope),
                                   float(p), seed64(seed), ptr(seed_buf), *row_ptr(dx, base), *row_ptr(S, base),
                                   ptr(dz), ptr(ws), nbytes, stream_handle(dev)), "xgat_bwd_edges")


def xgat_bwd_edges_g(sched, v, base: int, hs, s_src, nstate, g, acc, S, dz, H: int, C: int, slope, p, seed,
                     seed_buf):
    """The g-gathering edge pass over one source schedule whose rows start at ``base``."""
    lib, dev, E = load(), hs.device, v.n_edges
    ws, nbytes = workspace(lib.ppgat_xgat_bwd_g_workspace_bytes, sched.n_hub_items, C, H, device=dev)
    check(lib.ppgat_xgat_bwd_edges_g(_sched(sched), *edge_ptrs(E, v.row, v.csc_eid, v.dz_slot), E, C, H,
                                     _at(hs, base), _at(s_src, base), ptr(nstate), *row_ptr(g), float(slope),
                                     float(p), seed64(seed), ptr(seed_buf), _at(acc, base), *row_ptr(S, base),
                                     ptr(dz), ptr(ws), nbytes, stream_handle(dev)), "xgat_bwd_edges_g")


def xgat_bwd_edges_gd_colmax(sched, v, base: int, hs, s_src, nstate, g, acc, dz, pdal, gbits, H: int, C: int, slope,
                             p, seed, seed_buf):
    """The deferred-D edge pass over one source schedule whose rows start at ``base``: dalpha into dz,
    beta dalpha into pdal, acc, gbits.  nstate and g: the destination tables (local, or a halo layer's)."""
    lib, dev, E = load(), hs.device, v.n_edges
    ws, nbytes = workspace(lib.ppgat_xgat_bwd_g_workspace_bytes, sched.n_hub_items, C, H, device=dev)
    check(lib.ppgat_xgat_bwd_edges_gd_colmax(_sched(sched), *edge_ptrs(E, v.row, v.csc_eid, v.dz_slot), E, C, H,
                                             _at(hs, base), _at(s_src, base), ptr(nstate), *row_ptr(g),
                                             float(slope), float(p), seed64(seed), ptr(seed_buf), _at(acc, base),
                                             ptr(dz), ptr(pdal), ptr(gbits), ptr(ws), nbytes, stream_handle(dev)),
          "xgat_bwd_edges_gd_colmax")


def xgat_nstate(s_dst, m, inv_l, D, n: int, H: int, nstate):
    """nstate {s_dst, m, inv_l, D} of n rows (D None: left for xgat_nstate_set_d)."""
    check(load().ppgat_xgat_nstate(ptr(s_dst), ptr(m), ptr(inv_l), ptr(D), n, H, ptr(nstate),
                                   stream_handle(nstate.device)), "xgat_nstate")


def xgat_nstate_set_d(nstate, D, n: int, H: int):
    check(load().ppgat_xgat_nstate_set_d(ptr(nstate), ptr(D), n, H, stream_handle(nstate.device)),
          "xgat_nstate_set_d")


def xgat_bwd_dz(sched, v, base: int, s_src, nstate, dz, S, H: int, slope, p, seed, seed_buf):
    """The deferred-D dz pass over one source schedule: dz in place over dalpha, ds_src into S[base:, :H]."""
    lib, dev, E = load(), dz.device, v.n_edges
    ws, nbytes = workspace(lib.ppgat_xgat_bwd_dz_workspace_bytes, sched.n_hub_items, H, device=dev, floor=4)
    check(lib.ppgat_xgat_bwd_dz(_sched(sched), *edge_ptrs(E, v.row, v.csc_eid, v.dz_slot), E, H, _at(s_src, base),
                                ptr(nstate), float(slope), float(p), seed64(seed), ptr(seed_buf), ptr(dz),
                                *row_ptr(S, base), ptr(ws), nbytes, stream_handle(dev)), "xgat_bwd_dz")


def xgat_bwd_epilogue(S, A, n_dst: int, H: int, dx):
    """dx[:n_dst] += S A (the attention terms of the gt-gathering backward)."""
    check(load().ppgat_xgat_bwd_epilogue(*row_ptr(S), ptr(A), n_dst, dx.size(1), H, *row_ptr(dx),
                                         stream_handle(dx.device)), "xgat_bwd_epilogue")


def xgat_weight_grads(G, GV, W, a_s, a_d, H: int, C: int, dW, datt_src, datt_dst):
    check(load().ppgat_xgat_weight_grads(ptr(G), ptr(GV), ptr(W), ptr(a_s), ptr(a_d), H, C, W.size(1), ptr(dW),
                                         ptr(datt_src), ptr(datt_dst), stream_handle(W.device)), "xgat_weight_grads")
