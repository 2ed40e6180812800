"""Every kernel launch of the package (include/ppgat.h), one function per ABI entry or variant family.

The callers (the ops_* modules behind hip_ops, dist.py, sampler.py, evaluation.py, ...) decide
what runs, in which order and into which tensors; here those tensors are handed to libppgat.so
on the current stream of their device: workspace, schedule struct (a fresh one per call), NULL
edge arrays of an edge-less view, 64-bit seed, row offsets (``r0`` / ``base``: a row of the
tensor, made an address and a leading dimension by _lib.row_ptr), return-code check.  A launch
allocates its workspace and block partials only; where the caller keeps a workspace alive, or
allocates it before its outputs, ``*_workspace`` hands it out and the launch takes it.  Leading
dimensions (``ld*``) are the caller's: they are passed on as given.  _lib.py itself calls only
the entries it needs to load, check and profile the library.
"""
from __future__ import annotations

import ctypes

import torch

from ._lib import check, edge_ptrs, load, ptr, row_ptr, seed64, stream_handle, workspace


def _at(t, row: int = 0):
    return row_ptr(t, row)[0]


def _workspace_as(what: str, entry, *args, device, floor: int = 0):
    """_lib.workspace whose failure is reported under ``what`` instead of the entry's name."""
    nbytes = ctypes.c_size_t(0)
    check(entry(*args, ctypes.byref(nbytes)), what)
    return torch.empty(max(int(nbytes.value), floor), dtype=torch.uint8, device=device), nbytes.value


def _sched(sched, all_long: bool = False):
    cs = sched.cstruct()
    if all_long:  # hip_ops._xgat_dst_sum decides
        cs.n_long_items = -1
    return ctypes.byref(cs)


def _f32(n: int, dev):
    return torch.empty(n, dtype=torch.float32, device=dev)


# graph preprocessing (ppgat_csr_*, ppgat_schedule_*, ppgat_invert_index)
def supported_channels(channels: int) -> bool:
    return bool(load().ppgat_supported_channels(int(channels)))


def schedule_capacity(n_rows: int, n_edges: int, max_edges: int) -> int:
    return int(load().ppgat_schedule_capacity(n_rows, n_edges, max_edges))


def schedule_build(rowptr, n_rows: int, n_edges: int, max_edges: int, item_row, item_beg, item_end, hub_row, hub_ptr,
                   counts):
    """Work items over rowptr [n_rows + 1]; counts [4] int32 = (hubs, hub items, items, long rows)."""
    lib, dev = load(), rowptr.device
    ws, nbytes = workspace(lib.ppgat_schedule_workspace_bytes, n_rows, device=dev, floor=1)
    check(lib.ppgat_schedule_build(ptr(rowptr), n_rows, n_edges, max_edges, ptr(item_row), ptr(item_beg),
                                   ptr(item_end), ptr(hub_row), ptr(hub_ptr), ptr(counts), ptr(ws), nbytes,
                                   stream_handle(dev)), "schedule_build")


def csr_build(edge_index, n_edges: int, n_nodes: int, rowptr, col, csr_eid, colptr, row, csc_eid, csc2csr, bad):
    lib, dev = load(), edge_index.device
    ws, nbytes = workspace(lib.ppgat_csr_workspace_bytes, n_nodes, n_edges, device=dev, floor=1)
    with torch.cuda.device(dev):
        check(lib.ppgat_csr_build(ptr(edge_index), n_edges, n_nodes, ptr(rowptr), ptr(col), ptr(csr_eid), ptr(colptr),
                                  ptr(row), ptr(csc_eid), ptr(csc2csr), ptr(bad), ptr(ws), nbytes, stream_handle(dev)),
              "csr_build")


def invert_index(perm, n: int, inv):
    """inv[perm[k]] = k over n entries."""
    check(load().ppgat_invert_index(*edge_ptrs(n, perm), n, ptr(inv), stream_handle(inv.device)), "invert_index")


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


def bwd(g, h, s_src, s_dst, att_src, att_dst, bias, out, agg, m, inv_l, grad_out, heads: int, channels: int,
        mode: int, slope, p, seed, seed_buf, grad_h, datt_src, datt_dst, dbias):
    """The whole backward of the aggregate in one call (ppgat_bwd); ``g``: a hip_ops.CSRGraph."""
    lib, dev, N, E = load(), h.device, g.n_nodes, g.n_edges
    ws, nbytes = workspace(lib.ppgat_bwd_workspace_bytes, N, E, g.bwd_sched.n_hub_items, heads, channels, device=dev)
    check(lib.ppgat_bwd(_sched(g.bwd_sched), ptr(g.rowptr), *edge_ptrs(E, g.row, g.csc_eid, g.csc2csr), N, E, heads,
                        channels, ptr(h), ptr(s_src), ptr(s_dst), ptr(att_src), ptr(att_dst), ptr(bias), ptr(out),
                        ptr(agg), ptr(m), ptr(inv_l), ptr(grad_out), mode, float(slope), float(p), seed64(seed),
                        ptr(seed_buf), ptr(grad_h), ptr(datt_src), ptr(datt_dst), ptr(dbias), ptr(ws), nbytes,
                        stream_handle(dev)), "gat_bwd")


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


# projections and the fp32 matrix-core GEMMs (ppgat_project*, ppgat_gemm_*, ppgat_col*)
def project_supported(k: int, out_cols: int) -> bool:
    return bool(load().ppgat_project_supported(int(k), int(out_cols)))


def project(x, ldx: int, x_items, ldx_items: int, split: int, n: int, weight, bias, att_src, att_dst, y, s_src, s_dst):
    """y [n, HC] = [x; x_items] weight^T (+ bias), rows [0, split) from x; s_src / s_dst when att_* are given."""
    K, HC = weight.size(1), weight.size(0)
    check(load().ppgat_project(ptr(x), ldx, ptr(x_items), ldx_items, split, n, K, ptr(weight), weight.stride(0), HC,
                               ptr(bias), ptr(att_src), ptr(att_dst), ptr(y), HC, ptr(s_src), ptr(s_dst),
                               stream_handle(x.device)), "project")


def project_bwd_input(D, n: int, W, a_s, a_d, S, dx):
    """dx [n, K] = D W + S [A_src; A_dst] for heads = 1 (D [n, HC], S [n, 2], all contiguous)."""
    HC, K = W.shape
    check(load().ppgat_project_bwd_input(ptr(D), HC, n, HC, ptr(W), K, K, ptr(a_s), ptr(a_d), ptr(S), 2, ptr(dx), K,
                                         stream_handle(D.device)), "project_bwd_input")


def project_bwd_fused_supported(k: int) -> bool:
    return bool(load().ppgat_project_bwd_fused_supported(int(k)))


def project_bwd_fused_workspace(n: int, dev):
    return workspace(load().ppgat_project_bwd_fused_workspace_bytes, n, device=dev, floor=1)


def project_bwd_fused(D, S, x0, x1, split: int, n: int, W, a_s, a_d, dx, G, GV, ws, nbytes: int, producer=None):
    """dx, G = D^T x and GV = S^T x in one pass (heads = 1, HC = K; x = [x0; x1] split at ``split``).
    ``producer`` = (bias, s_dst, m, inv_l, nstate, dbias): the producing layer's backward prologue
    from dx as well (ppgat_project_bwd_fused_producer)."""
    lib = load()
    HC, K = W.shape
    head = (ptr(D), HC, ptr(S), 2, ptr(x0), K, ptr(x1), K, split, n, K, ptr(W), K, ptr(a_s), ptr(a_d), ptr(dx), K,
            ptr(G), ptr(GV))
    tail = (ptr(ws), nbytes, stream_handle(D.device))
    if producer is None:
        check(lib.ppgat_project_bwd_fused(*head, *tail), "project_bwd_fused")
    else:
        pb, ps_dst, pm, pinv_l, p_nstate, p_dbias = producer
        check(lib.ppgat_project_bwd_fused_producer(*head, ptr(pb), ptr(ps_dst), ptr(pm), ptr(pinv_l), 1.0,
                                                   ptr(p_nstate), ptr(p_dbias), *tail), "project_bwd_fused_producer")


def weight_grads(G, GV, W, a_s, a_d, heads: int, C: int, dW, datt_src, datt_dst):
    check(load().ppgat_weight_grads(ptr(G), ptr(GV), ptr(W), ptr(a_s), ptr(a_d), heads, C, W.size(1), ptr(dW),
                                    ptr(datt_src), ptr(datt_dst), stream_handle(W.device)), "weight_grads")


def gemm_tn(A, lda: int, B, ldb: int, B_items, ldb1: int, V, ldv: int, out, cs, vout):
    """out [M, K] = A^T [B; B_items], cs = colsum(A), vout = V^T B (each when given); with
    ``B_items`` the B rows come in two segments (ppgat_gemm_tn_seg)."""
    lib, dev = load(), A.device
    N, M, K = A.size(0), A.size(1), B.size(1)
    nv = 0 if V is None else V.size(1)
    ws, nbytes = workspace(lib.ppgat_gemm_tn_workspace_bytes, N, M, K, nv, device=dev)
    tail = (N, M, K, ptr(out), ptr(cs), ptr(V) if nv else None, ldv, nv, ptr(vout), ptr(ws), nbytes,
            stream_handle(dev))
    if B_items is None:
        check(lib.ppgat_gemm_tn(ptr(A), lda, ptr(B), ldb, *tail), "gemm_tn")
    else:
        check(lib.ppgat_gemm_tn_seg(ptr(A), lda, ptr(B), ldb, ptr(B_items), ldb1, B.size(0), *tail), "gemm_tn")


def gemm_nn_supported(m: int, k: int, n: int, b_layout: int) -> bool:
    return bool(load().ppgat_gemm_nn_supported(int(m), int(k), int(n), int(b_layout)))


def gemm_nn(x, ldx: int, B, b_layout: int, n: int, alpha, bias, y, ldy: int, rank=None, lds: int = 0):
    """y [M, n] = alpha x B (+ bias); ``rank`` = (S [M, nv], A [nv, n]): + S A (ppgat_gemm_nn_rank)."""
    lib, dev = load(), x.device
    M, K = x.shape
    ws, nbytes = None, 0
    if gemm_nn_supported(M, K, n, b_layout):
        ws, nbytes = _workspace_as("gemm_nn_workspace_bytes", lib.ppgat_gemm_nn_workspace_bytes, M, K, n, device=dev)
    head = (ptr(x), ldx, M, K, ptr(B), B.stride(0), b_layout, n, float(alpha), ptr(bias))
    tail = (ptr(y), ldy, ptr(ws) if nbytes else None, nbytes, stream_handle(dev))
    if rank is None:
        check(lib.ppgat_gemm_nn_ws(*head, *tail), "gemm_nn")
    else:
        S, A = rank
        check(lib.ppgat_gemm_nn_rank(*head, ptr(S), lds, S.size(1), ptr(A), n, *tail), "gemm_nn_rank")


def att_proj(W, a_s, a_d, heads: int, channels: int, A):
    check(load().ppgat_att_proj(ptr(W), ptr(a_s), ptr(a_d), heads, channels, W.size(1), ptr(A),
                                stream_handle(W.device)), "att_proj")


def rows_rank_update(S, lds: int, A, dx, lddx: int):
    """dx [n, K] += S [n, nv] A [nv, K] in place."""
    n, K = dx.shape
    check(load().ppgat_rows_rank_update(ptr(S), lds, S.size(1), ptr(A), K, n, K, ptr(dx), lddx,
                                        stream_handle(dx.device)), "rows_rank_update")


def colmax_abs(X, ld: int, out, src_ptr=None):
    """out [c] int32 = bits of max_i |X[i, :]|; with ``src_ptr`` over the rows that are an edge's
    source only (ppgat_colmax_abs_sources)."""
    lib, (n, c), st = load(), X.shape, stream_handle(X.device)
    if src_ptr is None:
        check(lib.ppgat_colmax_abs(ptr(X), ld, n, c, ptr(out), st), "colmax_abs")
    else:
        check(lib.ppgat_colmax_abs_sources(ptr(X), ld, n, c, ptr(src_ptr), ptr(out), st), "colmax_abs_sources")


def gemm_tn_big_workspace(n_rows: int, ma: int, nb: int, dev):
    return workspace(load().ppgat_gemm_tn_big_workspace_bytes, n_rows, ma, nb, device=dev, floor=1)


def gemm_tn_big(A, lda: int, B, ldb: int, out, ws, nbytes: int, b_bound=None, a_bits=None, cs=None):
    """out [ma, nb] = A^T B.  ``cs`` given: colsum(A) too (ppgat_gemm_tn_big_colsum); else ``a_bits``
    given: ppgat_gemm_tn_big_bounds; else ``b_bound`` = (bits, period, scale) given:
    ppgat_gemm_tn_big_bounded; else ppgat_gemm_tn_big."""
    lib = load()
    M, ma = A.shape
    head = (ptr(A), lda, ptr(B), ldb, M, ma, B.size(1))
    tail = (ptr(ws), nbytes, stream_handle(A.device))
    bits, period, scale = b_bound if b_bound is not None else (None, 1, 1.0)
    bound = (ptr(bits), int(period), float(scale))
    if cs is not None:
        check(lib.ppgat_gemm_tn_big_colsum(*head, ptr(a_bits), *bound, ptr(out), ptr(cs), *tail), "gemm_tn_big_colsum")
    elif a_bits is not None:
        check(lib.ppgat_gemm_tn_big_bounds(*head, ptr(a_bits), *bound, ptr(out), *tail), "gemm_tn_big_bounds")
    elif b_bound is not None:
        check(lib.ppgat_gemm_tn_big_bounded(*head, *bound, ptr(out), *tail), "gemm_tn_big_bounded")
    else:
        check(lib.ppgat_gemm_tn_big(*head, ptr(out), *tail), "gemm_tn_big")


def colsum_workspace(n: int, c: int, dev):
    return workspace(load().ppgat_colsum_workspace_bytes, n, c, device=dev, floor=1)


def colsum(Y, ld: int, out, ws, nbytes: int):
    n, c = Y.shape
    check(load().ppgat_colsum(ptr(Y), ld, n, c, ptr(out), ptr(ws), nbytes, stream_handle(Y.device)), "colsum")


def xgat_supported(in_channels: int, heads: int, channels: int) -> bool:
    return bool(load().ppgat_xgat_supported(int(in_channels), int(heads), int(channels)))


# the losses (ppgat_bpr_*, ppgat_ssm_*, ppgat_shs_*).  The workspace is the caller's: the forward
# leaves in it what the backward reads, and a prepared BPR backward fills it on a side stream.
def bpr_workspace(n_rows: int, n_triples: int, C: int, dev):
    return workspace(load().ppgat_bpr_workspace_bytes, n_rows, n_triples, C, device=dev)[0]


def bpr_bwd_prepare(n_rows: int, n_users: int, n_items: int, row_map, C: int, u, i, j, ws, stream):
    """The triple-only half of the loss backward into ``ws``, on ``stream`` (a torch.cuda.Stream:
    the one launch that does not run on the current stream)."""
    check(load().ppgat_bpr_bwd_prepare(n_rows, n_users, n_items, ptr(row_map), C, ptr(u), ptr(i), ptr(j), u.numel(),
                                       ptr(ws), ws.numel(), stream.cuda_stream), "bpr_bwd_prepare")


def bpr_fwd(Z, n_users: int, n_items: int, row_map, u, i, j, kind: int, loss, coef, bad, ws):
    n_rows, C = Z.shape
    check(load().ppgat_bpr_fwd(ptr(Z), n_rows, n_users, n_items, ptr(row_map), C, ptr(u), ptr(i), ptr(j), u.numel(),
                               kind, ptr(loss), ptr(coef), ptr(bad), ptr(ws), ws.numel(), stream_handle(Z.device)),
          "bpr_fwd")


def bpr_bwd(Z, n_users: int, n_items: int, row_map, u, i, j, coef, gl, dZ, ws, prepared: bool):
    """``prepared``: ``ws`` holds what bpr_bwd_prepare left (ppgat_bpr_bwd_prepared)."""
    lib = load()
    n_rows, C = Z.shape
    entry = lib.ppgat_bpr_bwd_prepared if prepared else lib.ppgat_bpr_bwd
    check(entry(ptr(Z), n_rows, n_users, n_items, ptr(row_map), C, ptr(u), ptr(i), ptr(j), u.numel(), ptr(coef),
                ptr(gl), ptr(dZ), ptr(ws), ws.numel(), stream_handle(Z.device)), "bpr_bwd")


def bpr_bwd_producer(Z, n_users: int, n_items: int, u, i, j, coef, gl, dZ, pb, ps_dst, pm, pinv_l, p_nstate, p_dbias,
                     ws):
    """bpr_bwd with the backward prologue of the layer that produced Z (its nstate and dbias from dZ)."""
    n_rows, C = Z.shape
    check(load().ppgat_bpr_bwd_producer(ptr(Z), n_rows, n_users, n_items, C, ptr(u), ptr(i), ptr(j), u.numel(),
                                        ptr(coef), ptr(gl), ptr(dZ), ptr(pb), ptr(ps_dst), ptr(pm), ptr(pinv_l), 1.0,
                                        ptr(p_nstate), ptr(p_dbias), ptr(ws), ws.numel(), stream_handle(Z.device)),
          "bpr_bwd_producer")


def ssm_workspace(n_rows: int, S: int, K1: int, C: int, dev):
    return workspace(load().ppgat_ssm_workspace_bytes, n_rows, S, K1, C, device=dev)[0]


def ssm_fwd(Z, n_users: int, n_items: int, u, cand, temperature, loss, coef, bad, ws, corr=None):
    """``corr`` [n_items]: the logQ term of the negatives (ppgat_ssm_fwd_corrected); None: ppgat_ssm_fwd."""
    lib = load()
    (n_rows, C), (S, K1) = Z.shape, cand.shape
    head = (ptr(Z), n_rows, n_users, n_items, C, ptr(u), ptr(cand))
    tail = (S, K1, temperature, ptr(loss), ptr(coef), ptr(bad), ptr(ws), ws.numel(), stream_handle(Z.device))
    if corr is None:
        check(lib.ppgat_ssm_fwd(*head, *tail), "ssm_fwd")
    else:
        check(lib.ppgat_ssm_fwd_corrected(*head, ptr(corr), *tail), "ssm_fwd_corrected")


def ssm_bwd(Z, n_users: int, n_items: int, u, cand, temperature, coef, gl, dZ, ws):
    (n_rows, C), (S, K1) = Z.shape, cand.shape
    check(load().ppgat_ssm_bwd(ptr(Z), n_rows, n_users, n_items, C, ptr(u), ptr(cand), S, K1, temperature, ptr(coef),
                               ptr(gl), ptr(dZ), ptr(ws), ws.numel(), stream_handle(Z.device)), "ssm_bwd")


def shs_workspace(n_rows: int, S: int, P: int, C: int, corrected: bool, dev):
    lib = load()
    return workspace(lib.ppgat_shs_corrected_workspace_bytes if corrected else lib.ppgat_shs_workspace_bytes, n_rows,
                     S, P, C, device=dev)[0]


def shs_fwd(Z, n_users: int, n_items: int, u, pos, pool, hist_ptr, hist_items, temperature, loss, lse, c0, bad, ws,
            corr=None):
    """``corr`` [n_items]: the logQ term of the pool (ppgat_shs_fwd_corrected, ``ws`` from
    shs_workspace(corrected=True)); None: ppgat_shs_fwd.  Leaves the mask words in ``ws``."""
    lib = load()
    n_rows, C = Z.shape
    head = (ptr(Z), n_rows, n_users, n_items, C, ptr(u), ptr(pos), u.numel(), ptr(pool), pool.numel(), ptr(hist_ptr),
            ptr(hist_items))
    tail = (temperature, ptr(loss), ptr(lse), ptr(c0), ptr(bad), ptr(ws), ws.numel(), stream_handle(Z.device))
    if corr is None:
        check(lib.ppgat_shs_fwd(*head, *tail), "shs_fwd")
    else:
        check(lib.ppgat_shs_fwd_corrected(*head, ptr(corr), *tail), "shs_fwd_corrected")


def shs_bwd(Z, n_users: int, n_items: int, u, pos, pool, temperature, lse, c0, gl, dZ, ws, corrected: bool):
    """Reads the mask words (and gathered corrections) shs_fwd left in ``ws``."""
    lib = load()
    n_rows, C = Z.shape
    entry, what = (lib.ppgat_shs_bwd_corrected, "shs_bwd_corrected") if corrected else (lib.ppgat_shs_bwd, "shs_bwd")
    check(entry(ptr(Z), n_rows, n_users, n_items, C, ptr(u), ptr(pos), u.numel(), ptr(pool), pool.numel(), temperature,
                ptr(lse), ptr(c0), ptr(gl), ptr(dZ), ptr(ws), ws.numel(), stream_handle(Z.device)), what)


# the samplers (ppgat_bpr_sampler_*, ppgat_bpr_sample*, ppgat_*eval_sample, ppgat_weighted_draws).
# ``hist_ptr`` int64 [n_users + 1] / ``hist_items`` int32: the users' train lists, sorted per user.
def bpr_sampler_prepare(user_ptr, items, n_users: int, nnz: int, items_sorted, eligible, n_eligible):
    lib, dev = load(), user_ptr.device
    ws, nbytes = _workspace_as("bpr_sampler_workspace_bytes", lib.ppgat_bpr_sampler_workspace_bytes, n_users, nnz,
                               device=dev, floor=1)
    check(lib.ppgat_bpr_sampler_prepare(ptr(user_ptr), ptr(items) if nnz else None, n_users, nnz, ptr(items_sorted),
                                        ptr(eligible), ptr(n_eligible), ptr(ws), nbytes, stream_handle(dev)),
          "bpr_sampler_prepare")


def weighted_draws(cdf, n_items: int, n: int, seed, offset: int, out):
    check(load().ppgat_weighted_draws(ptr(cdf), n_items, n, seed64(seed), offset, ptr(out),
                                      stream_handle(out.device)), "weighted_draws")


def _rows3(out):
    """The addresses of the three rows of ``out`` [3, n] (NULL each when n = 0, as an empty row's is)."""
    return tuple(_at(out, r) if out.size(1) else None for r in range(3))


def bpr_sample(hist_ptr, hist_items, eligible, n_eligible, n_items: int, samples: int, seed, offset: int, out, bad,
               cdf=None):
    """(u, i, j) into the rows of ``out`` [3, samples]; ``cdf``: j under the item weights
    (ppgat_weighted_bpr_sample), None: uniform (ppgat_bpr_sample)."""
    lib = load()
    head = (ptr(hist_ptr), ptr(hist_items), ptr(eligible), ptr(n_eligible), n_items)
    tail = (samples, seed64(seed), offset, *_rows3(out), ptr(bad), stream_handle(out.device))
    if cdf is None:
        check(lib.ppgat_bpr_sample(*head, *tail), "bpr_sample")
    else:
        check(lib.ppgat_weighted_bpr_sample(*head, ptr(cdf), *tail), "weighted_bpr_sample")


def bpr_sample_positives(user_ptr, items_orig, hist_items, n_users: int, nnz: int, n_items: int, neg_per_pos: int,
                         n: int, seed, t0: int, out, bad):
    check(load().ppgat_bpr_sample_positives(ptr(user_ptr), ptr(items_orig), ptr(hist_items), n_users, nnz, n_items,
                                            neg_per_pos, n, seed64(seed), t0, *_rows3(out), ptr(bad),
                                            stream_handle(out.device)), "bpr_sample_positives")


def eval_sample(hist_ptr, hist_items, u, pos, n_neg: int, n_items: int, seed, cands, bad, cdf=None):
    """cands [B, n_neg + 1]; ``cdf``: the negatives under the item weights (ppgat_weighted_eval_sample)."""
    lib = load()
    head = (ptr(hist_ptr), ptr(hist_items), ptr(u), ptr(pos), u.numel(), n_neg, n_items)
    tail = (seed64(seed), ptr(cands), ptr(bad), stream_handle(cands.device))
    if cdf is None:
        check(lib.ppgat_eval_sample(*head, *tail), "eval_sample")
    else:
        check(lib.ppgat_weighted_eval_sample(*head, ptr(cdf), *tail), "weighted_eval_sample")


# evaluation and serving (ppgat_sampled_rank, ppgat_full_rank, ppgat_full_topk, ppgat_serve_topk)
def sampled_rank(Z, n_users: int, n_items: int, row_map, u, cands, rank):
    n_rows, C = Z.shape
    check(load().ppgat_sampled_rank(ptr(Z), n_rows, n_users, n_items, ptr(row_map), C, ptr(u), ptr(cands), len(u),
                                    cands.size(1), ptr(rank), stream_handle(Z.device)), "sampled_rank")


def full_rank(Z_users, Z_items, u, pos, hist_ptr, hist_items, rank, ties):
    """Z_users / Z_items: row or column views of a table, used in place (_lib.row_ptr)."""
    lib, dev, n, C = load(), Z_users.device, u.numel(), Z_users.size(1)
    ws, nbytes = workspace(lib.ppgat_full_rank_workspace_bytes, n, Z_items.size(0), C, device=dev)
    check(lib.ppgat_full_rank(*row_ptr(Z_users), Z_users.size(0), *row_ptr(Z_items), Z_items.size(0), C,
                              *edge_ptrs(n, u, pos), n, ptr(hist_ptr), ptr(hist_items), *edge_ptrs(n, rank, ties),
                              ptr(ws) if nbytes else None, nbytes, stream_handle(dev)), "full_rank")


def full_topk(Z_users, Z_items, u, n: int, hist_ptr, hist_items, k: int, idx, scores):
    """``u`` None: the n = Z_users.size(0) users in order."""
    lib, dev, C = load(), Z_users.device, Z_users.size(1)
    ws, nbytes = workspace(lib.ppgat_full_topk_workspace_bytes, n, Z_items.size(0), C, k, device=dev)
    check(lib.ppgat_full_topk(*row_ptr(Z_users), Z_users.size(0), *row_ptr(Z_items), Z_items.size(0), C,
                              *edge_ptrs(n, u), n, ptr(hist_ptr), ptr(hist_items), k, *edge_ptrs(n, idx, scores),
                              ptr(ws) if nbytes else None, nbytes, stream_handle(dev)), "full_topk")


def serve_topk_workspace(n_items: int, C: int, B: int, dev):
    return _workspace_as("serve_topk_ws", load().ppgat_serve_topk_workspace_bytes, n_items, C, B, device=dev)


def serve_topk(item_vecs, hist_ptr, hist, max_len: int, B: int, k: int, out_idx, out_scores, ws, nbytes: int):
    n_items, C = item_vecs.shape
    check(load().ppgat_serve_topk(ptr(item_vecs), n_items, C, ptr(hist_ptr), ptr(hist), max_len, B, k, ptr(out_idx),
                                  ptr(out_scores), ptr(ws), nbytes, stream_handle(item_vecs.device)), "serve_topk")


# the modality-fusion MLP, InfoNCE and the MLP's dropout (ppgat_fusion_fwd_ws, ppgat_infonce, ppgat_relu_dropout)
def fusion_fwd(txt, img, img_index, img_fallback, Di: int, W1, b1, W2, b2, normalize: bool, out, z1):
    lib, dev = load(), txt.device
    n, Dt = txt.shape
    H1, Do = W1.size(0), W2.size(0)
    ws, nbytes = _workspace_as("fusion_fwd_workspace", lib.ppgat_fusion_fwd_workspace_bytes, Dt, Di, H1, Do,
                               device=dev)  # the pre-split W1 / W2 images
    check(lib.ppgat_fusion_fwd_ws(ptr(txt), ptr(img), ptr(img_index), ptr(img_fallback), n, Dt, Di, ptr(W1), ptr(b1),
                                  H1, ptr(W2), ptr(b2), Do, 1 if normalize else 0, ptr(out), ptr(z1), ptr(ws), nbytes,
                                  stream_handle(dev)), "fusion_fwd")


def infonce_workspace(B: int, D: int, dev):
    return _workspace_as("infonce_workspace_bytes", load().ppgat_infonce_workspace_bytes, B, D, device=dev)


def infonce(fused, txt_p, img_p, temperature, loss, dF, dT, dI, ws, nbytes: int):
    B, D = fused.shape
    check(load().ppgat_infonce(ptr(fused), ptr(txt_p), ptr(img_p), B, D, float(temperature), ptr(loss), ptr(dF),
                               ptr(dT), ptr(dI), ptr(ws), nbytes, stream_handle(fused.device)), "infonce")


def relu_dropout(z, p, seed, backward: bool, out):
    check(load().ppgat_relu_dropout(ptr(z), z.numel(), float(p), seed64(seed), 1 if backward else 0, ptr(out),
                                    stream_handle(z.device)), "relu_dropout")


# the item-item kNN selection (ppgat_knn_topk)
def knn_max_k() -> int:
    return int(load().ppgat_knn_max_k())


def knn_topk(S, ld: int, q0: int, nq: int, n: int, k: int, min_similarity, idx, sim, cnt):
    """The rows [q0, q0 + nq) of idx / sim / cnt from the similarity block S [nq, >= n] of those queries."""
    check(load().ppgat_knn_topk(ptr(S), ld, nq, n, q0, k, float(min_similarity), _at(idx, q0), _at(sim, q0),
                                _at(cnt, q0), stream_handle(S.device)), "knn_topk")


# Adam (ppgat_adam_*): per launch the tensors' addresses go in host arrays
def adam_max_tensors() -> int:
    return int(load().ppgat_adam_max_tensors())


def _ptr_array(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def adam_step(params, grads, exp_avg, exp_avg_sq, step_sizes, bias_corr, b1, b2, eps, weight_decay):
    """One multi-tensor step; step_sizes / bias_corr: per tensor, from the host step count."""
    n = len(params)
    check(load().ppgat_adam_step(n, _ptr_array(params), _ptr_array(grads), _ptr_array(exp_avg),
                                 _ptr_array(exp_avg_sq), (ctypes.c_int64 * n)(*[p.numel() for p in params]),
                                 (ctypes.c_float * n)(*step_sizes), (ctypes.c_float * n)(*bias_corr), float(b1),
                                 float(b2), float(eps), float(weight_decay), stream_handle(params[0].device)),
          "adam_step")


def adam_step_device(params, grads, exp_avg, exp_avg_sq, steps, lr, b1, b2, eps, weight_decay):
    """The capturable step: ``steps``: the device step counts, already advanced."""
    n = len(params)
    check(load().ppgat_adam_step_device(n, _ptr_array(params), _ptr_array(grads), _ptr_array(exp_avg),
                                        _ptr_array(exp_avg_sq), (ctypes.c_int64 * n)(*[p.numel() for p in params]),
                                        _ptr_array(steps), float(lr), float(b1), float(b2), float(eps),
                                        float(weight_decay), stream_handle(params[0].device)), "adam_step_device")


def adam_rows(p, exp_avg, exp_avg_sq, val, idx, step_size, bias_corr, b1, b2, eps, weight_decay, flag):
    """The lazy step of the rows ``idx`` of the table ``p`` with the gradient rows ``val``."""
    check(load().ppgat_adam_rows(ptr(p), ptr(exp_avg), ptr(exp_avg_sq), ptr(val), ptr(idx), idx.numel(), p.size(0),
                                 p.size(1), step_size, bias_corr, float(b1), float(b2), float(eps),
                                 float(weight_decay), ptr(flag), stream_handle(p.device)), "adam_rows")


# LightGCN propagation (ppgat_lgcn_hop)
def lgcn_supported(channels: int) -> bool:
    return bool(load().ppgat_lgcn_supported(int(channels)))


def lgcn_hop_workspace(n_hub_items: int, channels: int, dev):
    return _workspace_as("lgcn_hop_workspace_bytes", load().ppgat_lgcn_hop_workspace_bytes, n_hub_items, channels,
                         device=dev)[0]


def lgcn_hop(sched, idx, val, n_nodes: int, n_edges: int, C: int, s0, s1, ssplit: int, a0, a1, asplit: int, div, out,
             accw, ws):
    """s = A src over ``sched``; src = [s0; s1] split at ssplit, acc_in = [a0; a1] at asplit; ``ws`` or None."""
    check(load().ppgat_lgcn_hop(_sched(sched), *edge_ptrs(n_edges, idx, val), n_nodes, n_nodes, n_edges, C, ptr(s0),
                                ptr(s1), ssplit, ptr(a0), ptr(a1), asplit, float(div), ptr(out), ptr(accw), ptr(ws),
                                ws.numel() if ws is not None else 0, stream_handle(s0.device)), "lgcn_hop")
