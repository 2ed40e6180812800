"""Torch-facing wrappers over the C ABI (include/ppgat.h).

PyTorch is plumbing here: it owns device memory (caching allocator), the current
HIP stream and autograd.  All message-passing arithmetic runs in libppgat.so.
Every function raises if the library is absent or a tensor is not a contiguous
fp32/int64 ROCm tensor of the expected shape -- there is no CPU fallback.
"""
from __future__ import annotations

import ctypes
import os
import weakref
from dataclasses import dataclass
from typing import Callable, Optional

import torch

from . import _launch, _lib


def _require(cond: bool, msg: str):
    if not cond:
        raise RuntimeError(msg)


def _check_dev(name: str, t: torch.Tensor, dtype, device=None):
    _require(isinstance(t, torch.Tensor), f"{name}: expected a tensor")
    _require(t.is_cuda, f"{name}: ppgat runs on ROCm devices only (got {t.device}); there is no CPU path")
    _require(t.dtype == dtype, f"{name}: expected {dtype}, got {t.dtype}")
    _require(t.is_contiguous(), f"{name}: must be contiguous")
    if device is not None:
        _require(t.device == device, f"{name}: on {t.device}, expected {device}")


def _check_rows(name: str, t: torch.Tensor, dtype, device=None):
    """A 2-D operand passed with a row stride (column slices allowed): unit column stride."""
    _require(isinstance(t, torch.Tensor), f"{name}: expected a tensor")
    _require(t.is_cuda, f"{name}: ppgat runs on ROCm devices only (got {t.device}); there is no CPU path")
    _require(t.dtype == dtype, f"{name}: expected {dtype}, got {t.dtype}")
    _require(t.dim() == 2 and (t.stride(1) == 1 or t.size(1) <= 1), f"{name}: 2-D with unit column stride")
    if device is not None:
        _require(t.device == device, f"{name}: on {t.device}, expected {device}")


# ---------------------------------------------------------------------------
# graph preprocessing
# ---------------------------------------------------------------------------
# rows longer than this many edges are split into pieces (include/ppgat.h ppgat_schedule)
MAX_EDGES_PER_ITEM = 256


@dataclass
class Schedule:
    """Device work schedule over a CSR/CSC (owns the arrays ppgat_schedule points at)."""
    item_row: torch.Tensor
    item_beg: torch.Tensor
    item_end: torch.Tensor
    hub_row: torch.Tensor
    hub_ptr: torch.Tensor
    n_items: int
    n_hub_items: int
    n_hubs: int
    max_edges: int
    n_long_items: int = -1  # items [0, n_long_items) have > 16 edges (-1: unknown)

    def cstruct(self) -> "_lib.Schedule":
        return _lib.Schedule(self.item_row.data_ptr(), self.item_beg.data_ptr(), self.item_end.data_ptr(),
                             self.n_items, self.n_hub_items, self.hub_row.data_ptr(), self.hub_ptr.data_ptr(),
                             self.n_hubs, self.n_long_items)


def schedule_build(ptr: torch.Tensor, n_edges: int, max_edges: int = MAX_EDGES_PER_ITEM) -> Schedule:
    """Work items over ptr[N+1] (one host sync to read the four counts)."""
    lib = _lib.load()
    _check_dev("ptr", ptr, torch.int32)
    N = ptr.numel() - 1
    dev = ptr.device
    cap = int(lib.ppgat_schedule_capacity(N, n_edges, max_edges))
    _require(cap >= 0, "schedule_capacity: bad arguments")
    i32 = dict(dtype=torch.int32, device=dev)
    item_row = torch.empty(max(cap, 1), **i32)
    item_beg = torch.empty(max(cap, 1), **i32)
    item_end = torch.empty(max(cap, 1), **i32)
    hub_row = torch.empty(max(N, 1), **i32)
    hub_ptr = torch.empty(N + 1, **i32)
    counts = torch.empty(4, **i32)
    ws, nbytes = _lib.workspace(lib.ppgat_schedule_workspace_bytes, N, device=dev, floor=1)
    _lib.check(lib.ppgat_schedule_build(ptr.data_ptr(), N, n_edges, max_edges, item_row.data_ptr(),
                                        item_beg.data_ptr(), item_end.data_ptr(), hub_row.data_ptr(),
                                        hub_ptr.data_ptr(), counts.data_ptr(), ws.data_ptr(), nbytes,
                                        _lib.stream_handle(dev)), "schedule_build")
    n_hubs, n_hub_items, n_items, n_long_rows = (int(v) for v in counts.cpu().tolist())
    return Schedule(item_row, item_beg, item_end, hub_row, hub_ptr, n_items, n_hub_items, n_hubs, max_edges,
                    n_hub_items + n_long_rows)


@dataclass
class CSRGraph:
    """Static CSR-by-dst / CSC-by-src view of a COO edge_index (int32 indices) plus the
    work schedules of the forward (over rowptr) and backward pass B (over colptr)."""
    n_nodes: int
    n_edges: int
    rowptr: torch.Tensor
    col: torch.Tensor
    csr_eid: torch.Tensor
    colptr: torch.Tensor
    row: torch.Tensor
    csc_eid: torch.Tensor
    csc2csr: torch.Tensor
    fwd_sched: Schedule = None
    bwd_sched: Schedule = None
    # replicated-item partition (dist.build_replicated_graph) of a bipartite graph: (RU, pass-B
    # schedule over the user sources [0, RU), over the item sources [RU, N) with rows relative
    # to RU).  Item sources only reach user destinations, so their edge pass can run before the
    # item rows of grad_out are all-reduced (hip_ops.GATLayer.backward overlaps the two).
    bwd_split: tuple = None
    # the same partition's forward split by destination class: (RU, schedule over the user
    # destinations [0, RU), over the item destinations [RU, N) with rows relative to RU).  The
    # item rows' cross-rank merge (two all_reduces) then runs while the user rows aggregate.
    fwd_split: tuple = None
    # CSC position of each CSR slot (the inverse of csc2csr): pass B writes dz contiguously in
    # CSC order and the destination sums read it through this (_csr2csc builds it once)
    csr2csc: torch.Tensor = None
    # staged edge attributes (stage_edge_attr): [(tensor ref, key, attr_csr, attr_csc)], newest last
    edge_attr_staged: list = None

    @property
    def device(self):
        return self.rowptr.device

    def in_degree(self) -> torch.Tensor:
        return (self.rowptr[1:] - self.rowptr[:-1])

    def out_degree(self) -> torch.Tensor:
        return (self.colptr[1:] - self.colptr[:-1])


def csr_build(edge_index: torch.Tensor, n_nodes: int, max_edges: int = MAX_EDGES_PER_ITEM) -> CSRGraph:
    """edge_index LongTensor[2,E] (row 0 src, row 1 dst) -> CSRGraph on the same device.

    One host sync (the out-of-range index count), once per static graph.
    """
    lib = _lib.load()
    _require(edge_index.dim() == 2 and edge_index.size(0) == 2, "edge_index must be [2, E]")
    ei = edge_index.contiguous()
    _check_dev("edge_index", ei, torch.int64)
    dev = ei.device
    E = int(ei.size(1))
    N = int(n_nodes)
    i32 = dict(dtype=torch.int32, device=dev)
    rowptr = torch.empty(N + 1, **i32)
    colptr = torch.empty(N + 1, **i32)
    col = torch.empty(max(E, 1), **i32)
    csr_eid = torch.empty(max(E, 1), **i32)
    row = torch.empty(max(E, 1), **i32)
    csc_eid = torch.empty(max(E, 1), **i32)
    csc2csr = torch.empty(max(E, 1), **i32)
    bad = torch.empty(1, **i32)
    ws, nbytes = _lib.workspace(lib.ppgat_csr_workspace_bytes, N, E, device=dev, floor=1)
    with torch.cuda.device(dev):
        _lib.check(lib.ppgat_csr_build(ei.data_ptr(), E, N, rowptr.data_ptr(), col.data_ptr(), csr_eid.data_ptr(),
                                       colptr.data_ptr(), row.data_ptr(), csc_eid.data_ptr(), csc2csr.data_ptr(),
                                       bad.data_ptr(), ws.data_ptr(), nbytes, _lib.stream_handle(dev)),
                   "csr_build")
    nbad = int(bad.item())
    if nbad:
        raise RuntimeError(f"edge_index has {nbad} entries outside [0, {N})")
    with torch.cuda.device(dev):
        fs = schedule_build(rowptr, E, max_edges)
        bs = schedule_build(colptr, E, max_edges)
    G = CSRGraph(N, E, rowptr, col[:E], csr_eid[:E], colptr, row[:E], csc_eid[:E], csc2csr[:E], fs, bs)
    if _lib.debug_build():
        debug_validate_graph(G)
    with torch.cuda.device(dev):
        _csr2csc(G)
    return G


def _csr2csc(g) -> torch.Tensor:
    """g.csr2csc, built on the device from g.csc2csr on first use (ppgat_invert_index)."""
    if g.csr2csc is None:
        E = g.n_edges
        inv = torch.empty(max(E, 1), dtype=torch.int32, device=g.csc2csr.device)
        _lib.check(_lib.load().ppgat_invert_index(*_lib.edge_ptrs(E, g.csc2csr), E, inv.data_ptr(),
                                                  _lib.stream_handle(inv.device)), "invert_index")
        g.csr2csc = inv[:E]
    return g.csr2csc


def debug_validate_graph(G: "CSRGraph"):
    """Debug build (libppgat_debug.so): every index array of a graph view within its bounds
    before any kernel reads it (ppgat_check_index_range)."""
    N, E = G.n_nodes, G.n_edges
    for name, t, hi in (("rowptr", G.rowptr, E + 1), ("colptr", G.colptr, E + 1), ("col", G.col, N),
                        ("row", G.row, N), ("csr_eid", G.csr_eid, E), ("csc_eid", G.csc_eid, E),
                        ("csc2csr", G.csc2csr, E)):
        _lib.check_index_range(t, 0, hi, f"graph.{name}")


class _GraphCache:
    """Static-graph cache keyed on (data_ptr, _version, N, device); holds the key tensor."""

    def __init__(self, capacity: int = 8):
        self.capacity = capacity
        self.entries = []  # list of (key, edge_index ref, graph)

    def get(self, edge_index: torch.Tensor, n_nodes: int) -> CSRGraph:
        key = (edge_index.data_ptr(), edge_index._version, tuple(edge_index.shape), int(n_nodes),
               str(edge_index.device))
        for k, ref, g in self.entries:
            if k == key and ref is edge_index:
                return g
        g = csr_build(edge_index, n_nodes)
        self.entries.append((key, edge_index, g))
        if len(self.entries) > self.capacity:
            self.entries.pop(0)
        return g

    @staticmethod
    def _key(edge_index: torch.Tensor, n_nodes: int):
        return (edge_index.data_ptr(), edge_index._version, tuple(edge_index.shape), int(n_nodes),
                str(edge_index.device))

    def put(self, edge_index: torch.Tensor, n_nodes: int, graph: CSRGraph):
        """Register a graph made elsewhere (neighbors.NeighborSampler's derived one) under
        ``edge_index``: ``get`` then returns it without a csr_build.  Replaces an entry of the
        same tensor."""
        self.drop(edge_index)
        self.entries.append((self._key(edge_index, n_nodes), edge_index, graph))
        if len(self.entries) > self.capacity:
            self.entries.pop(0)

    def drop(self, edge_index: torch.Tensor):
        """Forget the entries of this very tensor (no-op when there is none)."""
        self.entries = [t for t in self.entries if t[1] is not edge_index]

    def clear(self):
        self.entries.clear()


graph_cache = _GraphCache()


# ---------------------------------------------------------------------------
# edge attributes (GATConv edge_dim): staging into slot order, once per (graph, tensor)
# ---------------------------------------------------------------------------
EDGE_MAX_DIM = 16  # include/ppgat.h PPGAT_EDGE_MAX_DIM
# how many times stage_edge_attr permuted a tensor (a cache hit leaves it alone)
EDGE_STAGE_COUNT = 0


def check_edge_attr(edge_attr, n_edges: int, device) -> torch.Tensor:
    """The user's ``edge_attr`` as [E, D] (1-D means D = 1, as in PyG): fp32, on ``device``, E rows,
    1 <= D <= EDGE_MAX_DIM, no gradient -- edge features are inputs here."""
    if not isinstance(edge_attr, torch.Tensor):
        raise ValueError("edge_attr: expected a tensor")
    if edge_attr.dtype != torch.float32:
        raise ValueError(f"edge_attr: expected torch.float32, got {edge_attr.dtype}")
    if edge_attr.device != device:
        raise ValueError(f"edge_attr: on {edge_attr.device}, expected {device}")
    if edge_attr.dim() not in (1, 2) or edge_attr.size(0) != n_edges:
        raise ValueError(f"edge_attr: expected [{n_edges}] or [{n_edges}, D], got {tuple(edge_attr.shape)}")
    if edge_attr.requires_grad:
        raise NotImplementedError("edge_attr.requires_grad: gradients with respect to edge features are not "
                                  "implemented")
    D = 1 if edge_attr.dim() == 1 else edge_attr.size(1)
    if D < 1:
        raise ValueError("edge_attr: expected at least one feature per edge")
    if D > EDGE_MAX_DIM:
        raise NotImplementedError(f"edge_attr with {D} features per edge not implemented (edge_dim <= "
                                  f"{EDGE_MAX_DIM})")
    return edge_attr


def stage_edge_attr(g: CSRGraph, edge_attr: torch.Tensor):
    """(attr_csr, attr_csc) [E, D]: ``edge_attr`` in the CSR and CSC slot order of ``g``
    (ppgat_edge_attr_permute), cached on the graph per (tensor object, version, pointers, shape) as
    _const_colmax does -- never on an address alone.  A miss launches kernels and must not happen
    inside a stream capture: stage eagerly first (a warm-up step, or this call)."""
    global EDGE_STAGE_COUNT
    edge_attr = check_edge_attr(edge_attr, g.n_edges, g.device)
    key = (edge_attr._version, edge_attr.data_ptr(), edge_attr.untyped_storage().data_ptr(), tuple(edge_attr.shape),
           tuple(edge_attr.stride()))
    if g.edge_attr_staged is None:
        g.edge_attr_staged = []
    g.edge_attr_staged = [e for e in g.edge_attr_staged if e[0]() is not None]
    for ref, k, a_csr, a_csc in g.edge_attr_staged:
        if ref() is edge_attr and k == key:
            return a_csr, a_csc
    _require(not torch.cuda.is_current_stream_capturing(),
             "stage_edge_attr: edge_attr is staged outside graph capture (run one eager step first)")
    E = g.n_edges
    D = 1 if edge_attr.dim() == 1 else edge_attr.size(1)
    src = edge_attr.reshape(E, D).contiguous()
    a_csr = torch.empty(max(E, 1), D, dtype=torch.float32, device=g.device)[:E]
    a_csc = torch.empty(max(E, 1), D, dtype=torch.float32, device=g.device)[:E]
    with torch.cuda.device(g.device):
        _launch.edge_attr_permute(src, g.csr_eid, E, a_csr)
        _launch.edge_attr_permute(src, g.csc_eid, E, a_csc)
    EDGE_STAGE_COUNT += 1
    g.edge_attr_staged = [e for e in g.edge_attr_staged if e[0]() is not edge_attr][-3:]
    g.edge_attr_staged.append((weakref.ref(edge_attr), key, a_csr, a_csc))
    return a_csr, a_csc


def edge_terms(g: CSRGraph, staged, edge_v: torch.Tensor, heads: int, want_csc: bool):
    """t_csr (and t_csc for the backward) [E, H] = staged attributes . edge_v [H, D] (ppgat_edge_terms)."""
    a_csr, a_csc = staged
    E = g.n_edges
    t_csr = torch.empty(max(E, 1) * heads, dtype=torch.float32, device=edge_v.device)
    t_csc = torch.empty(max(E, 1) * heads, dtype=torch.float32, device=edge_v.device) if want_csc else None
    _launch.edge_terms(a_csr, a_csc if want_csc else None, edge_v, E, heads, t_csr, t_csc)
    return t_csr, t_csc


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


# Test instrumentation (None in normal runs): a list that receives, per GAT layer call, the side
# of the LeakyReLU kink each edge's logit z = s_src[j] + s_dst[i] fell on in THIS forward --
# (edge_index column ids [E_local] int64, z > 0 [E_local, heads] bool), z formed exactly as the
# edge kernels form it (one fp32 add of the same node terms).  The full-size gradient checks
# hand it to the oracle (oracle/gat_oracle.py kink_pos): a logit within fp32 resolution of 0 may
# take either side in any fp32 implementation, and the logit gradient depends on the side.
KINK_TAP: Optional[list] = None


def _tap_kinks(rowptr, col, csr_eid, s_src, s_dst, heads: int):
    if KINK_TAP is None or col is None or rowptr is None:
        return
    E = int(col.numel())
    if E == 0:
        return
    # in slices of 2^23 edges: formed in one piece over the 200M edges of config 5's whole graph
    # ([E, H] gathers and compare) the sides came out wrong for part of the edges on this torch
    # build -- the destinations themselves and the kernels' results were right
    # (tests/test_gpu_cfg5_diag.py); sliced, the full-graph test's oracle agrees with them
    rp = rowptr.long()
    ss, sd = s_src.reshape(-1, heads), s_dst.reshape(-1, heads)
    sides = torch.empty(E, heads, dtype=torch.bool, device=col.device)
    step = 1 << 23
    for a in range(0, E, step):
        b = min(E, a + step)
        k = torch.arange(a, b, device=col.device)
        dst = torch.searchsorted(rp, k, right=True) - 1
        sides[a:b] = (ss[col[a:b].long()] + sd[dst]) > 0
    KINK_TAP.append((csr_eid[:E].long().clone(), sides))


def seed_buffer(dropout_p: float, device) -> Optional[torch.Tensor]:
    """Device slot for the effective mask seed a forward used (include/ppgat.h ppgat_fwd
    seed_used), handed to its backward; None without dropout."""
    return torch.empty(1, dtype=torch.int64, device=device) if dropout_p > 0 else None


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
    lib = _lib.load()
    N = g.n_nodes
    dev = h.device
    _check_dev("grad_out", grad_out, torch.float32, dev)
    grad_h = torch.empty(N, heads * channels, dtype=torch.float32, device=dev)
    datt_src = torch.empty(heads, channels, dtype=torch.float32, device=dev)
    datt_dst = torch.empty(heads, channels, dtype=torch.float32, device=dev)
    dbias = torch.empty(channels, dtype=torch.float32, device=dev) if want_bias_grad else None
    sched, E = g.bwd_sched, g.n_edges
    ws, nbytes = _lib.workspace(lib.ppgat_bwd_workspace_bytes, N, E, sched.n_hub_items, heads, channels, device=dev)
    cs = sched.cstruct()
    _lib.check(lib.ppgat_bwd(ctypes.byref(cs), g.rowptr.data_ptr(), *_lib.edge_ptrs(E, g.row, g.csc_eid, g.csc2csr),
                             N, E, heads, channels, h.data_ptr(), s_src.data_ptr(), s_dst.data_ptr(),
                             att_src.data_ptr(), att_dst.data_ptr(), _lib.ptr(bias), out.data_ptr(), _lib.ptr(agg),
                             m.data_ptr(), inv_l.data_ptr(), grad_out.data_ptr(), mode, float(slope),
                             float(dropout_p), _lib.seed64(seed), _lib.ptr(seed_buf), grad_h.data_ptr(),
                             datt_src.data_ptr(), datt_dst.data_ptr(), _lib.ptr(dbias), ws.data_ptr(), nbytes,
                             _lib.stream_handle(dev)), "gat_bwd")
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


def project_supported(k: int, out_cols: int) -> bool:
    return bool(_lib.load().ppgat_project_supported(int(k), int(out_cols)))


def project(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None,
            att_src: Optional[torch.Tensor] = None, att_dst: Optional[torch.Tensor] = None,
            x_items: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None):
    """y = [x; x_items] W^T (+ bias) on the matrix cores (include/ppgat.h ppgat_project), with
    s_src = y.att_src and s_dst = y.att_dst fused when att_src is given (heads = 1).
    Returns y (``out`` if given: contiguous [rows, HC]), or (y, s_src, s_dst)."""
    lib = _lib.load()
    _check_dev("x", x, torch.float32)
    _check_dev("weight", weight, torch.float32, x.device)
    if x_items is not None and x.size(0) == 0:
        x, x_items = x_items, None
    split = x.size(0)
    n = split + (x_items.size(0) if x_items is not None else 0)
    if x_items is not None:
        _check_dev("x_items", x_items, torch.float32, x.device)
    K, HC = weight.size(1), weight.size(0)
    dev = x.device
    y = out if out is not None else torch.empty(n, HC, dtype=torch.float32, device=dev)
    s_src = s_dst = None
    if att_src is not None:
        s_src = torch.empty(n, dtype=torch.float32, device=dev)
        s_dst = torch.empty(n, dtype=torch.float32, device=dev)
    _lib.check(lib.ppgat_project(x.data_ptr(), x.stride(0) if x.dim() == 2 and split > 1 else K, _lib.ptr(x_items),
                                 (x_items.stride(0) if x_items.size(0) > 1 else K) if x_items is not None else 0,
                                 split, n, K, weight.data_ptr(), weight.stride(0), HC, _lib.ptr(bias),
                                 _lib.ptr(att_src), _lib.ptr(att_dst), y.data_ptr(), HC, _lib.ptr(s_src),
                                 _lib.ptr(s_dst), _lib.stream_handle(dev)), "project")
    return y if att_src is None else (y, s_src, s_dst)


def weight_grads(G, GV, W, a_s, a_d, heads: int, C: int):
    """dW, datt_src, datt_dst from G = dh_msg^T x and GV = [ds_src; ds_dst]^T x (ppgat_weight_grads)."""
    lib = _lib.load()
    HC, K = W.shape
    dev = W.device
    dW = torch.empty(HC, K, dtype=torch.float32, device=dev)
    datt_src = torch.empty(heads, C, dtype=torch.float32, device=dev)
    datt_dst = torch.empty(heads, C, dtype=torch.float32, device=dev)
    _lib.check(lib.ppgat_weight_grads(G.data_ptr(), GV.data_ptr(), W.data_ptr(), a_s.data_ptr(), a_d.data_ptr(), heads,
                                      C, K, dW.data_ptr(), datt_src.data_ptr(), datt_dst.data_ptr(),
                                      _lib.stream_handle(dev)), "weight_grads")
    return dW, datt_src, datt_dst


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
        lib = _lib.load()
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
        if (heads == 1 and HC == K and bool(lib.ppgat_project_bwd_fused_supported(K)) and _fused_dxw_enabled()
                and not (_async_wgrad_enabled() and _grad_free(ctx.params))):
            # dx and D^T x, S^T x in one pass over D and x (ppgat_project_bwd_fused)
            dx = torch.empty(N, K, dtype=torch.float32, device=dev) if need_dx else None
            G = torch.empty(HC, K, dtype=torch.float32, device=dev)
            GV = torch.empty(2, K, dtype=torch.float32, device=dev)
            ws, nbytes = _lib.workspace(lib.ppgat_project_bwd_fused_workspace_bytes, N, device=dev, floor=1)
            x0, x1, sp = (x, xi, split) if seg else (x, None, N)
            if seg and split == 0:  # no user rows: every row from the item segment
                x0, x1, sp = xi, None, N
            prod = ctx.producer
            if prod is not None and dx is not None and prod.pro_state is not None:
                # also the producer layer's prologue: its nstate and dbias from dx (= its grad_out)
                pb, ps_dst, pm, pinv_l = prod.pro_state
                p_nstate = torch.empty(N, 1, 4, dtype=torch.float32, device=dev)
                p_dbias = torch.empty(K, dtype=torch.float32, device=dev) if pb is not None else None
                _lib.check(lib.ppgat_project_bwd_fused_producer(
                    D.data_ptr(), HC, S.data_ptr(), 2, x0.data_ptr(), K, _lib.ptr(x1), K, sp, N, K, W.data_ptr(), K,
                    a_s.data_ptr(), a_d.data_ptr(), dx.data_ptr(), K, G.data_ptr(), GV.data_ptr(), _lib.ptr(pb),
                    ps_dst.data_ptr(), pm.data_ptr(), pinv_l.data_ptr(), 1.0, p_nstate.data_ptr(), _lib.ptr(p_dbias),
                    ws.data_ptr(), nbytes, _lib.stream_handle(dev)), "project_bwd_fused_producer")
                prod.pro_result = (weakref.ref(dx), dx._version, p_nstate, p_dbias)
            else:
                _lib.check(lib.ppgat_project_bwd_fused(D.data_ptr(), HC, S.data_ptr(), 2, x0.data_ptr(), K,
                                                       _lib.ptr(x1), K, sp, N, K, W.data_ptr(), K, a_s.data_ptr(),
                                                       a_d.data_ptr(), _lib.ptr(dx), K, G.data_ptr(), GV.data_ptr(),
                                                       ws.data_ptr(), nbytes, _lib.stream_handle(dev)),
                           "project_bwd_fused")
            dW, datt_src, datt_dst = weight_grads(G, GV, W, a_s, a_d, heads, C)
            dx_u = dx[:split] if (dx is not None and had_items) else dx
            dx_i = dx[split:] if (dx is not None and had_items) else None
            return (dx_u, dW, datt_src.view(ctx.att_shapes[0]), datt_dst.view(ctx.att_shapes[1]), dbias,
                    None, None, None, None, None, None, None, dx_i, None, dv, None)
        if need_dx:
            if heads == 1 and project_supported(HC, K):  # reduction over HC, K output columns
                dx = torch.empty(N, K, dtype=torch.float32, device=dev)
                _lib.check(lib.ppgat_project_bwd_input(D.data_ptr(), HC, N, HC, W.data_ptr(), K, K, a_s.data_ptr(),
                                                       a_d.data_ptr(), S.data_ptr(), 2, dx.data_ptr(), K,
                                                       _lib.stream_handle(dev)), "project_bwd_input")
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
            global KINK_TAP
            xx = join_rows(x, x_items) if x_items is not None else x
            tap, KINK_TAP = KINK_TAP, None  # the instrumentation records the layer's own forward only
            try:
                _, st = xgat_forward(xx, W, a_s, a_d, None, XViews.of_graph(graph), heads, channels, slope, 0.0, 0,
                                     keep_agg=False)
            finally:
                KINK_TAP = tap
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


# ---------------------------------------------------------------------------
# projection with the MFMA weight-gradient kernel, and the fused BPR/BCE loss
# ---------------------------------------------------------------------------
_CONST_BOUNDS = {}


def _const_colmax(t: torch.Tensor) -> torch.Tensor:
    """colmax_abs(t) for a tensor the step does not change (the item features of the config-5
    projection's weight gradient): computed once per (tensor object, version, storage and data
    pointers, shape), so the column-max pass over it leaves the training step.  Only tensors the
    step does not differentiate reach it (_Linear's ``x_const``); a raw-pointer write that keeps
    all of these is the caller's to avoid."""
    key = (t._version, t.data_ptr(), t.untyped_storage().data_ptr(), tuple(t.shape), tuple(t.stride()))
    e = _CONST_BOUNDS.get(id(t))
    if e is not None and e[0]() is t and e[1] == key:
        return e[2]
    bits = colmax_abs(t)
    for k in [k for k, v in _CONST_BOUNDS.items() if v[0]() is None]:
        del _CONST_BOUNDS[k]
    _CONST_BOUNDS[id(t)] = (weakref.ref(t), key, bits)
    return bits


def gemm_tn(A: torch.Tensor, B: torch.Tensor, want_colsum: bool = False, V: Optional[torch.Tensor] = None,
            B_items: Optional[torch.Tensor] = None, b_const: bool = False):
    """A [N,M], B [N,K] (row strides may exceed the widths) -> (A^T B [M,K], colsum(A) [M]
    or None, V^T B [nv,K] or None), deterministic.  With ``B_items`` the B rows are
    cat(B, B_items) (two row segments, not concatenated).  ``b_const``: B does not change between
    calls (its column bound for the fp16 TN kernel is cached, _const_colmax)."""
    lib = _lib.load()
    for name, t in (("A", A), ("B", B)) + ((("B_items", B_items),) if B_items is not None else ()):
        _require(isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32,
                 f"gemm_tn: {name} must be an fp32 ROCm tensor")
        _require(t.dim() == 2 and t.stride(1) == 1, f"gemm_tn: {name} must be 2-D with unit column stride")
    split = B.size(0)
    nb = split + (B_items.size(0) if B_items is not None else 0)
    _require(A.size(0) == nb, "gemm_tn: A [N,M], B [N,K]")
    if A.size(1) == 0 or B.size(1) == 0 or nb == 0:  # empty product or empty reduction: zeros
        M0, K0, nv0 = A.size(1), B.size(1), (0 if V is None else V.size(1))
        z = A.new_zeros
        return z(M0, K0), (z(M0) if want_colsum else None), (z(nv0, K0) if nv0 else None)
    if not all(_aligned_rows(t) for t in (A, B) + ((B_items,) if B_items is not None else ())):
        # the kernels read 16-byte row segments: zero-pad the columns of any operand whose rows
        # are not 16-byte aligned (e.g. the [B, B] logit gradient of a ragged InfoNCE batch);
        # the zero columns only add output rows / columns that are dropped here
        M0, K0 = A.size(1), B.size(1)
        out, cs, vout = gemm_tn(_pad_cols4(A), _pad_cols4(B), want_colsum, V,
                                _pad_cols4(B_items) if B_items is not None else None)
        return (out[:M0, :K0].contiguous(), cs[:M0].contiguous() if cs is not None else None,
                vout[:, :K0].contiguous() if vout is not None else None)
    N, M, K = A.size(0), A.size(1), B.size(1)
    nv = 0 if V is None else V.size(1)
    if B_items is None and M * K > 128 * 128 and gemm_tn_big_supported(M, K):
        # beyond one 128 x 128 tile (config 5: 1024 x 256 over 1.9M rows): the matrix-core TN
        # kernel (ppgat_gemm_tn_big); column sums and V^T B through the small kernels
        bb = (_const_colmax(B), K, 1.0) if b_const else None
        if want_colsum:  # colsum(A) from the same pass over A
            out, cs = gemm_tn_big(A, B, b_bound=bb, want_colsum=True)
        else:
            out, cs = gemm_tn_big(A, B, b_bound=bb), None
        vout = None
        if nv:  # V^T B by the small kernel, V padded to a multiple of 4 columns (16-byte rows)
            Vp = torch.zeros(N, (nv + 3) // 4 * 4, dtype=torch.float32, device=A.device)
            Vp[:, :nv] = V
            vout = gemm_tn(Vp, B)[0][:nv].contiguous()
        return out, cs, vout
    if V is not None:
        _require(V.is_cuda and V.dtype == torch.float32 and V.dim() == 2 and V.stride(1) == 1 and V.size(0) == N,
                 "gemm_tn: V must be fp32 [N, nv] with unit column stride")
    out = torch.empty(M, K, dtype=torch.float32, device=A.device)
    cs = torch.empty(M, dtype=torch.float32, device=A.device) if want_colsum else None
    vout = torch.empty(max(nv, 1), K, dtype=torch.float32, device=A.device) if nv else None
    ws, nbytes = _lib.workspace(lib.ppgat_gemm_tn_workspace_bytes, N, M, K, nv, device=A.device)
    lda = A.stride(0) if N > 1 else max(M + (-M) % 4, 4)
    ldb = B.stride(0) if split > 1 else max(K + (-K) % 4, 4)
    ldv = (V.stride(0) if N > 1 else nv) if nv else 0
    if B_items is not None:
        ldb1 = B_items.stride(0) if B_items.size(0) > 1 else max(K + (-K) % 4, 4)
        _lib.check(lib.ppgat_gemm_tn_seg(A.data_ptr(), lda, B.data_ptr(), ldb, B_items.data_ptr(), ldb1, split, N, M,
                                         K, out.data_ptr(), _lib.ptr(cs), _lib.ptr(V) if nv else None, ldv, nv,
                                         _lib.ptr(vout), ws.data_ptr(), nbytes, _lib.stream_handle(A.device)),
                   "gemm_tn")
    else:
        _lib.check(lib.ppgat_gemm_tn(A.data_ptr(), lda, B.data_ptr(), ldb, N, M, K, out.data_ptr(), _lib.ptr(cs),
                                     _lib.ptr(V) if nv else None, ldv, nv, _lib.ptr(vout), ws.data_ptr(),
                                     nbytes, _lib.stream_handle(A.device)), "gemm_tn")
    return out, cs, vout


class _Linear(torch.autograd.Function):
    """y = x W^T + b on the matrix cores: the fused 128-column projection (ppgat_project) or
    the general GEMM (ppgat_gemm_nn, config 5's 256-wide layers; other widths zero-padded by
    ``mm_nn``); dx by ppgat_gemm_nn, dW (and db) through ppgat_gemm_tn (N = 10^5..10^7 rows
    split over the chip).  No vendor BLAS on any shape."""

    @staticmethod
    def forward(ctx, x, weight, bias, out_holder=None):
        # no gradient reached the output (the halo partition's locally computed halo item rows,
        # whose gradients are their owners' business): skip the backward instead of running it on
        # a materialised zero gradient (a zero fill, two column-max passes and a TN GEMM over the
        # 2.8M halo rows per step at world 8 on config 5)
        ctx.set_materialize_grads(False)
        x_const = not x.requires_grad  # (an input the step does not differentiate: the item features)
        x = x.contiguous()
        ctx.save_for_backward(x, weight)
        ctx.x_keep = x if x_const else None  # the object itself: its cached column bound is found by identity
        ctx.has_bias = bias is not None
        W = weight.detach().contiguous()
        b = bias.detach().contiguous() if bias is not None else None
        out = out_holder[0] if out_holder is not None else None  # (in a list: a buffer, not an autograd input)
        if project_supported(x.size(1), weight.size(0)):
            return project(x, W, b, out=out)
        elif gemm_nn_supported(x.size(0), x.size(1), weight.size(0), 1):
            return gemm_nn(x, W, 1, weight.size(0), bias=b, out=out)
        else:
            y = mm_nn(x, W, 1, weight.size(0), bias=b)
        return y if out is None else out.copy_(y)

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return None, None, None, None
        x, weight = ctx.saved_tensors
        g = g.contiguous()
        dx = None
        if ctx.needs_input_grad[0]:
            W = weight.detach().contiguous()
            if gemm_nn_supported(g.size(0), g.size(1), W.size(1), 0):
                dx = gemm_nn(g, W, 0, W.size(1))
            else:
                dx = mm_nn(g, W, 0, W.size(1))
        dW = db = None
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            xk = ctx.x_keep
            dW, db, _ = gemm_tn(g, xk if xk is not None else x, want_colsum=ctx.has_bias, b_const=xk is not None)
        return dx, dW, db if ctx.has_bias else None, None


def linear(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None,
           out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x W^T + b; with ``out`` (contiguous [rows, out_features]) written there and returned."""
    _require(x.is_cuda, "linear: ppgat runs on ROCm devices only; there is no CPU path")
    if x.dtype != torch.float32 or x.dim() != 2:
        raise NotImplementedError("ppgat linear: fp32 2-D input only")
    if out is not None:
        _require(out.is_cuda and out.dtype == torch.float32 and out.is_contiguous()
                 and out.shape == (x.size(0), weight.size(0)), "linear: out must be contiguous [rows, out_features]")
    return _Linear.apply(x, weight, bias, [out] if out is not None else None)


class _JoinRows(torch.autograd.Function):
    """cat([a, b]) of two row blocks that already lie back to back in one storage: the joined
    tensor is a new header on that storage (no copy); the gradient splits at the seam."""

    @staticmethod
    def forward(ctx, a, b):
        ctx.n = a.size(0)
        return a.new_empty(0).set_(a.untyped_storage(), a.storage_offset(), (a.size(0) + b.size(0), a.size(1)),
                                   (a.size(1), 1))

    @staticmethod
    def backward(ctx, g):
        return g[:ctx.n], g[ctx.n:]


def rows_adjacent(a: torch.Tensor, b: torch.Tensor) -> bool:
    """b's rows start where a's end, in one storage, both contiguous with the same width."""
    return (a.dim() == 2 and b.dim() == 2 and a.size(1) == b.size(1) and a.dtype == b.dtype and a.device == b.device
            and a.is_contiguous() and b.is_contiguous()
            and a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr()
            and b.storage_offset() == a.storage_offset() + a.numel())


def join_rows(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """torch.cat([a, b], 0), without the copy when the blocks are adjacent (model.node_table)."""
    return _JoinRows.apply(a, b) if rows_adjacent(a, b) else torch.cat([a, b], 0)


class _EmbeddingRows(torch.autograd.Function):
    """weight.index_select(0, idx) whose gradient for ``weight`` is row-sparse: a COO tensor with
    ``idx`` as its one sparse dimension and the incoming rows as its values -- no zero-filled
    [n_rows, d] gradient.  Not flagged coalesced: repeated ids in ``idx`` stay separate entries
    (they add on coalesce(), as index_select's backward adds them)."""

    @staticmethod
    def forward(ctx, weight, idx):
        ctx.save_for_backward(idx)
        ctx.shape = weight.shape
        return weight.index_select(0, idx)

    @staticmethod
    def backward(ctx, g):
        (idx,) = ctx.saved_tensors
        return torch.sparse_coo_tensor(idx[None], g.contiguous(), ctx.shape), None


def embedding_rows(weight: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """``weight.index_select(0, idx)`` for a 2-D table and int64 ``idx``, with a row-sparse gradient
    (``optim.Adam`` takes it: the lazy row step).  Pure torch on any device; launches no kernel."""
    _require(weight.dim() == 2 and idx.dim() == 1 and idx.dtype == torch.int64,
             "embedding_rows: weight [n, d] and int64 idx [k] expected")
    return _EmbeddingRows.apply(weight, idx)


# ---------------------------------------------------------------------------
# general fp32 matrix-core GEMMs (include/ppgat.h ppgat_gemm_nn / ppgat_gemm_tn_big)
# ---------------------------------------------------------------------------
def gemm_nn_supported(m: int, k: int, n: int, b_layout: int) -> bool:
    return bool(_lib.load().ppgat_gemm_nn_supported(int(m), int(k), int(n), int(b_layout)))


def gemm_nn(x: torch.Tensor, B: torch.Tensor, b_layout: int, n: int, alpha: float = 1.0,
            bias: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
            rank: Optional[tuple] = None) -> torch.Tensor:
    """alpha x B (+ bias): B [K, n] row-major (b_layout 0) or [n, K] (b_layout 1: x B^T).
    rank=(S [M, nv], A [nv, n]): + S A as well (ppgat_gemm_nn_rank; in the GEMM's epilogue on
    the large-M fp16 path, the same bits as gemm_nn followed by rank_update_)."""
    lib = _lib.load()
    _check_rows("x", x, torch.float32)
    _check_rows("B", B, torch.float32, x.device)
    M, K = x.shape
    y = out if out is not None else torch.empty(M, n, dtype=torch.float32, device=x.device)
    ldb = B.stride(0)
    nbytes = ctypes.c_size_t(0)
    if gemm_nn_supported(M, K, n, b_layout):
        _lib.check(lib.ppgat_gemm_nn_workspace_bytes(M, K, n, ctypes.byref(nbytes)), "gemm_nn_workspace_bytes")
    ws = torch.empty(int(nbytes.value), dtype=torch.uint8, device=x.device) if nbytes.value else None
    ldx, ldy = (x.stride(0) if M > 1 else K), (y.stride(0) if M > 1 else n)
    if rank is not None:
        S, A = rank
        nv = S.size(1)
        _require(S.dim() == 2 and S.size(0) == M and S.stride(1) == 1 and A.is_contiguous() and A.shape == (nv, n),
                 "gemm_nn: rank=(S [M, nv], A [nv, n] contiguous)")
        _lib.check(lib.ppgat_gemm_nn_rank(x.data_ptr(), ldx, M, K, B.data_ptr(), ldb, b_layout, n, float(alpha),
                                          _lib.ptr(bias), S.data_ptr(), S.stride(0) if M > 1 else nv, nv, A.data_ptr(),
                                          n, y.data_ptr(), ldy, _lib.ptr(ws), nbytes.value,
                                          _lib.stream_handle(x.device)), "gemm_nn_rank")
        return y
    _lib.check(lib.ppgat_gemm_nn_ws(x.data_ptr(), ldx, M, K, B.data_ptr(), ldb, b_layout, n,
                                    float(alpha), _lib.ptr(bias), y.data_ptr(), ldy,
                                    _lib.ptr(ws), nbytes.value, _lib.stream_handle(x.device)), "gemm_nn")
    return y


def _aligned_rows(t: torch.Tensor) -> bool:
    return t.dim() == 2 and t.stride(1) == 1 and (t.size(0) <= 1 or t.stride(0) % 4 == 0) and t.data_ptr() % 16 == 0


def _pad_cols4(t: torch.Tensor) -> torch.Tensor:
    """``t`` itself when its rows are 16-byte aligned, else a copy with its columns zero-padded
    to a multiple of 4."""
    if _aligned_rows(t):
        return t
    n, c = t.shape
    tp = torch.zeros(n, c + (-c) % 4, dtype=t.dtype, device=t.device)
    tp[:, :c] = t
    return tp


def mm_nn(x: torch.Tensor, B: torch.Tensor, b_layout: int, n: int, alpha: float = 1.0,
          bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """alpha x B (+ bias) for ANY shape on ppgat_gemm_nn: the reduction width is zero-padded to
    a multiple of 32 and the output width to a multiple of 128 where the kernel needs it (the
    padding adds exact zeros, so the result is the unpadded product).  B [K, n] (b_layout 0)
    or [n, K] (b_layout 1, i.e. x B^T).  No vendor BLAS on any shape."""
    _require(x.is_cuda and x.dtype == torch.float32 and x.dim() == 2, "mm_nn: x must be a 2-D fp32 ROCm tensor")
    M, K = x.shape
    if M == 0:
        return torch.zeros(0, n, dtype=torch.float32, device=x.device)
    Kp, Np = -(-max(K, 1) // 32) * 32, -(-max(n, 1) // 128) * 128
    if Kp != K or not _aligned_rows(x):
        xp = torch.zeros(M, Kp, dtype=torch.float32, device=x.device)
        xp[:, :K] = x
        x = xp
    B = B.detach()
    if Kp != K or Np != n or not _aligned_rows(B):
        Bp = torch.zeros((Kp, Np) if b_layout == 0 else (Np, Kp), dtype=torch.float32, device=x.device)
        if b_layout == 0:
            Bp[:K, :n] = B
        else:
            Bp[:n, :K] = B
        B = Bp
    if bias is not None and Np != n:
        bias = torch.cat([bias.detach().reshape(-1), bias.new_zeros(Np - n)])
    y = gemm_nn(x, B, b_layout, Np, alpha=alpha, bias=bias.detach().contiguous() if bias is not None else None)
    return y if Np == n else y[:, :n].contiguous()


def att_proj(W: torch.Tensor, a_s: torch.Tensor, a_d: torch.Tensor, heads: int, channels: int) -> torch.Tensor:
    """[2H, K] = [W_h^T att_src[h]; W_h^T att_dst[h]] (ppgat_att_proj)."""
    lib = _lib.load()
    K = W.size(1)
    A = torch.empty(2 * heads, K, dtype=torch.float32, device=W.device)
    _lib.check(lib.ppgat_att_proj(W.data_ptr(), a_s.data_ptr(), a_d.data_ptr(), heads, channels, K, A.data_ptr(),
                                  _lib.stream_handle(W.device)), "att_proj")
    return A


def rank_update_(dx: torch.Tensor, S: torch.Tensor, A: torch.Tensor) -> torch.Tensor:
    """dx += S A in place (ppgat_rows_rank_update; S [n, nv] with nv <= 16, A [nv, K])."""
    lib = _lib.load()
    n, K = dx.shape
    nv = S.size(1)
    _require(K % 4 == 0 and _aligned_rows(dx) and A.is_contiguous() and S.stride(1) == 1 and nv <= 16,
             "rank_update_: dx rows 16-byte aligned with K % 4 == 0, nv <= 16")
    _lib.check(lib.ppgat_rows_rank_update(S.data_ptr(), S.stride(0) if n > 1 else nv, nv, A.data_ptr(), K, n, K,
                                          dx.data_ptr(), dx.stride(0) if n > 1 else K, _lib.stream_handle(dx.device)),
               "rows_rank_update")
    return dx


def gemm_tn_big_supported(ma: int, nb: int) -> bool:
    return ma % 128 == 0 and nb % 128 == 0 and ma >= 128 and nb >= 128


def colmax_abs(X: torch.Tensor, src_ptr: Optional[torch.Tensor] = None) -> torch.Tensor:
    """IEEE bits (int32 view) of max_i |X[i, c]| per column (ppgat_colmax_abs; deterministic);
    with ``src_ptr`` (CSC pointers [n + 1]) over the rows that are an edge's source only
    (ppgat_colmax_abs_sources)."""
    lib = _lib.load()
    _check_rows("X", X, torch.float32)
    n, c = X.shape
    out = torch.empty(c, dtype=torch.int32, device=X.device)
    ld = X.stride(0) if n > 1 else c
    if src_ptr is not None:
        _check_dev("src_ptr", src_ptr, torch.int32, X.device)
        _require(src_ptr.numel() == n + 1, "colmax_abs: src_ptr must hold n + 1 CSC pointers")
        _lib.check(lib.ppgat_colmax_abs_sources(X.data_ptr(), ld, n, c, src_ptr.data_ptr(), out.data_ptr(),
                                                _lib.stream_handle(X.device)), "colmax_abs_sources")
        return out
    _lib.check(lib.ppgat_colmax_abs(X.data_ptr(), ld, n, c, out.data_ptr(), _lib.stream_handle(X.device)),
               "colmax_abs")
    return out


def gemm_tn_big(A: torch.Tensor, B: torch.Tensor, b_bound=None, a_bits=None, want_colsum: bool = False):
    """A [M, ma]^T B [M, nb] on the matrix cores (ppgat_gemm_tn_big), deterministic.  ``b_bound``
    = (bits [period] from colmax_abs, period, scale >= 1): an upper bound of |B| per column
    (column j: bits[j % period] * scale) that replaces the fp16 kernel's column-max pass over B
    (ppgat_gemm_tn_big_bounded).  ``a_bits`` [ma]: a bound of |A| over the rows whose B row is not
    zero (ppgat_gemm_tn_big_bounds: the other rows are clamped) in place of A's pass.
    ``want_colsum``: returns (out, colsum(A)), the column sums from the same pass over A
    (ppgat_gemm_tn_big_colsum)."""
    lib = _lib.load()
    _check_rows("A", A, torch.float32)
    _check_rows("B", B, torch.float32, A.device)
    M, ma = A.shape
    nb = B.size(1)
    ws, nbytes = _lib.workspace(lib.ppgat_gemm_tn_big_workspace_bytes, M, ma, nb, device=A.device, floor=1)
    out = torch.empty(ma, nb, dtype=torch.float32, device=A.device)
    lda, ldb, st = A.stride(0) if M > 1 else ma, B.stride(0) if M > 1 else nb, _lib.stream_handle(A.device)
    if want_colsum:
        if a_bits is not None:
            _require(a_bits.dtype == torch.int32 and a_bits.numel() == ma and a_bits.device == A.device,
                     "gemm_tn_big: a_bits must be int32 [ma] on A's device")
        bits, period, scale = b_bound if b_bound is not None else (None, 1, 1.0)
        if bits is not None:
            _require(bits.dtype == torch.int32 and bits.numel() == period and bits.device == A.device,
                     "gemm_tn_big: b_bound bits must be int32 [period] on A's device")
        cs = torch.empty(ma, dtype=torch.float32, device=A.device)
        _lib.check(lib.ppgat_gemm_tn_big_colsum(A.data_ptr(), lda, B.data_ptr(), ldb, M, ma, nb, _lib.ptr(a_bits),
                                                _lib.ptr(bits), int(period), float(scale), out.data_ptr(),
                                                cs.data_ptr(), ws.data_ptr(), nbytes, st), "gemm_tn_big_colsum")
        return out, cs
    if a_bits is not None:
        _require(a_bits.dtype == torch.int32 and a_bits.numel() == ma and a_bits.device == A.device,
                 "gemm_tn_big: a_bits must be int32 [ma] on A's device")
        bits, period, scale = b_bound if b_bound is not None else (None, 1, 1.0)
        _lib.check(lib.ppgat_gemm_tn_big_bounds(A.data_ptr(), lda, B.data_ptr(), ldb, M, ma, nb, a_bits.data_ptr(),
                                                _lib.ptr(bits), int(period), float(scale), out.data_ptr(),
                                                ws.data_ptr(), nbytes, st), "gemm_tn_big_bounds")
        return out
    if b_bound is not None:
        bits, period, scale = b_bound
        _require(bits.dtype == torch.int32 and bits.numel() == period and bits.device == A.device,
                 "gemm_tn_big: b_bound bits must be int32 [period] on A's device")
        _lib.check(lib.ppgat_gemm_tn_big_bounded(A.data_ptr(), lda, B.data_ptr(), ldb, M, ma, nb, bits.data_ptr(),
                                                 int(period), float(scale), out.data_ptr(), ws.data_ptr(),
                                                 nbytes, st), "gemm_tn_big_bounded")
        return out
    _lib.check(lib.ppgat_gemm_tn_big(A.data_ptr(), lda, B.data_ptr(), ldb, M, ma, nb, out.data_ptr(), ws.data_ptr(),
                                     nbytes, st), "gemm_tn_big")
    return out


def colsum(Y: torch.Tensor) -> torch.Tensor:
    """Column sums of Y [n, c] (ppgat_colsum over 128- or 256-column slabs; torch for widths not a multiple of 128)."""
    lib = _lib.load()
    _check_rows("Y", Y, torch.float32)
    n, c = Y.shape
    if c not in (128, 256) and c % 256 == 0:  # wider: 256-column slabs
        return torch.cat([colsum(Y[:, s:s + 256]) for s in range(0, c, 256)])
    if c not in (128, 256) and c % 128 == 0:
        return torch.cat([colsum(Y[:, s:s + 128]) for s in range(0, c, 128)])
    if c not in (128, 256):
        return Y.sum(0)
    ws, nbytes = _lib.workspace(lib.ppgat_colsum_workspace_bytes, n, c, device=Y.device, floor=1)
    out = torch.empty(c, dtype=torch.float32, device=Y.device)
    _lib.check(lib.ppgat_colsum(Y.data_ptr(), Y.stride(0) if n > 1 else c, n, c, out.data_ptr(), ws.data_ptr(),
                                nbytes, _lib.stream_handle(Y.device)), "colsum")
    return out


# ---------------------------------------------------------------------------
# multi-head layer, aggregate-then-transform (include/ppgat.h ppgat_xgat_*)
# ---------------------------------------------------------------------------
@dataclass
class XViews:
    """The edge lists the aggregate-then-transform layer runs on: CSR over the n_dst
    destination rows (forward, destination sums) and CSC over the n_src source rows
    (backward edge pass); source ids index x rows [0, n_src)."""
    n_dst: int
    n_src: int
    n_edges: int
    col: torch.Tensor
    csr_eid: torch.Tensor
    fwd_sched: Schedule
    row: torch.Tensor
    csc_eid: torch.Tensor
    dz_slot: torch.Tensor
    bwd_sched: Schedule
    bwd_sched_own: Optional[Schedule] = None   # sources [0, n_dst) (halo partition)
    bwd_sched_halo: Optional[Schedule] = None  # sources [n_dst, n_src), rows relative to n_dst
    # dz_slot None: dz in CSC order, summed per destination through csr2csc
    csr2csc: Optional[torch.Tensor] = None
    rowptr: Optional[torch.Tensor] = None  # CSR row pointers over the destinations (KINK_TAP only)
    colptr: Optional[torch.Tensor] = None  # CSC pointers over the sources [n_src + 1] (agg's column bound)

    @staticmethod
    def of_graph(g: "CSRGraph") -> "XViews":
        return XViews(g.n_nodes, g.n_nodes, g.n_edges, g.col, g.csr_eid, g.fwd_sched, g.row, g.csc_eid, None,
                      g.bwd_sched, csr2csc=_csr2csc(g), rowptr=g.rowptr, colptr=g.colptr)


def xgat_supported(in_channels: int, heads: int, channels: int) -> bool:
    return bool(_lib.load().ppgat_xgat_supported(int(in_channels), int(heads), int(channels)))


@dataclass
class XPhase:
    """One step of a phased aggregate-then-transform forward (dist._HaloLayerX): the destination
    rows [d0, d1) with their schedule (rows relative to d0), the source row ranges whose node
    scores this phase computes first (rows outside the own destination rows, e.g. halo rows that
    have just arrived), ``before()`` (e.g. make the stream wait for those rows' exchange) and
    ``after(out)`` (e.g. start sending the phase's output rows to the peers)."""
    d0: int
    d1: int
    sched: Schedule
    src_ranges: tuple = ()
    before: Optional[Callable] = None
    after: Optional[Callable] = None


def xgat_att_proj(weight, att_src, att_dst, heads: int, C: int) -> torch.Tensor:
    """A [2, H, K]: A_v[h] = W_h^T att_v[h] (ppgat_xgat_weights) -- the node scores are x . A."""
    W = weight.detach().contiguous()
    a_s = att_src.detach().reshape(heads, C).contiguous()
    a_d = att_dst.detach().reshape(heads, C).contiguous()
    A = torch.empty(2, heads, W.size(1), dtype=torch.float32, device=W.device)
    _launch.xgat_weights(W, a_s, a_d, heads, C, A=A)
    return A


def xgat_scores_rows(x_rows, A, s_src, s_dst=None):
    """s_src (and, given, s_dst) [n, H] of the rows x_rows [n, K] (row stride x_rows.stride(0))
    under A [2, H, K] (ppgat_xgat_scores; per row the same arithmetic whatever the launch)."""
    if x_rows.size(0):
        _launch.xgat_scores(x_rows, 0, x_rows.size(0), A, s_src, s_dst)


def xgat_forward(x, weight, att_src, att_dst, bias, v: "XViews", heads: int, C: int, slope: float, p: float,
                 seed: int, phases: Optional[list] = None, out: Optional[torch.Tensor] = None, scores=None,
                 keep_agg: Optional[bool] = None):
    """Forward of the aggregate-then-transform layer; returns (out [n_dst, C], saved state).

    ``phases`` (a list of XPhase partitioning [0, n_dst) in order): the node scores of the
    destination rows first, then per phase its sources' scores, the edge pass over its
    destination rows and their rows of the output GEMM.  Per destination the result is the
    same as the one-phase forward (same per-row kernels and order): bitwise equal.  ``out``: a
    contiguous [n_dst, C] destination (the next halo layer's own rows: no copy there).
    ``scores`` = (s_src [n_src, H], s_dst [>= n_dst, H]): the node scores, already computed
    (the halo partition: the owners computed them with the rows and sent them along, ready by
    each phase's ``before``) -- no score pass here.  ``keep_agg``: keep the aggregates for the
    backward (None: _xgat_keep_agg decides; the halo partition's backward needs them)."""
    x = x.contiguous()
    dev = x.device
    K = x.size(1)
    H = heads
    _require(x.size(0) == v.n_src, f"x has {x.size(0)} rows, the edge lists {v.n_src} sources")
    W = weight.detach().contiguous()
    a_s = att_src.detach().reshape(H, C).contiguous()
    a_d = att_dst.detach().reshape(H, C).contiguous()
    b = bias.detach().contiguous() if bias is not None else None
    A = torch.empty(2, H, K, dtype=torch.float32, device=dev)
    Wt = torch.empty(H * K, C, dtype=torch.float32, device=dev)
    _launch.xgat_weights(W, a_s, a_d, H, C, A=A, Wt=Wt)
    if phases is None:
        phases = [XPhase(0, v.n_dst, v.fwd_sched, ((v.n_dst, v.n_src),) if v.n_src > v.n_dst else ())]
    if scores is not None:
        s_src, s_dst = scores
        _require(s_src.shape == (v.n_src, H) and s_dst.size(0) >= max(v.n_dst, 1) and s_dst.size(1) == H
                 and s_src.is_contiguous() and s_dst.is_contiguous(), "xgat_forward: scores must be [n_src, H], [n_dst, H]")
    else:
        s_src = torch.empty(v.n_src, H, dtype=torch.float32, device=dev)
        s_dst = torch.empty(max(v.n_dst, 1), H, dtype=torch.float32, device=dev)
        # the destination rows' scores (s_src and s_dst), then each phase's other sources
        _launch.xgat_scores(x, 0, v.n_dst, A, s_src, s_dst)
    agg = torch.empty(v.n_dst, H, K, dtype=torch.float32, device=dev)
    m = torch.empty(v.n_dst, H, dtype=torch.float32, device=dev)
    inv_l = torch.empty(v.n_dst, H, dtype=torch.float32, device=dev)
    if out is None:
        out = torch.empty(v.n_dst, C, dtype=torch.float32, device=dev)
    _require(out.shape == (v.n_dst, C) and out.is_contiguous(), "xgat_forward: out must be contiguous [n_dst, C]")
    seed_buf = seed_buffer(p, dev)
    E = v.n_edges
    # column maxima of |x| over the rows the edge pass gathers (every source): the weight
    # gradient's bound of |agg| (_xgat_weight_grads), with no pass of its own over x
    xbits = torch.zeros(K, dtype=torch.int32, device=dev)
    for ph in phases:
        if ph.before is not None:
            ph.before()
        for r0, r1 in (ph.src_ranges if scores is None else ()):
            if r1 > r0:
                _launch.xgat_scores(x, r0, r1 - r0, A, s_src)
        nd = ph.d1 - ph.d0
        _launch.xgat_fwd_colmax(ph.sched, v, ph.d0, nd, x, s_src, s_dst, slope, p, seed, seed_buf, agg, m, inv_l,
                                xbits)
        if nd > 0:
            gemm_nn(agg[ph.d0:ph.d1].view(nd, H * K), Wt, 0, C, alpha=1.0 / H, bias=b, out=out[ph.d0:ph.d1])
        if ph.after is not None:
            ph.after(out)
    _tap_kinks(v.rowptr, v.col, v.csr_eid, s_src, s_dst, H)
    if not (keep_agg if keep_agg is not None else _xgat_keep_agg(v.n_dst, v.n_src, H, K, C, dev, E)):
        agg = None  # the backward's weight gradient comes from acc^T x (_xgat_weight_grads)
    saved = dict(x=x, W=W, a_s=a_s, a_d=a_d, A=A, s_src=s_src, s_dst=s_dst, agg=agg, m=m, inv_l=inv_l,
                 seed_buf=seed_buf, v=v, xbits=xbits, meta=(H, C, K, slope, p, seed, bias is not None))
    return out, saved


def _xgat_keep_agg(n_dst: int, n_src: int, H: int, K: int, C: int, dev, n_edges: int = 0) -> bool:
    """Whether the forward's aggregates agg [n_dst, H, C_in] stay alive for the backward's weight
    gradient G = g^T agg.  The same G is acc^T x (permuted): G[c, (h, k)] = sum_i g_i[c] agg^h_i[k]
    = sum_i sum_j beta^h_ij g_i[c] x_j[k] = sum_j acc^h_j[c] x_j[k], and the default backward
    builds acc [n_src, H, C] anyway -- so agg is only worth keeping while memory is not short: the
    acc^T x form costs an exact column-max pass over acc (4 H C bytes per source) instead of one
    over g (4 C per destination).  PPGAT_XGAT_AGG=keep / free forces a form; by default agg is
    dropped when four tensors of its size -- two layers' agg, the backward's hs and acc -- would
    take more than half of the device's memory: the whole 200M-edge graph on one GPU (61 GB each;
    tools/mem_probe.py: the agg-free step's peak is 239 GB there), not its 1/8 share (7.7 GB)."""
    mode = os.environ.get("PPGAT_XGAT_AGG", "auto")
    if mode == "keep":
        return True
    if _xgat_gather_mode(C, H, n_src, n_dst, n_edges, K) != "gd":  # the backward's own choice, same inputs
        return True  # the gt / g passes read agg in their prologue
    if mode == "free":
        return False
    total = torch.cuda.get_device_properties(dev).total_memory
    return 4 * (4.0 * H * max(K, C) * max(n_dst, n_src)) <= 0.5 * total


def xgat_backward(saved: dict, g: torch.Tensor, want_bias_grad: bool, halo_hook=None):
    """Backward of the aggregate-then-transform layer -> (dx [n_src, C_in], dW, datt_src [H, C],
    datt_dst [H, C], dbias).  With ``halo_hook`` and a view split into own sources [0, n_own)
    and halo sources (XViews.bwd_sched_own / bwd_sched_halo), the halo rows' input gradients
    are finished first and handed to halo_hook(dx_halo) -- which starts returning them to
    their owners -- before the own rows' edge pass and the weight-gradient GEMMs run."""
    x, W, a_s, a_d, A = saved["x"], saved["W"], saved["a_s"], saved["a_d"], saved["A"]
    s_src, s_dst, agg, m, inv_l, v = saved["s_src"], saved["s_dst"], saved["agg"], saved["m"], saved["inv_l"], saved["v"]
    H, C, K, slope, p, seed, has_bias = saved["meta"]
    dev = x.device
    g = g.contiguous()
    E = v.n_edges
    S = torch.zeros(v.n_src, 2 * H, dtype=torch.float32, device=dev)
    dz = torch.empty(max(E, 1) * H, dtype=torch.float32, device=dev)
    nstate = torch.empty(max(v.n_dst, 1), H, 4, dtype=torch.float32, device=dev)
    mode = _xgat_gather_mode(C, H, v.n_src, v.n_dst, E, K)
    if mode == "gd":
        return _xgat_backward_deferred_d(saved, g, S, dz, nstate, want_bias_grad, halo_hook)
    Wg = torch.empty(C, H * K, dtype=torch.float32, device=dev)
    _launch.xgat_weights(W, None, None, H, C, Wg=Wg)
    gt = gemm_nn(g, Wg, 0, H * K)
    _launch.xgat_bwd_prologue(gt, agg, s_dst, m, inv_l, v.n_dst, K, H, nstate)
    if mode == "g":
        # gather g_i per edge (C floats) instead of gt_i (H * C_in): hs = x W^T / H per source,
        # the per-head message gradient acc [n_src, H * C], then dx = acc W / H + S A_att with the
        # attention terms in the GEMM's epilogue
        hs = gemm_nn(x, W, 1, H * C, alpha=1.0 / H)
        acc = torch.empty(v.n_src, H * C, dtype=torch.float32, device=dev)
        dx = torch.empty(v.n_src, K, dtype=torch.float32, device=dev)
        A2 = A.view(2 * H, K)
        gargs = (hs, s_src, nstate, g, acc, S, dz, H, C, slope, p, seed, saved["seed_buf"])
        n0 = v.n_dst
        if halo_hook is not None and v.bwd_sched_halo is not None:
            # the halo sources first: their rows of dx (no destination terms) go back to their
            # owners while the own sources' edge pass runs
            _launch.xgat_bwd_edges_g(v.bwd_sched_halo, v, n0, *gargs)
            if v.n_src > n0:
                gemm_nn(acc[n0:], W, 0, K, alpha=1.0 / H, out=dx[n0:], rank=(S[n0:, :H], A2[:H]))
            halo_hook(dx[n0:])
            _launch.xgat_bwd_edges_g(v.bwd_sched_own, v, 0, *gargs)
            _xgat_dst_sum(v, dz, S[:, H:], H)
            gemm_nn(acc[:n0], W, 0, K, alpha=1.0 / H, out=dx[:n0], rank=(S[:n0], A2))
        else:
            _launch.xgat_bwd_edges_g(v.bwd_sched, v, 0, *gargs)
            _xgat_dst_sum(v, dz, S[:, H:], H)
            gemm_nn(acc, W, 0, K, alpha=1.0 / H, out=dx, rank=(S, A2))  # + sum_h ds_src^h A_src^h + ds_dst^h A_dst^h
            if halo_hook is not None:
                halo_hook(dx[n0:])
        del hs, acc
        return _xgat_weight_grads(None, saved, g, S, dx, want_bias_grad, None)
    dx = torch.empty(v.n_src, K, dtype=torch.float32, device=dev)
    args = (x, s_src, nstate, gt, A, S, dz, dx, H, slope, p, seed, saved["seed_buf"])
    if halo_hook is not None and v.bwd_sched_halo is not None:
        _launch.xgat_bwd_edges(v.bwd_sched_halo, v, v.n_dst, *args)
        halo_hook(dx[v.n_dst:])
        _launch.xgat_bwd_edges(v.bwd_sched_own, v, 0, *args)
    else:
        _launch.xgat_bwd_edges(v.bwd_sched, v, 0, *args)
        if halo_hook is not None:
            halo_hook(dx[v.n_dst:])
    _xgat_dst_sum(v, dz, S[:, H:], H)
    _launch.xgat_bwd_epilogue(S, A, v.n_dst, H, dx)
    return _xgat_weight_grads(None, saved, g, S, dx, want_bias_grad, None)


def _xgat_bytes(mode: str, n_src: int, n_dst: int, n_edges: int, C: int, H: int, K: int) -> float:
    """HBM bytes of one multi-head layer backward per formulation: per edge the
    gathered row (g_i: 4C, or gt_i: 4HK) and the per-edge terms; per source the hs and acc rows
    of the g-gathering passes (written, read back: 4 x 4HC) and x / dx (2 x 4K), or x / dx only;
    per destination the gt GEMM and its prologue (3 x 4HK) in the gt-gathering pass."""
    if mode == "gt":
        return n_edges * (4 + 24 * H + 4 * H * K) + n_dst * 12 * H * K + n_src * 8 * K
    return n_edges * (4 + 24 * H + 4 * C) + n_src * (8 * K + 16 * H * C)


def _xgat_gather_mode(C: int, H: int, n_src: Optional[int] = None, n_dst: Optional[int] = None,
                      n_edges: Optional[int] = None, K: Optional[int] = None) -> str:
    """Which multi-head backward runs (read per call): "gd" gathers g_i per edge and defers D (no
    gt GEMM: ppgat_xgat_bwd_edges_gd + D by a destination sum + ppgat_xgat_bwd_dz); "g" gathers
    g_i with D from the gt GEMM's prologue (ppgat_xgat_bwd_edges_g); "gt" gathers gt_i
    (ppgat_xgat_bwd_edges, round 2's pass).  DESIGN.md §4.2.  PPGAT_XGAT_GATHER picks one; by
    default "gd", except where the layer's sources far outnumber its destinations (the halo
    partition at 8 ranks: 11M local rows for 1.9M own) and the g-gathering passes' per-source
    GEMMs would move more bytes than gathering gt_i per edge (_xgat_bytes)."""
    if C != 256 or H not in (2, 4):
        return "gt"
    mode = os.environ.get("PPGAT_XGAT_GATHER")
    if mode in ("g", "gt", "gd"):
        return mode
    if n_src is not None and n_src > n_dst and \
            _xgat_bytes("gt", n_src, n_dst, n_edges, C, H, K) < _xgat_bytes("gd", n_src, n_dst, n_edges, C, H, K):
        return "gt"
    return "gd"


def _xgat_backward_deferred_d(saved: dict, g, S, dz, nstate, want_bias_grad: bool, halo_hook):
    """The default multi-head backward: D^h_i = sum_j beta dalpha from the edge
    pass itself instead of gt^h_i . agg^h_i, so neither gt = g W_grad nor its prologue runs."""
    x, W, A = saved["x"], saved["W"], saved["A"]
    s_src, s_dst, m, inv_l, v = saved["s_src"], saved["s_dst"], saved["m"], saved["inv_l"], saved["v"]
    H, C, K, slope, p, seed, has_bias = saved["meta"]
    dev = x.device
    E = v.n_edges
    n0 = v.n_dst
    seed_buf = saved["seed_buf"]
    _launch.xgat_nstate(s_dst, m, inv_l, None, n0, H, nstate)
    hs = gemm_nn(x, W, 1, H * C, alpha=1.0 / H)
    acc = torch.empty(v.n_src, H * C, dtype=torch.float32, device=dev)
    pdal = torch.empty(max(E, 1) * H, dtype=torch.float32, device=dev)
    gbits = torch.zeros(C, dtype=torch.int32, device=dev)  # |g| over the gathered rows: the G product's A bound
    split = halo_hook is not None and v.bwd_sched_halo is not None
    scheds = [(v.bwd_sched_halo, n0), (v.bwd_sched_own, 0)] if split else [(v.bwd_sched, 0)]
    for sched, base in scheds:  # dalpha (into dz) and beta dalpha per edge, acc per source
        _launch.xgat_bwd_edges_gd_colmax(sched, v, base, hs, s_src, nstate, g, acc, dz, pdal, gbits, H, C, slope, p,
                                         seed, seed_buf)
    del hs
    D = torch.empty(max(n0, 1), H, dtype=torch.float32, device=dev)
    _xgat_dst_sum(v, pdal, D, H)  # D_i = sum_j beta dalpha
    del pdal
    _launch.xgat_nstate(s_dst, m, inv_l, D, n0, H, nstate)
    dza = (s_src, nstate, dz, S, H, slope, p, seed, seed_buf)  # the dz pass: dz in place over dalpha, ds_src into S
    dx = torch.empty(v.n_src, K, dtype=torch.float32, device=dev)
    A2 = A.view(2 * H, K)
    if split:
        # the halo sources first: their rows of dx (no destination terms) go back to their owners
        # while the own sources' dz pass, the destination sums and the GEMMs run
        _launch.xgat_bwd_dz(v.bwd_sched_halo, v, n0, *dza)
        if v.n_src > n0:
            gemm_nn(acc[n0:], W, 0, K, alpha=1.0 / H, out=dx[n0:], rank=(S[n0:, :H], A2[:H]))
        halo_hook(dx[n0:])
        _launch.xgat_bwd_dz(v.bwd_sched_own, v, 0, *dza)
        _xgat_dst_sum(v, dz, S[:, H:], H)
        gemm_nn(acc[:n0], W, 0, K, alpha=1.0 / H, out=dx[:n0], rank=(S[:n0], A2))
    else:
        _launch.xgat_bwd_dz(v.bwd_sched, v, 0, *dza)
        _xgat_dst_sum(v, dz, S[:, H:], H)
        gemm_nn(acc, W, 0, K, alpha=1.0 / H, out=dx, rank=(S, A2))
        if halo_hook is not None:
            halo_hook(dx[n0:])
    if saved["agg"] is not None:
        del acc
        return _xgat_weight_grads(None, saved, g, S, dx, want_bias_grad, None, gbits=gbits)
    return _xgat_weight_grads(None, saved, g, S, dx, want_bias_grad, None, acc=acc)


def _xgat_dst_sum(v: "XViews", dz, out, H: int):
    """Per-destination sums of dz (per edge and head) into ``out`` [n_dst, H], fixed order: ds_dst
    into the column view S[:, H:], or a table of its own."""
    # a thread per short destination (k_dst_sum_vh_short) pays off on the halo tables' rows of
    # ~2 edges (4 x 1.48 -> 4 x 0.71 ms per step at the world-8 probe); at the share's ~13 it
    # measured slower than 16 lanes per item (0.70 vs 0.54 ms per call, profiles/r06/
    # x13_cfg5_kernel_stats.csv against r05/w43): all items on the 16-lane kernel (same bits)
    _launch.bwd_dst_sum(v.fwd_sched, v.n_dst, v.n_edges, H, dz, v.csr2csc, out, csc=v.dz_slot is None,
                        all_long=v.n_edges > 6 * max(v.n_dst, 1))


def _xgat_weight_grads(lib, saved: dict, g, S, dx, want_bias_grad: bool, st, x_rows=None, xbits=None, acc=None,
                       gbits=None):
    """dW, datt, dbias from G = g^T agg and GV = S^T x (``x_rows``: the rows of x that S covers,
    default all of the layer's source rows; ``xbits``: a column bound of the source rows of x,
    colmax_abs bits -- default the forward's, gathered by its edge pass; ``gbits``: a column bound
    of |g| over the destinations with an in-edge, from the backward's edge pass).  Without a
    saved agg (_xgat_keep_agg): G from ``acc`` [n_src, H * C] as (acc^T x) permuted.
    ``lib`` and ``st`` are not used (the launches find the library and the stream themselves);
    they keep their places for the tools and tests that wrap this function by position."""
    x, W, a_s, a_d, agg, v = saved["x"], saved["W"], saved["a_s"], saved["a_d"], saved["agg"], saved["v"]
    H, C, K, slope, p, seed, has_bias = saved["meta"]
    dev = x.device
    GV = gemm_tn(S, x if x_rows is None else x_rows)[0]
    if agg is None:
        _require(acc is not None and x_rows is None, "xgat weight gradients: no agg saved and no acc given")
        # G'[(h, c), k] = sum_j acc^h_j[c] x_j[k]; B = x with its exact column maxima over ALL rows
        # (a row without out-edges has acc_j = 0 but its x_j still meets the fp16 split)
        Gp = gemm_tn_big(acc, x, b_bound=(colmax_abs(x), K, 1.0))
        G = Gp.view(H, C, K).permute(1, 0, 2).reshape(C, H * K).contiguous()
        del Gp
        return (dx,) + _xgat_weight_grads_from_G(saved, G, GV, g, want_bias_grad)
    # |agg^h_i[k]| = |sum_j beta_ij x_j[k]| <= max_j |x_j[k]| / (1 - p) over i's sources j (the
    # attention weights sum to 1, the kept ones scaled by 1 / (1 - p)): a column bound of agg from
    # the column maxima of the SOURCE rows of x (1 KB per row; a row with no out-edge -- however
    # large -- never enters an aggregate and must not loosen the bound: the fp16 split's error is
    # relative to it) instead of a pass over agg (4 KB per row); 2^-10 margin for fp32 rounding
    if xbits is None:
        xbits = saved.get("xbits")
    xbound = (colmax_abs(x, v.colptr) if xbits is None else xbits, K,
              (1.0 / (1.0 - p) if p > 0 else 1.0) * (1.0 + 2.0 ** -10))
    # (rows of g without an in-edge are outside gbits; their agg rows are zero: clamped, they add 0)
    if saved["meta"][6] and want_bias_grad:  # dbias = colsum(g) from the same pass over g
        G, gsum = gemm_tn_big(g, agg.view(v.n_dst, H * K), b_bound=xbound, a_bits=gbits, want_colsum=True)
    else:
        G, gsum = gemm_tn_big(g, agg.view(v.n_dst, H * K), b_bound=xbound, a_bits=gbits), None
    dW, datt_src, datt_dst, dbias = _xgat_weight_grads_from_G(saved, G, GV, g, want_bias_grad, gsum)
    return dx, dW, datt_src, datt_dst, dbias


def _xgat_weight_grads_from_G(saved: dict, G, GV, g, want_bias_grad: bool, gsum=None):
    W, a_s, a_d = saved["W"], saved["a_s"], saved["a_d"]
    H, C, K, slope, p, seed, has_bias = saved["meta"]
    dev = W.device
    dW = torch.empty_like(W)
    datt_src = torch.empty(H, C, dtype=torch.float32, device=dev)
    datt_dst = torch.empty(H, C, dtype=torch.float32, device=dev)
    _launch.xgat_weight_grads(G, GV, W, a_s, a_d, H, C, dW, datt_src, datt_dst)
    dbias = (gsum if gsum is not None else colsum(g)) if (has_bias and want_bias_grad) else None
    return dW, datt_src, datt_dst, dbias


class GATLayerX(torch.autograd.Function):
    """x [n_src, C_in] -> out [n_dst, C]: GATConv with H heads in the aggregate-then-transform
    form (include/ppgat.h ppgat_xgat_*): the edge pass gathers x_j once per edge for all heads,
    the per-head aggregates are transformed by one matrix-core GEMM; backward gt = g W / H
    (GEMM), one edge pass by source, dW = g^T agg (TN GEMM) + attention terms."""

    @staticmethod
    def forward(ctx, x, weight, att_src, att_dst, bias, v: "XViews", heads: int, C: int, slope: float, p: float,
                seed: int):
        out, ctx.saved = xgat_forward(x, weight, att_src, att_dst, bias, v, heads, C, slope, p, seed)
        ctx.att_shapes = (att_src.shape, att_dst.shape)
        return out

    @staticmethod
    def backward(ctx, g):
        dx, dW, datt_src, datt_dst, dbias = xgat_backward(ctx.saved, g, ctx.needs_input_grad[4])
        ctx.saved = None
        return (dx, dW, datt_src.view(ctx.att_shapes[0]), datt_dst.view(ctx.att_shapes[1]), dbias,
                None, None, None, None, None, None)


def gat_layer_x(x, weight, att_src, att_dst, bias, views: XViews, heads: int, channels: int, slope: float,
                dropout_p: float = 0.0, seed: int = 0, edge_v=None, edge_attr=None):
    if edge_v is not None or edge_attr is not None:
        raise NotImplementedError("gat_layer_x: edge features on the aggregate-then-transform layer are not "
                                  "implemented")
    _require(x.is_cuda, "gat_layer_x: ppgat runs on ROCm devices only; there is no CPU path")
    return GATLayerX.apply(x, weight, att_src, att_dst, bias, views, heads, channels, float(slope), float(dropout_p),
                           int(seed))


LOSS_KINDS = {"bpr": 0, "bce": 1}


class _BadIndex:
    """Out-of-range u/i/j are clamped on the device and counted; the count is copied to
    pinned host memory asynchronously and checked at the next loss call (or by
    ``check_bpr_indices()``), so the hot path never waits on the host."""
    pending = []

    @classmethod
    def track(cls, bad: torch.Tensor, error=None):
        """``error``: (exception type, message with one ``{}`` for the count) raised in place of
        the IndexError when the count is not zero."""
        if torch.cuda.is_current_stream_capturing():  # a captured step: no host copy / event query
            return
        host = torch.empty(1, dtype=torch.int32, pin_memory=True)
        host.copy_(bad, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        cls.pending.append((ev, host, error))

    @classmethod
    def raise_pending(cls, wait: bool = False):
        if torch.cuda.is_current_stream_capturing():
            return
        keep = []
        for ev, host, error in cls.pending:
            if wait:
                ev.synchronize()
            if wait or ev.query():
                if int(host.item()) != 0:
                    cls.pending = []
                    if error is not None:
                        raise error[0](error[1].format(int(host.item())))
                    raise IndexError(f"bpr_loss: {int(host.item())} triples with u/i/j out of range")
            else:
                keep.append((ev, host, error))
        cls.pending = keep


def check_bpr_indices():
    """Raise IndexError if any earlier bpr_loss call saw out-of-range indices (syncs)."""
    _BadIndex.raise_pending(wait=True)


class BprPrepared:
    """The triple-only half of the loss backward (ppgat_bpr_bwd_prepare), launched on a side
    stream: made before the model's forward it runs beside it.  Hand it to ``bpr_loss(...,
    prepared=)`` with the same triples and Z shape; the loss joins the side stream back into
    the current one after its own forward kernels, so nothing after the loss can see a
    half-built workspace and the workspace is not freed under the side stream."""

    def __init__(self, n_rows: int, n_users: int, n_items: int, C: int, u, i, j, row_map=None):
        lib = _lib.load()
        dev = u.device
        _require(u.is_cuda, "bpr_prepare: ppgat runs on ROCm devices only; there is no CPU path")
        if C not in (32, 64, 128, 256):
            raise NotImplementedError("bpr_loss: hidden size must be 32/64/128/256")
        self.given = tuple(t.data_ptr() for t in (u, i, j))
        self.u, self.i, self.j = (t.contiguous().to(torch.int64) for t in (u, i, j))
        for name, t in (("u", self.u), ("i", self.i), ("j", self.j)):
            _check_dev(name, t, torch.int64, dev)
        if row_map is not None:
            _check_dev("row_map", row_map, torch.int32, dev)
        self.row_map = row_map
        self.meta = (int(n_rows), int(n_users), int(n_items), int(C), self.u.numel())
        self.ws, _ = _lib.workspace(lib.ppgat_bpr_workspace_bytes, int(n_rows), self.u.numel(), int(C), device=dev)
        main = torch.cuda.current_stream(dev)
        self.side = _side_stream(dev)
        self.side.wait_stream(main)  # the triples and the workspace come from the current stream
        _lib.check(lib.ppgat_bpr_bwd_prepare(int(n_rows), int(n_users), int(n_items), _lib.ptr(row_map), int(C),
                                             self.u.data_ptr(), self.i.data_ptr(), self.j.data_ptr(), self.u.numel(),
                                             self.ws.data_ptr(), self.ws.numel(), self.side.cuda_stream),
                   "bpr_bwd_prepare")
        # the side stream uses these blocks: if the handle is dropped unconsumed (a failed take(),
        # a forward that raised), the allocator must not hand them to current-stream work before
        # the prepare kernels are done
        for t in (self.ws, self.u, self.i, self.j):
            t.record_stream(self.side)
        self.used = False

    def take(self, n_rows, n_users, n_items, C, u, i, j, row_map):
        """(u, i, j, workspace) of this handle, after checking it was made for exactly this
        call (the same triple tensors, sizes and row map), once."""
        _require(not self.used, "bpr_loss: a prepared handle serves one loss call")
        _require(self.meta == (n_rows, n_users, n_items, C, u.numel())
                 and self.given == tuple(t.data_ptr() for t in (u, i, j))
                 and _lib.ptr(row_map) == _lib.ptr(self.row_map),
                 "bpr_loss: prepared for other triples / sizes")
        self.used = True
        return self.u, self.i, self.j, self.ws


def bpr_prepare(n_rows: int, n_users: int, n_items: int, C: int, u, i, j, row_map=None) -> BprPrepared:
    """Start the triple-only half of the loss backward on a side stream (see BprPrepared)."""
    return BprPrepared(n_rows, n_users, n_items, C, u, i, j, row_map)


class _BPRLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, Z, u, i, j, n_users: int, n_items: int, kind: int, row_map, prep=None, grad_rows: int = 0,
                grad_buf=None):
        lib = _lib.load()
        ctx.grad_rows = int(grad_rows)
        ctx.grad_buf = grad_buf
        # Z straight from a heads = 1 GATLayer: the loss backward also does that layer's prologue
        ctx.producer = (_producer_of(Z, N=Z.size(0), C=Z.size(1))
                        if (row_map is None and prep is None and _producer_fusion_enabled()) else None)
        Z = Z.contiguous()
        _check_dev("Z", Z, torch.float32)
        n_rows, C = Z.shape
        S = u.numel()
        if prep is not None:
            u, i, j, ws = prep.take(n_rows, n_users, n_items, C, u, i, j, row_map)
        u, i, j = (t.contiguous().to(torch.int64) for t in (u, i, j))
        for name, t in (("u", u), ("i", i), ("j", j)):
            _check_dev(name, t, torch.int64, Z.device)
        if row_map is not None:
            _check_dev("row_map", row_map, torch.int32, Z.device)
        _BadIndex.raise_pending()
        if prep is None:
            ws, _ = _lib.workspace(lib.ppgat_bpr_workspace_bytes, n_rows, S, C, device=Z.device)
        loss = torch.empty(1, dtype=torch.float32, device=Z.device)
        coef = torch.empty(max(S, 1), 2, dtype=torch.float32, device=Z.device)
        bad = torch.empty(1, dtype=torch.int32, device=Z.device)
        # the forward only touches the workspace's block partials, which the prepare leaves alone
        _lib.check(lib.ppgat_bpr_fwd(Z.data_ptr(), n_rows, n_users, n_items, _lib.ptr(row_map), C, u.data_ptr(),
                                     i.data_ptr(), j.data_ptr(), S, kind, loss.data_ptr(), coef.data_ptr(),
                                     bad.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_handle(Z.device)),
                   "bpr_fwd")
        if prep is not None:
            torch.cuda.current_stream(Z.device).wait_stream(prep.side)
        _BadIndex.track(bad)
        ctx.save_for_backward(Z, u, i, j, coef)
        ctx.ws = ws
        ctx.prepared = prep is not None
        ctx.row_map = row_map
        ctx.meta = (n_rows, n_users, n_items, C, S)
        return loss.view(())  # (a view: its backward is a reshape, where loss[0]'s is a zero fill + copy)

    @staticmethod
    def backward(ctx, gl):
        lib = _lib.load()
        Z, u, i, j, coef = ctx.saved_tensors
        n_rows, n_users, n_items, C, S = ctx.meta
        gl = gl.reshape(1).to(torch.float32).contiguous()
        # grad_rows > n_rows: dZ is the top of a [grad_rows, C] buffer (the halo partition's top
        # layer takes the buffer as its gradient table, dist._halo_xgat_backward_deferred_d)
        # (``grad_buf``: that buffer, the caller's persistent one -- its rows past n_rows are the caller's)
        buf, ctx.grad_buf = ctx.grad_buf, None
        if buf is not None:
            _require(buf.dim() == 2 and buf.size(0) >= n_rows and buf.size(1) == C and buf.dtype == Z.dtype and
                     buf.device == Z.device and buf.is_contiguous(), "bpr: grad_buf must be a contiguous "
                     "[>= n_rows, C] buffer of Z's dtype and device")
            dZ = buf[:n_rows]
        else:
            dZ = (torch.empty(ctx.grad_rows, C, dtype=Z.dtype, device=Z.device)[:n_rows] if ctx.grad_rows > n_rows
                  else torch.empty_like(Z))
        ws = ctx.ws
        prod, ctx.producer = ctx.producer, None
        if prod is not None and prod.pro_state is not None:
            # also the producing layer's backward prologue (its nstate and dbias) from dZ
            pb, ps_dst, pm, pinv_l = prod.pro_state
            p_nstate = torch.empty(n_rows, 1, 4, dtype=torch.float32, device=Z.device)
            p_dbias = torch.empty(C, dtype=torch.float32, device=Z.device) if pb is not None else None
            _lib.check(lib.ppgat_bpr_bwd_producer(
                Z.data_ptr(), n_rows, n_users, n_items, C, u.data_ptr(), i.data_ptr(), j.data_ptr(), S,
                coef.data_ptr(), gl.data_ptr(), dZ.data_ptr(), _lib.ptr(pb), ps_dst.data_ptr(), pm.data_ptr(),
                pinv_l.data_ptr(), 1.0, p_nstate.data_ptr(), _lib.ptr(p_dbias), ws.data_ptr(), ws.numel(),
                _lib.stream_handle(Z.device)), "bpr_bwd_producer")
            prod.pro_result = (weakref.ref(dZ), dZ._version, p_nstate, p_dbias)
        else:
            fn = lib.ppgat_bpr_bwd_prepared if ctx.prepared else lib.ppgat_bpr_bwd
            _lib.check(fn(Z.data_ptr(), n_rows, n_users, n_items, _lib.ptr(ctx.row_map), C, u.data_ptr(),
                          i.data_ptr(), j.data_ptr(), S, coef.data_ptr(), gl.data_ptr(), dZ.data_ptr(), ws.data_ptr(),
                          ws.numel(), _lib.stream_handle(Z.device)), "bpr_bwd")
        ctx.ws = None
        return dZ, None, None, None, None, None, None, None, None, None, None


def bpr_loss(Z: torch.Tensor, n_users: int, u, i, j, loss: str = "bpr", prepared: BprPrepared = None) -> torch.Tensor:
    """Fused loss of train_gat_pyg.py:313-322 (``loss`` in {"bpr", "bce"}); ``prepared`` from
    ``bpr_prepare`` (made before the forward) moves the backward's sort off the critical path."""
    _require(Z.is_cuda, "bpr_loss: ppgat runs on ROCm devices only; there is no CPU path")
    if Z.size(1) not in (32, 64, 128, 256):
        raise NotImplementedError("bpr_loss: hidden size must be 32/64/128/256")
    return _BPRLoss.apply(Z, u, i, j, int(n_users), Z.size(0) - int(n_users), LOSS_KINDS[loss], None, prepared)


def _check_correction(who: str, correction, Z: torch.Tensor, n_items: int) -> torch.Tensor:
    """The logQ table of a softmax loss: fp32 [n_items] on Z's device, no gradient (raises before
    any launch otherwise)."""
    if not isinstance(correction, torch.Tensor) or correction.dtype != torch.float32 or correction.dim() != 1:
        raise ValueError(f"{who}: correction must be a 1-D float32 tensor")
    if correction.numel() != n_items:
        raise ValueError(f"{who}: correction must have one entry per item ({n_items}), got {correction.numel()}")
    if correction.device != Z.device:
        raise ValueError(f"{who}: correction must be on Z's device ({Z.device}), got {correction.device}")
    return correction.detach().contiguous()


def _track_correction(who: str, used: torch.Tensor):
    """One device check of the correction terms a call subtracts (``used`` = correction[negatives]):
    -inf (an item the sampler never draws) and NaN are refused, deferred like the index checks."""
    bad = (~(used > float("-inf"))).sum().to(torch.int32).reshape(1)  # NaN > -inf is False too
    _BadIndex.track(bad, (ValueError, who + ": {} correction terms of sampled negatives are -inf or NaN (an item of "
                                            "zero sampling weight among the negatives?)"))


class _SoftmaxLoss(torch.autograd.Function):
    """Sampled-softmax loss (ppgat_ssm_fwd / ppgat_ssm_bwd).  No producer hand-off: the layer
    that produced Z takes its ordinary backward prologue."""

    @staticmethod
    def forward(ctx, Z, u, cand, n_users: int, n_items: int, temperature: float, corr=None):
        lib = _lib.load()
        # Z straight from a GATLayer: a hand-off an earlier consumer left on that node is stale
        # for the gradient this loss returns -- dropped in backward, never made here
        ctx.producer = _producer_of(Z, N=Z.size(0), C=Z.size(1))
        Z = Z.contiguous()
        _check_dev("Z", Z, torch.float32)
        n_rows, C = Z.shape
        S, K1 = cand.shape
        u, cand = u.contiguous(), cand.contiguous()
        _check_dev("u", u, torch.int64, Z.device)
        _check_dev("cand", cand, torch.int64, Z.device)
        _BadIndex.raise_pending()
        ws, _ = _lib.workspace(lib.ppgat_ssm_workspace_bytes, n_rows, S, K1, C, device=Z.device)
        loss = torch.empty(1, dtype=torch.float32, device=Z.device)
        coef = torch.empty(max(S, 1), K1, dtype=torch.float32, device=Z.device)
        bad = torch.empty(1, dtype=torch.int32, device=Z.device)
        if corr is None:
            _lib.check(lib.ppgat_ssm_fwd(Z.data_ptr(), n_rows, n_users, n_items, C, u.data_ptr(), cand.data_ptr(), S,
                                         K1, temperature, loss.data_ptr(), coef.data_ptr(), bad.data_ptr(),
                                         ws.data_ptr(), ws.numel(), _lib.stream_handle(Z.device)), "ssm_fwd")
        else:
            if S > 0:
                _track_correction("softmax_loss", corr[cand[:, 1:].clamp(0, n_items - 1)])
            _lib.check(lib.ppgat_ssm_fwd_corrected(Z.data_ptr(), n_rows, n_users, n_items, C, u.data_ptr(),
                                                   cand.data_ptr(), corr.data_ptr(), S, K1, temperature,
                                                   loss.data_ptr(), coef.data_ptr(), bad.data_ptr(), ws.data_ptr(),
                                                   ws.numel(), _lib.stream_handle(Z.device)), "ssm_fwd_corrected")
        _BadIndex.track(bad)
        ctx.save_for_backward(Z, u, cand, coef)
        ctx.ws = ws
        ctx.meta = (n_rows, n_users, n_items, C, S, K1, temperature)
        ctx.corrected = corr is not None
        return loss.view(())

    @staticmethod
    def backward(ctx, gl):
        lib = _lib.load()
        Z, u, cand, coef = ctx.saved_tensors
        n_rows, n_users, n_items, C, S, K1, temperature = ctx.meta
        gl = gl.reshape(1).to(torch.float32).contiguous()
        dZ = torch.empty_like(Z)
        prod, ctx.producer = ctx.producer, None
        if prod is not None:
            prod.pro_result = None
        _lib.check(lib.ppgat_ssm_bwd(Z.data_ptr(), n_rows, n_users, n_items, C, u.data_ptr(), cand.data_ptr(), S, K1,
                                     temperature, coef.data_ptr(), gl.data_ptr(), dZ.data_ptr(), ctx.ws.data_ptr(),
                                     ctx.ws.numel(), _lib.stream_handle(Z.device)), "ssm_bwd")
        ctx.ws = None
        return (dZ,) + (None,) * (6 if ctx.corrected else 5)  # (one per input of this apply)


def softmax_loss(Z: torch.Tensor, n_users: int, u, cand, temperature: float = 1.0, correction=None) -> torch.Tensor:
    """Sampled-softmax loss: ``cand`` [S, M + 1] int64 item ids, column 0 the positive of user
    ``u[t]``, the rest its sampled negatives (``BPRSampler.sample_candidates``);
    ``mean_t(logsumexp_m s[t, m] - s[t, 0])`` with ``s = <Z[u], Z[n_users + cand]> / temperature``.
    Fused forward and a deterministic backward (no float atomics).
    ``correction`` (fp32 [n_items], e.g. ``BPRSampler.correction(M)``): the logQ term of negatives
    that were not drawn uniformly, ``s[t, m] -= correction[cand[t, m]]`` for m >= 1, never for the
    positive; it takes no gradient, and the terms the call uses must not be -inf or NaN."""
    if not isinstance(cand, torch.Tensor) or cand.dim() != 2 or cand.dtype != torch.int64 or cand.size(1) < 2:
        raise ValueError("softmax_loss: cand must be a 2-D int64 tensor [S, M + 1] with at least 2 columns")
    if not isinstance(u, torch.Tensor) or u.dtype != torch.int64 or u.numel() != cand.size(0):
        raise ValueError("softmax_loss: u must be an int64 tensor with one user per row of cand")
    temperature = float(temperature)
    if not (temperature > 0.0 and temperature != float("inf")):
        raise ValueError("softmax_loss: temperature must be finite and > 0")
    _require(Z.is_cuda, "softmax_loss: ppgat runs on ROCm devices only; there is no CPU path")
    if Z.dim() != 2 or Z.size(1) not in (32, 64, 128, 256):
        raise NotImplementedError("softmax_loss: hidden size must be 32/64/128/256")
    if correction is None:
        return _SoftmaxLoss.apply(Z, u.reshape(-1), cand, int(n_users), Z.size(0) - int(n_users), temperature)
    corr = _check_correction("softmax_loss", correction, Z, Z.size(0) - int(n_users))
    return _SoftmaxLoss.apply(Z, u.reshape(-1), cand, int(n_users), Z.size(0) - int(n_users), temperature, corr)


class _SharedSoftmaxLoss(torch.autograd.Function):
    """Shared-negatives softmax loss (ppgat_shs_fwd / ppgat_shs_bwd).  No producer hand-off: the
    layer that produced Z takes its ordinary backward prologue."""

    @staticmethod
    def forward(ctx, Z, u, pos, pool, hist_ptr, hist_items, n_users: int, n_items: int, temperature: float,
                corr=None):
        lib = _lib.load()
        # Z straight from a GATLayer: a hand-off an earlier consumer left on that node is stale
        # for the gradient this loss returns -- dropped in backward, never made here
        ctx.producer = _producer_of(Z, N=Z.size(0), C=Z.size(1))
        Z = Z.contiguous()
        _check_dev("Z", Z, torch.float32)
        n_rows, C = Z.shape
        S, P = u.numel(), pool.numel()
        u, pos, pool = u.contiguous(), pos.contiguous(), pool.contiguous()
        for name, t in (("u", u), ("pos", pos), ("pool", pool)):
            _check_dev(name, t, torch.int64, Z.device)
        if hist_ptr is not None:
            _check_dev("history ptr", hist_ptr, torch.int64, Z.device)
            _check_dev("history items", hist_items, torch.int32, Z.device)
        _BadIndex.raise_pending()
        ws, _ = _lib.workspace(lib.ppgat_shs_workspace_bytes if corr is None else
                               lib.ppgat_shs_corrected_workspace_bytes, n_rows, S, P, C, device=Z.device)
        loss = torch.empty(1, dtype=torch.float32, device=Z.device)
        lse = torch.empty(max(S, 1), dtype=torch.float32, device=Z.device)
        c0 = torch.empty(max(S, 1), dtype=torch.float32, device=Z.device)
        bad = torch.empty(2, dtype=torch.int32, device=Z.device)
        if corr is None:
            _lib.check(lib.ppgat_shs_fwd(Z.data_ptr(), n_rows, n_users, n_items, C, u.data_ptr(), pos.data_ptr(), S,
                                         pool.data_ptr(), P, _lib.ptr(hist_ptr), _lib.ptr(hist_items), temperature,
                                         loss.data_ptr(), lse.data_ptr(), c0.data_ptr(), bad.data_ptr(),
                                         ws.data_ptr(), ws.numel(), _lib.stream_handle(Z.device)), "shs_fwd")
        else:
            _track_correction("shared_softmax_loss", corr[pool.clamp(0, n_items - 1)])
            _lib.check(lib.ppgat_shs_fwd_corrected(Z.data_ptr(), n_rows, n_users, n_items, C, u.data_ptr(),
                                                   pos.data_ptr(), S, pool.data_ptr(), P, _lib.ptr(hist_ptr),
                                                   _lib.ptr(hist_items), corr.data_ptr(), temperature,
                                                   loss.data_ptr(), lse.data_ptr(), c0.data_ptr(), bad.data_ptr(),
                                                   ws.data_ptr(), ws.numel(), _lib.stream_handle(Z.device)),
                       "shs_fwd_corrected")
        _BadIndex.track(bad[1:], (ValueError, "shared_softmax_loss: pool must be strictly ascending "
                                              "({} entries not above their predecessor)"))
        _BadIndex.track(bad[:1], (IndexError, "shared_softmax_loss: {} of u/pos/pool out of range"))
        ctx.save_for_backward(Z, u, pos, pool, lse, c0)
        ctx.ws = ws  # the mask words (and gathered corrections) the forward left: the backward reads them
        ctx.corrected = corr is not None
        ctx.meta = (n_rows, n_users, n_items, C, S, P, temperature)
        return loss.view(())

    @staticmethod
    def backward(ctx, gl):
        lib = _lib.load()
        Z, u, pos, pool, lse, c0 = ctx.saved_tensors
        n_rows, n_users, n_items, C, S, P, temperature = ctx.meta
        gl = gl.reshape(1).to(torch.float32).contiguous()
        dZ = torch.empty_like(Z)
        prod, ctx.producer = ctx.producer, None
        if prod is not None:
            prod.pro_result = None
        entry = lib.ppgat_shs_bwd_corrected if ctx.corrected else lib.ppgat_shs_bwd
        _lib.check(entry(Z.data_ptr(), n_rows, n_users, n_items, C, u.data_ptr(), pos.data_ptr(), S, pool.data_ptr(), P,
                         temperature, lse.data_ptr(), c0.data_ptr(), gl.data_ptr(), dZ.data_ptr(), ctx.ws.data_ptr(),
                         ctx.ws.numel(), _lib.stream_handle(Z.device)), entry.__name__[6:])
        ctx.ws = None
        return (dZ,) + (None,) * (9 if ctx.corrected else 8)  # (one per input of this apply)


def shared_softmax_loss(Z: torch.Tensor, n_users: int, u, pos, pool, temperature: float = 1.0,
                        history=None) -> torch.Tensor:
    """Softmax loss with negatives shared across the batch: every positive ``pos[t]`` of user
    ``u[t]`` is scored against the same ``pool`` [P] of item ids (int64, strictly ascending, e.g.
    ``BPRSampler.sample_pool``); ``mean_t(log(exp(s0) + sum_j exp(s[t, j])) - s0)`` over the pool
    items that are neither the sample's positive nor in its user's ``history`` (a ``BPRSampler``
    or its ``(ptr, items)`` pair; None: only the positive is masked).  The scores are a
    matrix-core product that is never written; deterministic backward (no float atomics).
    A pool that was not drawn uniformly takes ``shared_softmax_loss_corrected``."""
    return shared_softmax_loss_corrected(Z, n_users, u, pos, pool, temperature, history=history, correction=None)


def shared_softmax_loss_corrected(Z: torch.Tensor, n_users: int, u, pos, pool, temperature: float = 1.0,
                                  history=None, correction=None) -> torch.Tensor:
    """``shared_softmax_loss`` with a logQ term: ``correction`` (fp32 [n_items], e.g.
    ``BPRSampler.pool_correction()``) is subtracted from the logit of every pool entry,
    ``s[t, j] -= correction[pool[j]]``, never from the positive's own logit; it takes no gradient,
    and the pool's terms must not be -inf or NaN.  ``None``: the uncorrected entries and code path."""
    for name, t in (("u", u), ("pos", pos), ("pool", pool)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or t.dim() != 1:
            raise ValueError(f"shared_softmax_loss: {name} must be a 1-D int64 tensor")
    if u.numel() != pos.numel():
        raise ValueError("shared_softmax_loss: u and pos must have one entry per sample")
    if pool.numel() < 1:
        raise ValueError("shared_softmax_loss: pool must hold at least one item")
    temperature = float(temperature)
    if not (temperature > 0.0 and temperature != float("inf")):
        raise ValueError("shared_softmax_loss: temperature must be finite and > 0")
    _require(Z.is_cuda, "shared_softmax_loss: ppgat runs on ROCm devices only; there is no CPU path")
    if Z.dim() != 2 or Z.size(1) not in (64, 128):
        raise NotImplementedError("shared_softmax_loss: hidden size must be 64/128")
    hist_ptr = hist_items = None
    if history is not None:
        hist_ptr, hist_items = (history.ptr, history.items) if hasattr(history, "ptr") else history
        if hist_ptr.numel() != int(n_users) + 1:
            raise ValueError("shared_softmax_loss: history ptr must have n_users + 1 entries")
    if correction is None:
        return _SharedSoftmaxLoss.apply(Z, u, pos, pool, hist_ptr, hist_items, int(n_users),
                                        Z.size(0) - int(n_users), temperature)
    corr = _check_correction("shared_softmax_loss", correction, Z, Z.size(0) - int(n_users))
    return _SharedSoftmaxLoss.apply(Z, u, pos, pool, hist_ptr, hist_items, int(n_users), Z.size(0) - int(n_users),
                                    temperature, corr)


def bpr_loss_mapped(Z: torch.Tensor, n_users: int, n_items: int, row_map: torch.Tensor, u, i, j,
                    loss: str = "bpr", prepared: BprPrepared = None, grad_rows: int = 0,
                    grad_buf: Optional[torch.Tensor] = None) -> torch.Tensor:
    """bpr_loss over a Z whose rows are laid out by row_map (node id -> row).  ``grad_rows``: the
    gradient of Z is the top of a buffer of that many rows (the rest is the caller's);
    ``grad_buf``: that buffer, supplied by the caller (kept across steps)."""
    if Z.size(1) not in (32, 64, 128, 256):
        raise NotImplementedError("bpr_loss: hidden size must be 32/64/128/256")
    return _BPRLoss.apply(Z, u, i, j, int(n_users), int(n_items), LOSS_KINDS[loss], row_map, prepared, grad_rows,
                          grad_buf)


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
