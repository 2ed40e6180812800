"""Graph preprocessing behind hip_ops: the checks every wrapper shares, CSR / CSC views and their work
schedules (csr_build, schedule_build, graph_cache), edge-attribute staging, and the two pieces both
layer forms share -- the dropout seed slot and the LeakyReLU kink tap of the tests.

Module state lives here and only here: ``KINK_TAP`` and ``EDGE_STAGE_COUNT`` are rebound, so they
are read and set on this module, never through hip_ops.  No CPU fallback anywhere.
"""
from __future__ import annotations

import weakref
from dataclasses import dataclass
from typing import Optional

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
    _check_dev("ptr", ptr, torch.int32)
    N = ptr.numel() - 1
    dev = ptr.device
    cap = _launch.schedule_capacity(N, n_edges, max_edges)
    _require(cap >= 0, "schedule_capacity: bad arguments")
    i32 = dict(dtype=torch.int32, device=dev)
    item_row = torch.empty(max(cap, 1), **i32)
    item_beg = torch.empty(max(cap, 1), **i32)
    item_end = torch.empty(max(cap, 1), **i32)
    hub_row = torch.empty(max(N, 1), **i32)
    hub_ptr = torch.empty(N + 1, **i32)
    counts = torch.empty(4, **i32)
    _launch.schedule_build(ptr, N, n_edges, max_edges, item_row, item_beg, item_end, hub_row, hub_ptr, counts)
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
    _launch.csr_build(ei, E, N, rowptr, col, csr_eid, colptr, row, csc_eid, csc2csr, bad)
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
        _launch.invert_index(g.csc2csr, E, inv)
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
