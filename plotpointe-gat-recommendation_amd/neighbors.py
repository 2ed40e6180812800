"""Fan-out neighbour sampling: a per-epoch sampled graph, derived on the device without a sort.

Each destination keeps at most ``fanout`` of its in-edges, drawn uniformly without replacement
(Robert Floyd's subset algorithm on the samplers' counter stream; the rule is stated in
include/ppgat.h and restated in numpy by tests/_nsample_ref.py).  The sampled graph's CSR / CSC
views and schedules are compacted out of the parent's (csrc/ppgat_nsample.hip, DESIGN.md section
21), so a resample costs scans and streaming passes and no ``csr_build``; the sampler itself
synchronises once (the kept-edge count sizes its outputs), and ``schedule_build`` reads its counts
as it does for every graph.  ROCm tensors only, as everywhere.

Seed-subgraph sampling (``sample_subgraph`` / ``SubgraphSampler``; csrc/ppgat_subgraph.hip, DESIGN.md
section 22): a row's sample depends on (seed, row, degree, cap) alone, so the L-hop sampled
in-neighbourhood of a mini-batch's seed nodes is a restriction of that sampled graph; it is
extracted, relabelled into a small graph and handed to the layers, whose work then scales with the
batch instead of the graph.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch

from . import _launch, _lib, hip_ops

MAX_FANOUT = 64  # include/ppgat.h ppgat_neighbor_max_fanout(): one lane of a wave per kept neighbour
MAX_HOPS = 8  # include/ppgat.h ppgat_subgraph_max_hops()
_M64 = (1 << 64) - 1
_EPOCH_DRAW = 1023  # the draw number of the epoch seeds: past any row's draws 0 .. MAX_FANOUT - 1


def draw64(seed: int, t: int, k: int) -> int:
    """csrc/ppgat_sample.hip draw64 in Python integers (splitmix64 finaliser over (seed, t, k))."""
    z = ((seed & _M64) + (t + 1) * 0x9E3779B97F4A7C15) & _M64
    z ^= ((k + 1) * 0xD1B54A32D192ED03) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def epoch_seed(seed: int, epoch: int) -> int:
    """The seed of epoch ``epoch``: a draw of the stream, not ``seed + epoch * constant`` (draw64
    adds (t + 1) * 0x9E37... to the seed, so an additive offset would alias epoch e + 1's row t
    with epoch e's row t + 1)."""
    return draw64(seed, epoch, _EPOCH_DRAW)


def sample_neighbors(edge_index: torch.Tensor, n_nodes: int, fanout: int, seed: int,
                     fanout_of: Optional[torch.Tensor] = None, graph: Optional[hip_ops.CSRGraph] = None,
                     workspace=None):
    """-> (edge_index_s [2, E'] int64, eid [E'] int64, graph_s: CSRGraph of edge_index_s).

    ``edge_index_s`` = the kept columns of ``edge_index`` in their order, ``eid`` their column
    numbers (``edge_attr[eid]`` is the sampled graph's attribute tensor).  ``fanout`` in
    [1, MAX_FANOUT]; ``fanout_of`` int32 [n_nodes]: an entry >= 0 replaces ``fanout`` for that
    destination (0 keeps nothing, above MAX_FANOUT raises), an entry < 0 keeps all.  ``graph``: the
    parent's CSRGraph (from ``graph_cache`` when None).  ``workspace``: the (tensor, byte count) of
    ``_launch.neighbor_workspace(n_nodes, E, device)`` to reuse across calls on one stream (some
    14 B per parent edge; allocated per call when None).  One host sync of its own, plus the two
    schedule builds'."""
    hip_ops._require(edge_index.dim() == 2 and edge_index.size(0) == 2, "edge_index must be [2, E]")
    hip_ops._check_dev("edge_index", edge_index, torch.int64)
    if not 1 <= int(fanout) <= MAX_FANOUT:
        raise NotImplementedError(f"sample_neighbors: fanout {fanout} outside [1, {MAX_FANOUT}]")
    dev, N = edge_index.device, int(n_nodes)
    if fanout_of is not None:
        hip_ops._check_dev("fanout_of", fanout_of, torch.int32, dev)
        hip_ops._require(fanout_of.shape == (N,), f"fanout_of: expected shape ({N},), got {tuple(fanout_of.shape)}")
    g = hip_ops.graph_cache.get(edge_index, N) if graph is None else graph
    hip_ops._require(g.n_nodes == N and g.n_edges == edge_index.size(1) and g.device == dev,
                     "sample_neighbors: graph is not the graph of edge_index")
    i32, i64 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        hip_ops._csr2csc(g)  # the pick flags the kept edges' CSC slots through it (csr_build leaves it)
        ws, nbytes = _launch.neighbor_workspace(N, g.n_edges, dev) if workspace is None else workspace
        rowptr_s, info = torch.empty(N + 1, **i32), torch.empty(2, **i32)
        _launch.neighbor_count(g, fanout, fanout_of, rowptr_s, info, ws, nbytes)
        Es, bad = (int(v) for v in info.tolist())  # the sampler's one host sync
        if bad:
            raise ValueError(f"sample_neighbors: fanout_of has entries above {MAX_FANOUT}")
        col, csr_eid, row, csc_eid, csc2csr, csr2csc = (torch.empty(max(Es, 1), **i32) for _ in range(6))
        colptr = torch.empty(N + 1, **i32)
        edge_index_s, eid = torch.empty(2, Es, **i64), torch.empty(Es, **i64)
        _launch.neighbor_sample(g, edge_index, seed, rowptr_s, Es, col, csr_eid, edge_index_s, eid, ws, nbytes)
        _launch.neighbor_derive(g, Es, colptr, row, csc_eid, csc2csr, csr2csc, ws, nbytes)
        max_edges = g.fwd_sched.max_edges
        fs = hip_ops.schedule_build(rowptr_s, Es, max_edges)
        bs = hip_ops.schedule_build(colptr, Es, max_edges)
    gs = hip_ops.CSRGraph(N, Es, rowptr_s, col[:Es], csr_eid[:Es], colptr, row[:Es], csc_eid[:Es], csc2csr[:Es], fs, bs,
                          csr2csc=csr2csc[:Es])
    if _lib.debug_build():
        hip_ops.debug_validate_graph(gs)
    return edge_index_s, eid, gs


@dataclass
class Subgraph:
    """The L-hop sampled in-neighbourhood of a seed set, relabelled (``sample_subgraph``; the rule is
    stated in include/ppgat.h "seed-subgraph sampling")."""
    n_id: torch.Tensor  # [N_s] int64: the kept nodes' global ids, ascending (users precede items)
    depth: torch.Tensor  # [N_s] int32: 0 at the seeds
    n_users_s: int  # how many n_id entries are < n_users
    edge_index_s: torch.Tensor  # [2, E_s] int64, local ids, in ascending original edge id
    eid: torch.Tensor  # [E_s] int64: the original columns (edge_attr[eid] carries attributes over)
    seed_local: torch.Tensor  # [len(seeds)] int64: the seeds' local ids, in the seeds' order
    graph_s: hip_ops.CSRGraph  # the graph of edge_index_s over N_s nodes (csr_build's, bit for bit)

    @property
    def n_nodes(self) -> int:
        return int(self.n_id.numel())

    @property
    def n_edges(self) -> int:
        return int(self.eid.numel())

    def localize(self, ids: torch.Tensor) -> torch.Tensor:
        """Global node ids -> local ids (a binary search of ``n_id``); an id outside the subgraph
        raises ``ValueError`` (one host sync: the check)."""
        hip_ops._check_dev("ids", ids, torch.int64, self.n_id.device)
        n = self.n_nodes
        if n == 0:
            if ids.numel():
                raise ValueError("Subgraph.localize: the subgraph is empty")
            return ids.clone()
        pos = torch.searchsorted(self.n_id, ids)
        found = self.n_id[pos.clamp(max=n - 1)] == ids
        if not bool(found.all()):
            raise ValueError(f"Subgraph.localize: {int((~found).sum())} ids are not nodes of the subgraph")
        return pos


def subgraph_workspace(n_nodes: int, n_edges: int, device):
    """((tensor, bytes) of the subgraph passes, (tensor, bytes) of the neighbour sampler's): what
    ``sample_subgraph(..., workspace=)`` reuses across calls on one stream."""
    return (_launch.subgraph_workspace(n_nodes, device), _launch.neighbor_workspace(n_nodes, n_edges, device))


def sample_subgraph(edge_index: torch.Tensor, n_nodes: int, seeds: torch.Tensor, hops: int, fanout: int, seed: int,
                    fanout_of: Optional[torch.Tensor] = None, n_users: Optional[int] = None,
                    graph: Optional[hip_ops.CSRGraph] = None, workspace=None) -> Subgraph:
    """The ``hops``-hop in-neighbourhood of ``seeds`` (int64, any order, duplicates allowed) inside
    the graph ``sample_neighbors(edge_index, n_nodes, fanout, seed, fanout_of)`` keeps, relabelled
    into a small graph: the edges of the sampled graph whose destination lies within ``hops - 1``
    sampled hops of a seed, over the nodes within ``hops``.  ``hops`` in [0, MAX_HOPS] (0: the unique
    seeds, no edges); a seed outside [0, n_nodes) raises ``ValueError``.  ``n_users`` (default
    ``n_nodes``) splits ``n_id`` into users and items.  ``graph`` / ``workspace``: the parent's
    CSRGraph and ``subgraph_workspace(...)``, as in ``sample_neighbors``.  One host sync of its own
    (the two sizes and the flags, read together), plus the two schedule builds'."""
    hip_ops._require(edge_index.dim() == 2 and edge_index.size(0) == 2, "edge_index must be [2, E]")
    hip_ops._check_dev("edge_index", edge_index, torch.int64)
    dev, N = edge_index.device, int(n_nodes)
    hip_ops._check_dev("seeds", seeds, torch.int64, dev)
    hip_ops._require(seeds.dim() == 1, "seeds must be 1-D")
    if not 0 <= int(hops) <= MAX_HOPS:
        raise ValueError(f"sample_subgraph: hops {hops} outside [0, {MAX_HOPS}]")
    if not 1 <= int(fanout) <= MAX_FANOUT:
        raise NotImplementedError(f"sample_subgraph: fanout {fanout} outside [1, {MAX_FANOUT}]")
    nu = N if n_users is None else int(n_users)
    hip_ops._require(0 <= nu <= N, f"sample_subgraph: n_users {nu} outside [0, {N}]")
    if fanout_of is not None:
        hip_ops._check_dev("fanout_of", fanout_of, torch.int32, dev)
        hip_ops._require(fanout_of.shape == (N,), f"fanout_of: expected shape ({N},), got {tuple(fanout_of.shape)}")
    g = hip_ops.graph_cache.get(edge_index, N) if graph is None else graph
    hip_ops._require(g.n_nodes == N and g.n_edges == edge_index.size(1) and g.device == dev,
                     "sample_subgraph: graph is not the graph of edge_index")
    i32, i64 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.int64, device=dev)
    hops, T = int(hops), int(seeds.numel())
    with torch.cuda.device(dev):
        hip_ops._csr2csc(g)
        (sws, sbytes), (nws, nbytes) = subgraph_workspace(N, g.n_edges, dev) if workspace is None else workspace
        info = torch.empty(6, **i32)  # (E_s, the count's bad) then (N_s, n_users_s, bad seed, bad fanout_of)
        cap, rowptr_p, colptr_p = torch.empty(max(N, 1), **i32), torch.empty(N + 1, **i32), torch.empty(N + 1, **i32)
        _launch.subgraph_seed(seeds, N, info[2:], sws, sbytes)
        for hop in range(hops):
            _launch.subgraph_expand(g, hop, fanout, fanout_of, seed, sws, sbytes)
        _launch.subgraph_plan(N, nu, hops, fanout, fanout_of, cap, info[2:], sws, sbytes)
        _launch.neighbor_count(g, fanout, cap, rowptr_p, info, nws, nbytes)
        Es, bad, Ns, nus, bad_seed, bad_cap = (int(v) for v in info.tolist())  # the one host sync
        if bad_seed:
            raise ValueError(f"sample_subgraph: seeds has entries outside [0, {N})")
        if bad or bad_cap:
            raise ValueError(f"sample_subgraph: fanout_of has entries above {MAX_FANOUT}")
        col, csr_eid, row, csc_eid, csc2csr, csr2csc = (torch.empty(max(Es, 1), **i32) for _ in range(6))
        edge_index_s, eid = torch.empty(2, Es, **i64), torch.empty(Es, **i64)
        _launch.neighbor_sample(g, edge_index, seed, rowptr_p, Es, col, csr_eid, edge_index_s, eid, nws, nbytes)
        _launch.neighbor_derive(g, Es, colptr_p, row, csc_eid, csc2csr, csr2csc, nws, nbytes)
        n_id, depth, seed_local = torch.empty(Ns, **i64), torch.empty(Ns, **i32), torch.empty(T, **i64)
        rowptr_s, colptr_s = torch.empty(Ns + 1, **i32), torch.empty(Ns + 1, **i32)
        _launch.subgraph_relabel(N, Ns, Es, seeds, rowptr_p, colptr_p, n_id, depth, rowptr_s, colptr_s, col, row,
                                 edge_index_s, seed_local, sws, sbytes)
        max_edges = g.fwd_sched.max_edges
        fs = hip_ops.schedule_build(rowptr_s, Es, max_edges)
        bs = hip_ops.schedule_build(colptr_s, Es, max_edges)
    gs = hip_ops.CSRGraph(Ns, Es, rowptr_s, col[:Es], csr_eid[:Es], colptr_s, row[:Es], csc_eid[:Es], csc2csr[:Es],
                          fs, bs, csr2csc=csr2csc[:Es])
    if _lib.debug_build():
        hip_ops.debug_validate_graph(gs)
    return Subgraph(n_id, depth, nus, edge_index_s, eid, seed_local, gs)


class SubgraphSampler:
    """Mini-batch subgraphs of one parent graph: ``batch(epoch, b, seeds)`` -> ``Subgraph`` under
    ``epoch_seed(epoch_seed(seed, epoch), b)``.  ``graph_s`` is registered in
    ``hip_ops.graph_cache`` under ``edge_index_s`` (the layers find it and never call
    ``csr_build``) and the previous batch's entry is dropped; one workspace serves every batch."""

    def __init__(self, edge_index: torch.Tensor, n_nodes: int, hops: int, fanout: int, seed: int = 42,
                 fanout_of: Optional[torch.Tensor] = None, n_users: Optional[int] = None):
        hip_ops._check_dev("edge_index", edge_index, torch.int64)
        self.edge_index, self.n_nodes, self.hops, self.fanout, self.seed = (edge_index, int(n_nodes), int(hops),
                                                                            int(fanout), int(seed))
        self.fanout_of, self.n_users = fanout_of, n_users
        self.graph = hip_ops.graph_cache.get(edge_index, self.n_nodes)  # held: the parent may leave the cache
        self._last = None
        with torch.cuda.device(edge_index.device):
            self._workspace = subgraph_workspace(self.n_nodes, self.graph.n_edges, edge_index.device)

    def batch(self, epoch: int, b: int, seeds: torch.Tensor) -> Subgraph:
        sub = sample_subgraph(self.edge_index, self.n_nodes, seeds, self.hops, self.fanout,
                              epoch_seed(epoch_seed(self.seed, int(epoch)), int(b)), fanout_of=self.fanout_of,
                              n_users=self.n_users, graph=self.graph, workspace=self._workspace)
        if self._last is not None:
            hip_ops.graph_cache.drop(self._last)
        hip_ops.graph_cache.put(sub.edge_index_s, sub.n_nodes, sub.graph_s)
        self._last = sub.edge_index_s
        return sub


class NeighborSampler:
    """A graph resampled per epoch: ``epoch(e)`` -> (edge_index_s, eid, graph_s) under
    ``epoch_seed(seed, e)``.  The derived graph is registered in ``hip_ops.graph_cache`` under
    ``edge_index_s``, so ``model(item_feats, edge_index_s)`` finds it and never calls
    ``csr_build``; the previous epoch's entry is dropped (at 200M edges a graph is several GB).  The
    sampler's workspace is allocated once and reused by every epoch."""

    def __init__(self, edge_index: torch.Tensor, n_nodes: int, fanout: int, seed: int = 42,
                 fanout_of: Optional[torch.Tensor] = None):
        self.edge_index, self.n_nodes, self.fanout, self.seed, self.fanout_of = (edge_index, int(n_nodes), int(fanout),
                                                                                 int(seed), fanout_of)
        self.graph = hip_ops.graph_cache.get(edge_index, self.n_nodes)  # held: the parent may leave the cache
        self._last = None
        with torch.cuda.device(edge_index.device):
            self._workspace = _launch.neighbor_workspace(self.n_nodes, self.graph.n_edges, edge_index.device)

    def epoch(self, e: int):
        out = sample_neighbors(self.edge_index, self.n_nodes, self.fanout, epoch_seed(self.seed, int(e)),
                               fanout_of=self.fanout_of, graph=self.graph, workspace=self._workspace)
        if self._last is not None:
            hip_ops.graph_cache.drop(self._last)
        hip_ops.graph_cache.put(out[0], self.n_nodes, out[2])
        self._last = out[0]
        return out
