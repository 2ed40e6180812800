"""LightGCN baseline -- scripts/train_lightgcn.py, on the device.

``build_adj``   -- :130-157, the normalised adjacency in the reference's entry order
                   (two directed entries per train interaction, un-coalesced), vectorised.
``LGCNGraph``   -- the CSR / CSC views of (adj_indices, adj_values) with per-slot values and
                   the work schedules (hub splitting) of ``hip_ops.csr_build``.
``propagate``   -- :64-76 as an autograd function: K launches of ``ppgat_lgcn_hop`` with the
                   running layer mean fused in; the backward is the same recurrence over the
                   CSC view (A^T; A is not assumed symmetric).
``LightGCN``    -- :51-79, same constructor, construction order and state_dict keys
                   (E_user.weight, E_item.weight, adj_indices, adj_values), so seeded weights
                   match and checkpoints load both ways.

No CPU path: tensors live on a ROCm device and the library must be loaded.
"""
from __future__ import annotations

from typing import Dict, Tuple

import numpy as np
import torch

from . import _launch, hip_ops


def build_adj(n_users: int, n_items: int, train_pos_idx: Dict[int, np.ndarray]) -> Tuple[torch.Tensor, torch.Tensor]:
    """train_lightgcn.py:130-157 -> (indices int64 [2, nnz], values float32 [nnz]), bit for bit:
    entries (u, n_users + i), (n_users + i, u) per interaction in dict / list order; deg counts
    interactions per node (repeats count) clipped to >= 1; value float32(1 / sqrt(deg_r * deg_c))
    formed in float64."""
    keys = list(train_pos_idx.keys())
    lens = np.fromiter((len(train_pos_idx[k]) for k in keys), dtype=np.int64, count=len(keys))
    us = np.repeat(np.asarray(keys, dtype=np.int64), lens)
    its = (np.concatenate([np.asarray(train_pos_idx[k], dtype=np.int64) for k in keys]) if len(keys)
           else np.zeros(0, np.int64)) + n_users
    rows = np.empty(2 * len(us), dtype=np.int64)
    cols = np.empty(2 * len(us), dtype=np.int64)
    rows[0::2], cols[0::2] = us, its
    rows[1::2], cols[1::2] = its, us
    n = n_users + n_items
    # the reference accumulates the counts in float32 (exact below 2^24) and clips at 1
    deg = np.clip((np.bincount(us, minlength=n) + np.bincount(its, minlength=n)).astype(np.float32), 1.0, None)
    d64 = deg.astype(np.float64)
    vals = (1.0 / np.sqrt(d64[rows] * d64[cols])).astype(np.float32)
    return torch.from_numpy(np.vstack([rows, cols])), torch.from_numpy(vals)


class LGCNGraph:
    """out = A x over A = sparse_coo(adj_indices [2, nnz] (row, col), adj_values): CSR by row for
    the forward (``val_csr`` per CSR slot, slots in the entries' original order, so a repeated
    entry contributes twice as in the un-coalesced COO product) and CSC by column for the
    backward (``val_t = val_csr[csc2csr]``)."""

    def __init__(self, adj_indices: torch.Tensor, adj_values: torch.Tensor, n_nodes: int):
        hip_ops._require(adj_indices.is_cuda and adj_values.is_cuda,
                         "LGCNGraph: ppgat runs on ROCm devices only; there is no CPU path")
        hip_ops._require(adj_indices.dim() == 2 and adj_indices.size(0) == 2 and
                         adj_values.numel() == adj_indices.size(1), "LGCNGraph: indices [2, nnz], values [nnz]")
        # message-passing orientation: source = column, destination = row
        ei = torch.stack([adj_indices[1], adj_indices[0]]).to(torch.int64).contiguous()
        self.g = hip_ops.csr_build(ei, int(n_nodes))
        vals = adj_values.to(torch.float32).contiguous()
        self.n_nodes = int(n_nodes)
        self.n_edges = self.g.n_edges
        self.val_csr = vals[self.g.csr_eid.long()].contiguous()
        self.val_t = self.val_csr[self.g.csc2csr.long()].contiguous()
        self._ws = {}

    @property
    def device(self):
        return self.g.device

    def workspace(self, sched, channels: int) -> torch.Tensor:
        """The hub pieces' partial rows (one buffer per schedule and width, reused by every hop:
        hops are ordered on the stream)."""
        key = (id(sched), channels)
        ws = self._ws.get(key)
        if ws is None:
            ws = self._ws[key] = _launch.lgcn_hop_workspace(sched.n_hub_items, channels, self.device)
        return ws


class _GraphCache:
    """LGCNGraph per (adj_indices, adj_values) buffer pair, keyed on identity and version."""

    def __init__(self, capacity: int = 4):
        self.capacity = capacity
        self.entries = []

    def get(self, adj_indices: torch.Tensor, adj_values: torch.Tensor, n_nodes: int) -> LGCNGraph:
        key = (adj_indices.data_ptr(), adj_indices._version, adj_values.data_ptr(), adj_values._version,
               tuple(adj_indices.shape), int(n_nodes), str(adj_indices.device))
        for k, ri, rv, g in self.entries:
            if k == key and ri is adj_indices and rv is adj_values:
                return g
        g = LGCNGraph(adj_indices, adj_values, n_nodes)
        self.entries.append((key, adj_indices, adj_values, g))
        if len(self.entries) > self.capacity:
            self.entries.pop(0)
        return g

    def clear(self):
        self.entries.clear()


graph_cache = _GraphCache()


def supported(channels: int) -> bool:
    return _launch.lgcn_supported(channels)


def hop(graph: LGCNGraph, src, acc_in=None, div: float = 1.0, want_out: bool = True, accw=None,
        transpose: bool = False, out=None):
    """One ``ppgat_lgcn_hop``: s = A src (A^T with ``transpose``); returns (out, accw) with
    out = s when ``want_out`` and accw = (acc_in + s) / div when ``accw`` (a tensor to write, which
    may be acc_in itself) or ``acc_in`` is given.  ``src`` / ``acc_in``: one [N, C] tensor or a
    pair of row segments (top, bottom)."""
    g = graph.g
    N, E = graph.n_nodes, graph.n_edges
    dev = graph.device

    def segs(name, t):
        if t is None:
            return None, None, 0, None
        a, b = t if isinstance(t, (tuple, list)) else (t, None)
        for nm, x in ((name, a), (name, b)):
            if x is not None:
                hip_ops._check_dev(nm, x, torch.float32, dev)
                hip_ops._require(x.dim() == 2, f"{nm}: [rows, C]")
        rows = a.size(0) + (b.size(0) if b is not None else 0)
        hip_ops._require(rows == N, f"{name}: {rows} rows but the graph has {N} nodes")
        hip_ops._require(b is None or b.size(1) == a.size(1), f"{name}: segments of different widths")
        return a, b, a.size(0), a.size(1)

    s0, s1, ssplit, C = segs("src", src)
    a0, a1, asplit, Ca = segs("acc_in", acc_in)
    hip_ops._require(Ca is None or Ca == C, "acc_in: width differs from src")
    if accw is None and acc_in is not None:
        accw = torch.empty(N, C, dtype=torch.float32, device=dev)
    if want_out and out is None:
        out = torch.empty(N, C, dtype=torch.float32, device=dev)
    if not want_out:
        out = None
    sched = g.bwd_sched if transpose else g.fwd_sched
    idx = g.row if transpose else g.col
    val = graph.val_t if transpose else graph.val_csr
    ws = graph.workspace(sched, C) if sched.n_hub_items > 0 and supported(C) else None
    _launch.lgcn_hop(sched, idx, val, N, E, C, s0, s1, ssplit, a0, a1, asplit, div, out, accw, ws)
    return out, accw


def _recurrence(graph: LGCNGraph, x0, K: int, transpose: bool) -> torch.Tensor:
    """((x0 + A x0) + A^2 x0 + ...) / (K + 1) in K launches (K >= 1): hop 1 writes out_1 and the
    running sum, middle hops update the sum in place, hop K writes only the result."""
    if K == 1:
        return hop(graph, x0, acc_in=x0, div=2.0, want_out=False, transpose=transpose)[1]
    out, acc = hop(graph, x0, acc_in=x0, transpose=transpose)
    spare = None
    for k in range(2, K):
        nxt, _ = hop(graph, out, acc_in=acc, accw=acc, transpose=transpose, out=spare)
        out, spare = nxt, out
    # out_K is not stored; the mean overwrites the running sum
    return hop(graph, out, acc_in=acc, accw=acc, div=float(K + 1), want_out=False, transpose=transpose)[1]


class _Propagate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x_user, x_item, graph: LGCNGraph, K: int):
        ctx.graph, ctx.K, ctx.n_users = graph, K, x_user.size(0)
        return _recurrence(graph, (x_user, x_item), K, transpose=False)

    @staticmethod
    def backward(ctx, gz):
        gz = gz.contiguous()
        d = _recurrence(ctx.graph, gz, ctx.K, transpose=True)
        return d[:ctx.n_users], d[ctx.n_users:], None, None


def propagate(x_user: torch.Tensor, x_item: torch.Tensor, graph: LGCNGraph, K: int) -> torch.Tensor:
    """Z [n_users + n_items, d] = mean over k = 0..K of A^k cat(x_user, x_item)
    (train_lightgcn.py:64-73).  K = 0 returns the concatenation and launches nothing."""
    for name, t in (("x_user", x_user), ("x_item", x_item)):
        hip_ops._check_dev(name, t, torch.float32, graph.device)
    hip_ops._require(x_user.dim() == 2 and x_item.dim() == 2 and x_user.size(1) == x_item.size(1),
                     "propagate: x_user [n_users, d], x_item [n_items, d]")
    hip_ops._require(x_user.size(0) + x_item.size(0) == graph.n_nodes, "propagate: rows differ from the graph's nodes")
    K = int(K)
    hip_ops._require(K >= 0, "propagate: K >= 0")
    if K == 0:
        return torch.cat([x_user, x_item], dim=0)
    if not supported(x_user.size(1)):
        raise NotImplementedError(f"propagate: embedding width {x_user.size(1)} (64, 128 or 256)")
    return _Propagate.apply(x_user, x_item, graph, K)


class LightGCN(torch.nn.Module):
    """train_lightgcn.py:51-79."""

    def __init__(self, n_users: int, n_items: int, embed_dim: int, adj_indices: torch.Tensor,
                 adj_values: torch.Tensor, n_layers: int = 3):
        super().__init__()
        self.n_users = n_users
        self.n_items = n_items
        self.E_user = torch.nn.Embedding(n_users, embed_dim)
        self.E_item = torch.nn.Embedding(n_items, embed_dim)
        torch.nn.init.normal_(self.E_user.weight, std=0.1)
        torch.nn.init.normal_(self.E_item.weight, std=0.1)
        self.register_buffer("adj_indices", adj_indices)  # 2 x nnz
        self.register_buffer("adj_values", adj_values)    # nnz
        self.embed_dim = embed_dim
        self.n_layers = n_layers

    def graph(self) -> LGCNGraph:
        if not self.E_user.weight.is_cuda:
            raise RuntimeError("LightGCN: ppgat runs on ROCm devices only; there is no CPU path")
        return graph_cache.get(self.adj_indices, self.adj_values, self.n_users + self.n_items)

    def propagate_all(self, K: int) -> torch.Tensor:
        return propagate(self.E_user.weight, self.E_item.weight, self.graph(), K)

    def propagate(self, K: int) -> Tuple[torch.Tensor, torch.Tensor]:
        acc = self.propagate_all(K)
        return acc[: self.n_users], acc[self.n_users:]

    def score(self, U: torch.Tensor, I: torch.Tensor) -> torch.Tensor:
        return (U * I).sum(dim=-1)

    def forward(self, item_feats=None, edge_index=None) -> torch.Tensor:
        """Z [N, d] with ``self.n_layers`` hops (the signature evaluation.eval_sampled,
        export_item_embeddings and the serving path call models with; both arguments unused)."""
        return self.propagate_all(self.n_layers)


def train_step(model: LightGCN, opt, u, i, j, K: int = None):
    """One mini-batch of train_lightgcn.py:317-334: propagate, -log(sigmoid(pos - neg) + 1e-8).mean()
    (the fused ``bpr`` loss), zero_grad, backward, step.  Returns the loss (device scalar)."""
    Z = model.propagate_all(model.n_layers if K is None else K)
    loss = hip_ops.bpr_loss(Z, model.n_users, u, i, j, "bpr")
    opt.zero_grad()
    loss.backward()
    opt.step()
    return loss
