"""Consumers of the inference forward.

* ``eval_sampled``        -- scripts/train_gat_pyg.py:150-176 (identical custom :184-210):
  no-grad forward, 1 held-out positive + ``eval_neg_k`` rejection-sampled negatives per
  user, rank = #(score > positive's score) + 1, Recall@K / NDCG@K means.  The negatives
  are drawn with the reference's exact ``np.random`` call sequence (so a seeded run
  evaluates the same candidates); the scoring of all users is ONE device pass
  (``ppgat_sampled_rank``) instead of a GEMV + device->host sync per user.
  ``sampler=`` (a sampler.BPRSampler over the train lists) draws the candidates on the
  device too (``ppgat_eval_sample``: same rule, counter-based stream), so the whole
  evaluation is two kernels and one copy of the ranks; ``fast=True`` draws the same
  distribution with vectorised numpy (different stream).
* ``eval_full`` / ``full_rank`` -- the full-ranking protocol of the LightGCN literature: the
  held-out positive against EVERY item outside the user's train history (no sampling, so the
  metrics are exact and comparable with published ones).  One fused matrix-core pass
  (``ppgat_full_rank``): the ``[users, items]`` score matrix is never written.
* ``recommend_topk`` / ``topk_metrics`` / ``eval_topk`` -- the recommender's output: for every
  user the K best items outside the train history, from the same fused product with a selection
  epilogue (``ppgat_full_topk``), and the metrics that need the lists (several held-out items
  per user, precision, catalogue coverage).
* ``export_item_embeddings`` -- tools/export_item_embeddings.py:139-145.
* ``top_k_for_user_items`` / ``top_k_batch`` -- serving/runtime.py:56-76 on the device
  (``ppgat_serve_topk``): user vector = mean of history rows, history masked to -1e9,
  the k best descending with ties by smaller item index.
"""
from __future__ import annotations

import math
from typing import Dict, Sequence

import numpy as np
import torch

from . import _launch


def sample_eval_candidates(train_pos_idx: Dict[int, np.ndarray], eval_pos: Dict[int, int], n_items: int,
                           eval_neg_k: int):
    """The reference's candidate draw (train_gat_pyg.py:157-167), same np.random sequence."""
    user_pos_sets = {u: set(pos) for u, pos in train_pos_idx.items()}
    users = np.empty(len(eval_pos), np.int64)
    cands = np.empty((len(eval_pos), eval_neg_k + 1), np.int64)
    for t, (u, pos_i) in enumerate(eval_pos.items()):
        avoid = user_pos_sets.get(u, set()) | {pos_i}
        negs = []
        while len(negs) < eval_neg_k:
            cand = np.random.randint(0, n_items)
            if cand not in avoid:
                negs.append(cand)
        users[t] = u
        cands[t, 0] = pos_i
        cands[t, 1:] = negs
    return users, cands


def sample_eval_candidates_fast(train_pos_idx: Dict[int, np.ndarray], eval_pos: Dict[int, int], n_items: int,
                                eval_neg_k: int, seed: int = 0):
    """Same distribution (uniform over items not in train history + positive), vectorised."""
    rng = np.random.default_rng(seed)
    users = np.fromiter(eval_pos.keys(), np.int64, len(eval_pos))
    pos = np.fromiter(eval_pos.values(), np.int64, len(eval_pos))
    negs = rng.integers(0, n_items, (len(users), eval_neg_k))
    for _ in range(64):
        bad = negs == pos[:, None]
        for t, u in enumerate(users):
            hist = train_pos_idx.get(int(u))
            if hist is not None and len(hist):
                bad[t] |= np.isin(negs[t], hist)
        if not bad.any():
            break
        negs[bad] = rng.integers(0, n_items, int(bad.sum()))
    return users, np.concatenate([pos[:, None], negs], 1)


def sampled_rank(Z: torch.Tensor, n_users: int, users: np.ndarray, cands: np.ndarray, row_map=None) -> np.ndarray:
    """rank[b] = #(scores > positive score) + 1 for candidate lists (column 0 = positive)."""
    if not Z.is_cuda or Z.dtype != torch.float32:
        raise RuntimeError("sampled_rank: fp32 ROCm tensor required (no CPU path)")
    Z = Z.contiguous()
    dev = Z.device
    n_rows, C = Z.shape
    n_items = (n_rows - n_users) if row_map is None else int(row_map.numel()) - n_users
    u = torch.as_tensor(users, dtype=torch.int64).to(dev).contiguous()
    c = torch.as_tensor(cands, dtype=torch.int64).to(dev).contiguous()
    rank = torch.empty(len(u), dtype=torch.int32, device=dev)
    _launch.sampled_rank(Z, n_users, n_items, row_map, u, c, rank)
    return rank.cpu().numpy()


def metrics_from_ranks(ranks: np.ndarray, Ks: Sequence[int] = (10, 20)) -> Dict[str, float]:
    """train_gat_pyg.py:158-176 aggregation (key order recall@K..., ndcg@K...)."""
    metrics = {f"recall@{k}": [] for k in Ks}
    metrics.update({f"ndcg@{k}": [] for k in Ks})
    for r in ranks.tolist():
        for k in Ks:
            hit = 1.0 if r <= k else 0.0
            metrics[f"recall@{k}"].append(hit)
            metrics[f"ndcg@{k}"].append((1.0 / math.log2(r + 1)) if hit else 0.0)
    return {m: float(np.mean(v)) if v else 0.0 for m, v in metrics.items()}


def _edge_kw(edge_attr) -> dict:
    """The model forward's edge argument (only models built with edge_dim take one)."""
    return {} if edge_attr is None else {"edge_attr": edge_attr}


def eval_sampled(model, cfg, item_feats: torch.Tensor, edge_index: torch.Tensor,
                 train_pos_idx: Dict[int, np.ndarray], eval_pos: Dict[int, int], Ks=(10, 20), fast: bool = False,
                 sampler=None, seed: int = 0, edge_attr=None):
    """Mirror of eval_sampled (train_gat_pyg.py:150-176); ``cfg.eval_neg_k`` negatives.
    ``edge_attr``: the edge features of a model built with edge_dim (here and in the functions below)."""
    with torch.no_grad():
        Z = model(item_feats, edge_index, **_edge_kw(edge_attr))
    if sampler is not None:
        if not eval_pos:
            return metrics_from_ranks(np.zeros(0, np.int64), Ks)
        users = np.fromiter(eval_pos.keys(), np.int64, len(eval_pos))
        pos = np.fromiter(eval_pos.values(), np.int64, len(eval_pos))
        cands = sampler.eval_candidates(users, pos, cfg.eval_neg_k, seed)
        return metrics_from_ranks(sampled_rank(Z, model.n_users, users, cands), Ks)
    if fast:
        users, cands = sample_eval_candidates_fast(train_pos_idx, eval_pos, model.n_items, cfg.eval_neg_k)
    else:
        users, cands = sample_eval_candidates(train_pos_idx, eval_pos, model.n_items, cfg.eval_neg_k)
    if len(users) == 0:
        return metrics_from_ranks(np.zeros(0, np.int64), Ks)
    ranks = sampled_rank(Z, model.n_users, users, cands)
    return metrics_from_ranks(ranks, Ks)


def full_rank(Z_users: torch.Tensor, Z_items: torch.Tensor, users, pos, sampler=None, return_ties: bool = False):
    """rank[b] = 1 + #{items i outside history(users[b]) + {pos[b]} : s(i) > s(pos[b])} over the
    whole catalogue, s(i) = <Z_users[users[b]], Z_items[i]> (strict, as the sampled rule).

    ``Z_users`` [n_users, C] / ``Z_items`` [n_items, C]: fp32 ROCm tensors with dense rows; row or
    column views of one table are used in place (the leading dimension is ``stride(0)``).
    ``sampler``: a sampler.BPRSampler over the train lists (its sorted history CSR is the
    excluded set); None = nothing but the positive is excluded.  ``return_ties`` adds the count
    of non-excluded items whose score EQUALS the positive's (a collapsed model shows there: the
    strict rule ranks every user first when all scores are equal)."""
    for t in (Z_users, Z_items):
        if not t.is_cuda or t.dtype != torch.float32 or t.dim() != 2:
            raise RuntimeError("full_rank: 2-D fp32 ROCm tensors required (no CPU path)")
    if Z_users.size(1) != Z_items.size(1) or Z_users.device != Z_items.device:
        raise ValueError("full_rank: Z_users and Z_items differ in width or device")
    dev = Z_users.device
    u = torch.as_tensor(users, dtype=torch.int64).to(dev).contiguous()
    p = torch.as_tensor(pos, dtype=torch.int64).to(dev).contiguous()
    if u.shape != p.shape or u.dim() != 1:
        raise ValueError("full_rank: users and pos must be 1-D and of equal length")
    if sampler is not None and (sampler.n_users != Z_users.size(0) or sampler.n_items != Z_items.size(0)):
        raise ValueError("full_rank: the sampler's history is over other users / items than the tables")
    n = u.numel()
    rank = torch.empty(n, dtype=torch.int32, device=dev)
    ties = torch.empty(n, dtype=torch.int32, device=dev) if return_ties else None
    _launch.full_rank(Z_users, Z_items, u, p, None if sampler is None else sampler.ptr,
                      None if sampler is None else sampler.items, rank, ties)
    if return_ties:
        return rank.cpu().numpy(), ties.cpu().numpy()
    return rank.cpu().numpy()


def eval_full(model, cfg, item_feats: torch.Tensor, edge_index: torch.Tensor,
              train_pos_idx: Dict[int, np.ndarray], eval_pos: Dict[int, int], Ks=(10, 20), sampler=None,
              edge_attr=None):
    """eval_sampled's call shape and returned dict, under the full-ranking protocol: each held-out
    positive is ranked against every item outside the user's train history (``full_rank``).
    ``sampler``: a sampler.BPRSampler over the train lists; None builds one from
    ``train_pos_idx``.  ``cfg`` is unused (no negatives are drawn)."""
    with torch.no_grad():
        Z = model(item_feats, edge_index, **_edge_kw(edge_attr))
    if not eval_pos:
        return metrics_from_ranks(np.zeros(0, np.int64), Ks)
    n_users, n_items = model.n_users, model.n_items
    if sampler is None:
        from . import sampler as sampler_mod
        from .train import user_csr
        ptr, flat = user_csr(train_pos_idx, n_users)
        sampler = sampler_mod.BPRSampler(ptr, flat, n_items, device=Z.device)
    users = np.fromiter(eval_pos.keys(), np.int64, len(eval_pos))
    pos = np.fromiter(eval_pos.values(), np.int64, len(eval_pos))
    ranks = full_rank(Z[:n_users], Z[n_users:n_users + n_items], users, pos, sampler=sampler)
    return metrics_from_ranks(ranks, Ks)


def recommend_topk(Z_users: torch.Tensor, Z_items: torch.Tensor, users=None, k: int = 20, sampler=None,
                   return_scores: bool = True):
    """The recommender's output: for each query user the ``k`` best items outside the user's train
    history, best first under the total order (score descending, item index ascending), scores
    s(i) = <Z_users[u], Z_items[i]> -- bitwise the scores ``full_rank`` compares.

    Returns device tensors ``(idx [n, k] int32, scores [n, k] fp32)`` (``idx`` alone with
    ``return_scores=False``); a user with fewer than ``k`` eligible items has the tail -1 / -inf.
    ``users``: the query users (may repeat); None = every user of ``Z_users`` in order.  Tables
    and ``sampler`` as in ``full_rank``: row or column views of one node table are used in place,
    the sampler's sorted history CSR is the excluded set (None = nothing is excluded).  One fused
    matrix-core pass (``ppgat_full_topk``): the ``[users, items]`` score matrix is never written."""
    for t in (Z_users, Z_items):
        if not t.is_cuda or t.dtype != torch.float32 or t.dim() != 2:
            raise RuntimeError("recommend_topk: 2-D fp32 ROCm tensors required (no CPU path)")
    if Z_users.size(1) != Z_items.size(1) or Z_users.device != Z_items.device:
        raise ValueError("recommend_topk: Z_users and Z_items differ in width or device")
    dev = Z_users.device
    u = None
    if users is not None:
        u = torch.as_tensor(users, dtype=torch.int64).to(dev).contiguous()
        if u.dim() != 1:
            raise ValueError("recommend_topk: users must be 1-D")
    if sampler is not None and (sampler.n_users != Z_users.size(0) or sampler.n_items != Z_items.size(0)):
        raise ValueError("recommend_topk: the sampler's history is over other users / items than the tables")
    n = Z_users.size(0) if u is None else u.numel()
    k = int(k)
    idx = torch.empty(n, k, dtype=torch.int32, device=dev)
    sc = torch.empty(n, k, dtype=torch.float32, device=dev) if return_scores else None
    _launch.full_topk(Z_users, Z_items, u, n, None if sampler is None else sampler.ptr,
                      None if sampler is None else sampler.items, k, idx, sc)
    return (idx, sc) if return_scores else idx


def _held_out_csr(held_out, n: int):
    """(ptr int64 [n + 1], items int64) from a (ptr, items) CSR or a list with one int or one
    sequence of held-out items per query."""
    if isinstance(held_out, tuple) and len(held_out) == 2:
        ptr, items = np.asarray(held_out[0], np.int64), np.asarray(held_out[1], np.int64)
    else:
        rows = [np.atleast_1d(np.asarray(h, np.int64)) for h in held_out]
        ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
        items = np.concatenate(rows) if rows else np.zeros(0, np.int64)
    if len(ptr) != n + 1 or (len(ptr) and ptr[-1] != len(items)):
        raise ValueError("topk_metrics: held_out must have one entry per row of idx")
    return ptr, items


def topk_metrics(idx, held_out, n_items: int, Ks: Sequence[int] = (10, 20)) -> Dict[str, float]:
    """List metrics of top-K recommendations (host numpy).  ``idx`` [n, k]: ``recommend_topk``'s
    lists (-1 = no item); ``held_out``: per query one held-out item or several (a list of ints /
    sequences, or a ``(ptr, items)`` CSR).  Means over the queries with at least one held-out item:

    * ``recall@K``    hits / |held out|  (the LightGCN papers' Recall@K)
    * ``ndcg@K``      DCG / IDCG, IDCG over min(|held out|, K) items
    * ``precision@K`` hits / K
    * ``hit@K``       1 if any held-out item is in the first K
    * ``coverage@K``  distinct items in the first K of all lists / n_items

    With one held-out item per query, ``recall@K`` and ``ndcg@K`` are ``metrics_from_ranks``'
    values for rank = position + 1."""
    if isinstance(idx, torch.Tensor):
        idx = idx.cpu().numpy()
    idx = np.asarray(idx, np.int64)
    if idx.ndim != 2:
        raise ValueError("topk_metrics: idx must be [n, k]")
    n, kmax = idx.shape
    if any(K < 1 or K > kmax for K in Ks):
        raise ValueError(f"topk_metrics: every K must be in [1, {kmax}] (the lists' length)")
    ptr, items = _held_out_csr(held_out, n)
    lens = np.diff(ptr)
    rows = np.repeat(np.arange(n, dtype=np.int64), lens)
    keys = np.unique(rows * n_items + items)  # duplicates in a held-out set count once
    lens = np.bincount(keys // n_items, minlength=n) if n else lens
    hits = (idx >= 0) & np.isin(np.arange(n, dtype=np.int64)[:, None] * n_items + idx, keys)
    have = lens > 0
    disc = np.array([1.0 / math.log2(q + 2) for q in range(kmax)])
    idcg = np.concatenate([[0.0], np.cumsum(disc)])
    out = {}
    per = {}
    for K in Ks:
        h = hits[have, :K]
        nh = h.sum(1)
        m = lens[have]
        per[f"recall@{K}"] = nh / m
        per[f"ndcg@{K}"] = (h * disc[:K]).sum(1) / idcg[np.minimum(m, K)]
        per[f"precision@{K}"] = nh / float(K)
        per[f"hit@{K}"] = (nh > 0).astype(np.float64)
    for name in ("recall", "ndcg", "precision", "hit"):
        for K in Ks:
            v = per[f"{name}@{K}"]
            out[f"{name}@{K}"] = float(np.mean(v)) if len(v) else 0.0
    for K in Ks:
        top = idx[:, :K]
        out[f"coverage@{K}"] = float(len(np.unique(top[top >= 0]))) / float(n_items)
    return out


def eval_topk(model, cfg, item_feats: torch.Tensor, edge_index: torch.Tensor,
              train_pos_idx: Dict[int, np.ndarray], eval_pos: Dict[int, object], Ks=(10, 20), sampler=None,
              edge_attr=None):
    """``eval_full``'s call shape with the metrics that need the lists: the model's forward, the
    max(Ks) best items outside each evaluated user's train history (``recommend_topk``), and
    ``topk_metrics`` against the held-out items.  ``eval_pos`` values: one item or a sequence of
    items per user.  ``cfg`` is unused."""
    with torch.no_grad():
        Z = model(item_feats, edge_index, **_edge_kw(edge_attr))
    n_users, n_items = model.n_users, model.n_items
    if not eval_pos:
        return topk_metrics(np.zeros((0, max(Ks)), np.int64), [], n_items, Ks)
    if sampler is None:
        from . import sampler as sampler_mod
        from .train import user_csr
        ptr, flat = user_csr(train_pos_idx, n_users)
        sampler = sampler_mod.BPRSampler(ptr, flat, n_items, device=Z.device)
    users = np.fromiter(eval_pos.keys(), np.int64, len(eval_pos))
    idx = recommend_topk(Z[:n_users], Z[n_users:n_users + n_items], users, k=max(Ks), sampler=sampler,
                         return_scores=False)
    return topk_metrics(idx, list(eval_pos.values()), n_items, Ks)


def export_item_embeddings(model, item_feats: torch.Tensor, edge_index: torch.Tensor, edge_attr=None) -> np.ndarray:
    """tools/export_item_embeddings.py:139-142: eval-mode no-grad forward, items' rows."""
    model.eval()
    with torch.no_grad():
        Z = model(item_feats, edge_index, **_edge_kw(edge_attr))
        return Z[model.n_users:].detach().cpu().numpy().astype(np.float32)


def attention_topk(model, item_feats: torch.Tensor, edge_index: torch.Tensor, k: int, layer: int = -1,
                   edge_attr=None):
    """The k (1..32) most-attended in-neighbours of every node in layer ``layer`` of a GAT model
    (PyGGAT, PyGGATv2, CustomGAT): ``(src [N, k] int64, weight [N, k] fp32, count [N] int32)``.
    src[i] are source node ids (edge_index[0] of the chosen edges), most attended first, ranked
    by the head-mean attention weight (ties: the earlier edge_index column first), -1 past the
    node's in-degree; weight the head means (0 in the pads); count = min(k, in-degree).  The
    weights are the eval-mode ones (model.attention); they are computed in CSR slot order and
    selected there (ppgat_attention_topk), so no [E, H] array in edge order is formed."""
    from . import hip_ops
    from .model import layer_attention
    layers = model.convs if hasattr(model, "convs") else model.layers
    if edge_attr is not None and getattr(model, "edge_dim", None) is None:
        raise NotImplementedError(f"{type(model).__name__}: edge features are not implemented")
    alpha, = layer_attention(model, layers, item_feats, edge_index, edge_attr, order="slot", only=int(layer))
    graph = hip_ops.graph_cache.get(edge_index, model.n_users + item_feats.size(0))
    eid, val, cnt = hip_ops.attention_topk(graph, alpha, int(k))
    e = eid.long()
    src = torch.where(e >= 0, edge_index[0][e.clamp_min(0)], e) if graph.n_edges else e
    return src, val, cnt


def top_k_batch(item_vecs: torch.Tensor, histories: Sequence[Sequence[int]], k: int = 20):
    """serving/runtime.py:56-76 for a batch of users on the device (ppgat_serve_topk): per
    history, the mean of its rows, scores over every item, the history masked to -1e9, the
    k best descending (ties by smaller index).  Returns (indices [B, k] int64, scores [B, k])."""
    if not item_vecs.is_cuda or item_vecs.dtype != torch.float32:
        raise RuntimeError("top_k_batch: fp32 ROCm item vectors required (no CPU path)")
    iv = item_vecs.contiguous()
    n_items, C = iv.shape
    dev = iv.device
    idx_out, sc_out = [], []
    for b0 in range(0, len(histories), 256):
        chunk = histories[b0:b0 + 256]
        for h in chunk:
            assert len(h) > 0, "Need at least one item id from user history"
        lens = np.array([len(h) for h in chunk], np.int64)
        ptr = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)])).to(dev)
        hist = torch.from_numpy(np.concatenate([np.asarray(h, np.int64) for h in chunk])).to(dev)
        B = len(chunk)
        ws, nbytes = _launch.serve_topk_workspace(n_items, C, B, dev)
        oi = torch.empty(B, k, dtype=torch.int32, device=dev)
        os_ = torch.empty(B, k, dtype=torch.float32, device=dev)
        _launch.serve_topk(iv, ptr, hist, int(lens.max()), B, int(k), oi, os_, ws, nbytes)
        idx_out.append(oi.long())
        sc_out.append(os_)
    return torch.cat(idx_out), torch.cat(sc_out)


def top_k_for_user_items(item_vecs: torch.Tensor, item_ids, k: int = 20):
    """serving/runtime.py:56-76 on the device: (indices, scores) of the top-k items for the
    mean of the history rows, history excluded, descending (ppgat_serve_topk)."""
    assert len(item_ids) > 0, "Need at least one item id from user history"
    idx, sc = top_k_batch(item_vecs, [list(item_ids)], k)
    return idx[0].cpu().numpy(), sc[0].cpu().numpy()
