"""Trainer counterpart of scripts/train_gat_pyg.py / scripts/train_gat_custom.py main().

Same flags, seeds, split/edge-index/sampler code paths, epoch structure (one large BPR
batch per epoch, eval each epoch, best-val checkpoint, reload, test), metrics-JSON schema
``{"best_val_ndcg@20", "val", "test", "config", "notes"}`` and optional JSONL events
(``run_start`` / ``epoch_end`` / ``run_complete``, plotpointe/utils/structured_log.py:19-38).
GCS is out of scope: the ``--*-prefix`` flags name LOCAL directories holding the same file
names (interactions.parquet, node_maps.json, {fused,txt}_interacted.npy); outputs go to
``{models_prefix}/checkpoints/{run_id}.pt`` and ``{models_prefix}/metrics_{run_id}.json``.
``--synthetic cfg1|cfg2`` builds the SURVEY.md 8(d) stand-in inputs instead.
``--model-family lightgcn`` is scripts/train_lightgcn.py's main(): its flags and defaults, the
mini-batch loop over every train interaction x ``--neg-per-pos`` negatives, the same outputs.

    python -m plotpointe_gat_amd.train ...   (or: python plotpointe-gat-recommendation_amd/train.py ...)
"""
from __future__ import annotations

import argparse
import json
import os
import random
import sys
import time
from dataclasses import dataclass
from pathlib import Path
from typing import Any, Dict, Optional

import numpy as np
import torch

if __package__ in (None, ""):  # executed as a file
    import importlib
    sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
    _pkg = importlib.import_module("plotpointe-gat-recommendation_amd")
    data, evaluation, model_mod = _pkg.data, importlib.import_module(_pkg.__name__ + ".evaluation"), _pkg.model
    sampler_mod, lightgcn_mod, optim_mod = _pkg.sampler, _pkg.lightgcn, _pkg.optim
    neighbors_mod = _pkg.neighbors
else:
    from . import data, evaluation
    from . import model as model_mod
    from . import sampler as sampler_mod
    from . import lightgcn as lightgcn_mod
    from . import optim as optim_mod
    from . import neighbors as neighbors_mod


def set_seed(seed: int):
    """train_gat_pyg.py:39-43."""
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    torch.cuda.manual_seed_all(seed)


def enable_determinism(seed: Optional[int] = None):
    """plotpointe/utils/random.py:23-44 (our kernels are deterministic regardless)."""
    if seed is not None:
        set_seed(seed)
    os.environ.setdefault("CUBLAS_WORKSPACE_CONFIG", ":16:8")
    try:
        torch.use_deterministic_algorithms(True, warn_only=True)
    except Exception:
        pass


def log_event(event: str, run_id: Optional[str] = None, **fields: Any) -> Dict[str, Any]:
    """plotpointe/utils/structured_log.py:19-38."""
    rec: Dict[str, Any] = {"ts": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()), "event": event}
    if run_id:
        rec["run_id"] = run_id
    rec.update(fields)
    try:
        sys.stdout.write(json.dumps(rec) + os.linesep)
        sys.stdout.flush()
    except Exception:
        pass
    return rec


@dataclass
class Config:
    """train_gat_pyg.py:46-65 (+ model_family, attn_dropout exposed)."""
    project_id: str
    region: str
    staging_prefix: str
    graphs_prefix: str
    embeddings_prefix: str
    models_prefix: str
    hidden_dim: int = 128
    layers: int = 2
    heads: int = 1
    attn_dropout: float = 0.1
    lr: float = 1e-3
    l2: float = 1e-4
    epochs: int = 20
    samples_per_epoch: int = 200_000
    seed: int = 42
    eval_neg_k: int = 1000
    item_features: str = "fused"
    loss: str = "bpr"
    model_family: str = "gat_pyg"
    share_weights: bool = False  # gatv2_pyg: lin_r is lin_l
    edge_features: str = "none"  # gat_pyg: "rating" feeds (r - 1) / 4 per edge to GATConv(edge_dim=1)
    negative_sampling: str = "uniform"  # "popularity": negatives drawn in proportion to (train count)^power
    popularity_power: float = 0.75
    logq: str = "auto"           # loss "softmax": subtract log(expected count) from the sampled logits;
    #                              "auto" = on exactly when negative_sampling is "popularity"
    negatives: int = 16          # loss "softmax": sampled negatives per positive (a convention, not tuned)
    temperature: float = 1.0     # loss "softmax": the logits are <u, i> / temperature


@dataclass
class LGCNConfig:
    """train_lightgcn.py:33-48."""
    project_id: str
    region: str
    staging_prefix: str
    graphs_prefix: str
    models_prefix: str
    embed_dim: int = 64
    n_layers: int = 3
    lr: float = 1e-3
    l2: float = 1e-4
    epochs: int = 50
    batch_size: int = 8192
    neg_per_pos: int = 5
    seed: int = 42
    eval_neg_k: int = 1000


def _local(prefix: str) -> Path:
    if prefix.startswith("gs://"):
        raise ValueError(f"{prefix}: GCS is out of scope here; pass a local directory")
    return Path(prefix)


def load_inputs(cfg: Config, synthetic: Optional[str]):
    """-> (train_pos_idx, val_pos_idx, test_pos_idx, n_users, n_items, item_feats np)"""
    if synthetic:
        if synthetic == "cfg1":
            inter = data.synthetic_interactions_small(seed=0)
        elif synthetic == "cfg2":
            g = data.synthetic_ui_graph(seed=42)
            val = {u: int(v) for u, v in enumerate(g.val_item.tolist()) if v >= 0}
            test = {u: int(v) for u, v in enumerate(g.test_item.tolist()) if v >= 0}
            dim = 128 if cfg.item_features == "fused" else 384
            return g.train_pos_idx(), val, test, g.n_users, g.n_items, data.synthetic_item_features(g.n_items, dim)
        else:
            raise ValueError(synthetic)
        maps = data.node_maps_from_interactions(inter)
        feats = np.random.RandomState(0).standard_normal((maps["n_items"], 384)).astype(np.float32)
    else:
        import pandas as pd
        inter = pd.read_parquet(_local(cfg.staging_prefix) / "interactions.parquet")
        with open(_local(cfg.graphs_prefix) / "node_maps.json") as f:
            maps = json.load(f)
        feat_name = "fused_interacted.npy" if cfg.item_features == "fused" else "txt_interacted.npy"
        feats = np.load(_local(cfg.embeddings_prefix) / feat_name)
    u2i, i2i = data.index_maps(maps)
    tr, va, te = data.map_splits_to_index(*data.build_splits(inter), u2i, i2i)
    return tr, va, te, int(maps["n_users"]), int(maps["n_items"]), feats


def load_edge_attr(cfg: Config, synthetic: Optional[str], tr) -> Optional[np.ndarray]:
    """The edge features of ``data.build_edge_index(n_users, n_items, tr)`` under cfg.edge_features:
    None, or the rating weights [E, 1] (data.edge_attr_rating) from the interactions load_inputs
    read (config 2's synthetic graph has no ratings: 1.0 per edge)."""
    if getattr(cfg, "edge_features", "none") == "none":
        return None
    if synthetic == "cfg2":
        return data.edge_attr_rating(tr)
    if synthetic:
        inter = data.synthetic_interactions_small(seed=0)
        maps = data.node_maps_from_interactions(inter)
    else:
        import pandas as pd
        inter = pd.read_parquet(_local(cfg.staging_prefix) / "interactions.parquet")
        with open(_local(cfg.graphs_prefix) / "node_maps.json") as f:
            maps = json.load(f)
    u2i, i2i = data.index_maps(maps)
    return data.edge_attr_rating(tr, inter, u2i, i2i)


def check_edge_features(args):
    """--edge-features other than none: --model-family gat_pyg on one GPU only."""
    if args.edge_features == "none":
        return
    if args.model_family != "gat_pyg":
        raise NotImplementedError(f"--edge-features {args.edge_features} with --model-family {args.model_family} is "
                                  "not implemented: edge features are GATConv's (--model-family gat_pyg)")
    if args.world_size > 1:
        raise NotImplementedError(f"--edge-features {args.edge_features} with --world-size {args.world_size} is not "
                                  "implemented: the sharded layers take no edge features (--world-size 1)")


def check_softmax_loss(args):
    """--loss softmax: the GAT families on one GPU only; --negatives >= 1, --temperature > 0.
    --shared-negatives P > 0 (one pool per epoch instead of per-positive negatives) only with it."""
    if args.shared_negatives < 0:
        raise ValueError("--shared-negatives must be >= 0")
    if args.shared_negatives > 0 and args.loss != "softmax":
        raise ValueError(f"--shared-negatives {args.shared_negatives} needs --loss softmax (got --loss {args.loss})")
    if args.loss != "softmax":
        return
    if args.model_family == "lightgcn":
        raise NotImplementedError("--loss softmax with --model-family lightgcn is not implemented: the LightGCN "
                                  "trainer keeps its mini-batch BPR loss")
    if args.world_size > 1:
        raise NotImplementedError(f"--loss softmax with --world-size {args.world_size} is not implemented: the "
                                  "sharded trainers take the BPR/BCE loss (--world-size 1)")
    if args.negatives < 1:
        raise ValueError("--negatives must be >= 1")
    if not (args.temperature > 0 and args.temperature != float("inf")):
        raise ValueError("--temperature must be finite and > 0")


def check_fanout(args):
    """--fanout F > 0 (fan-out neighbour sampling, neighbors.NeighborSampler): the GAT families on
    one GPU only; F and --fanout-items within the sampler's range, --resample-every >= 1."""
    if args.fanout == 0:
        if args.fanout_items is not None:
            raise ValueError("--fanout-items needs --fanout")
        return
    if args.model_family == "lightgcn":
        raise NotImplementedError("--fanout with --model-family lightgcn is not implemented: LightGCN's adjacency "
                                  "values are degree-normalised, so sampling the graph changes them")
    if args.world_size > 1:
        raise NotImplementedError(f"--fanout with --world-size {args.world_size} is not implemented: the sharded "
                                  "trainers partition the whole graph once (--world-size 1)")
    if not 1 <= args.fanout <= neighbors_mod.MAX_FANOUT:
        raise ValueError(f"--fanout {args.fanout}: expected 1..{neighbors_mod.MAX_FANOUT} (0 = off)")
    if args.fanout_items is not None and not 0 <= args.fanout_items <= neighbors_mod.MAX_FANOUT:
        raise ValueError(f"--fanout-items {args.fanout_items}: expected 0..{neighbors_mod.MAX_FANOUT}")
    if args.resample_every < 1:
        raise ValueError("--resample-every must be >= 1")


def check_subgraph_batch(args):
    """--subgraph-batch B > 0 (mini-batch training on seed subgraphs, neighbors.SubgraphSampler): the
    GAT families on one GPU, private negatives only; it restricts the --fanout sampled graph, so it
    needs --fanout >= 1, and every batch draws its own sample (--resample-every 1)."""
    if args.subgraph_batch == 0:
        return
    if args.subgraph_batch < 0:
        raise ValueError(f"--subgraph-batch {args.subgraph_batch}: expected >= 0 (0 = off)")
    if args.model_family == "lightgcn":
        raise NotImplementedError("--subgraph-batch with --model-family lightgcn is not implemented: the LightGCN "
                                  "trainer has its own mini-batch loop over the whole normalised adjacency")
    if args.world_size > 1:
        raise NotImplementedError(f"--subgraph-batch with --world-size {args.world_size} is not implemented: the "
                                  "sharded trainers partition the whole graph once (--world-size 1)")
    if args.shared_negatives > 0:
        raise NotImplementedError(f"--subgraph-batch with --shared-negatives {args.shared_negatives} is not "
                                  "implemented: the shared pool and the history mask are keyed by global item ids")
    if args.fanout < 1:
        raise ValueError("--subgraph-batch needs --fanout >= 1: a subgraph is a restriction of the sampled graph")
    if args.resample_every != 1:
        raise ValueError("--subgraph-batch draws a sample per batch: --resample-every must stay 1")


def check_sparse_adam(args):
    """--sparse-adam (optim.Adam's lazy row step on the user table, fed by forward_subgraph's
    row-sparse gradient) is the optimiser of the mini-batch trainer: it needs --subgraph-batch > 0."""
    if args.sparse_adam and args.subgraph_batch <= 0:
        raise ValueError("--sparse-adam needs --subgraph-batch > 0: only a mini-batch step leaves user rows untouched")


def subgraph_epoch(model, opt, item_feats, sub_sampler, epoch: int, batch: int, n_users: int, u, i, j,
                   loss: str = "bpr", edge_attr=None, softmax=None, sparse_grad: bool = False):
    """One epoch of mini-batch steps on seed subgraphs.  The epoch's triples (or ``softmax`` =
    (cand [S, M + 1], temperature[, logQ table by global item id])) are cut in order into
    ceil(S / batch) batches; per batch the seeds are its users and ``n_users +`` its items, the
    subgraph is ``sub_sampler.batch(epoch - 1, b, seeds)``, and forward, loss (on ``seed_local``:
    the seeds' local ids in the seeds' order), zero_grad, backward and ``opt.step()`` run on it.
    ``sparse_grad``: the user table's gradient is row-sparse over the batch's users (--sparse-adam).
    Returns (the sample-weighted mean loss, a 0-d tensor; batches; mean nodes; mean edges)."""
    S = int(u.numel())
    n_batches = (S + batch - 1) // batch
    total = torch.zeros((), dtype=torch.float32, device=u.device)
    nodes = edges = 0
    for b in range(n_batches):
        lo_, hi_ = b * batch, min(S, (b + 1) * batch)
        s = hi_ - lo_
        if softmax is not None:
            cand, temperature, *corr = softmax
            items = cand[lo_:hi_].reshape(-1)
        else:
            items = torch.cat([i[lo_:hi_], j[lo_:hi_]])
        sub = sub_sampler.batch(epoch - 1, b, torch.cat([u[lo_:hi_], items + n_users]))
        nus = sub.n_users_s
        ul, il = sub.seed_local[:s].contiguous(), sub.seed_local[s:] - nus
        Z = model.forward_subgraph(item_feats, sub, edge_attr, sparse_grad=sparse_grad)
        if softmax is not None:
            corr_s = corr[0].index_select(0, sub.n_id[nus:] - n_users) if corr else None
            lo = model_mod.softmax_loss(Z, nus, ul, il.view(s, -1), temperature, correction=corr_s)
        else:
            lo = model_mod.bpr_loss(Z, nus, ul, il[:s].contiguous(), il[s:].contiguous(), loss)
        opt.zero_grad()
        lo.backward()
        opt.step()
        total += lo.detach() * s
        nodes += sub.n_nodes
        edges += sub.n_edges
    d = max(n_batches, 1)
    return total / max(S, 1), n_batches, nodes / d, edges / d


def check_negative_sampling(args) -> bool:
    """--negative-sampling / --popularity-power / --logq -> whether the logQ correction is on.
    Popularity sampling and the correction are the GAT families' on one GPU (refused like --loss
    softmax elsewhere); the correction exists for --loss softmax only, and it needs the sampling
    distribution, so --logq on needs --negative-sampling popularity; popularity-weighted BPR/BCE
    negatives come from the device sampler (--fast-sampler)."""
    pop = args.negative_sampling == "popularity"
    if not pop and args.logq != "on":
        return False
    if args.model_family == "lightgcn":
        raise NotImplementedError("--negative-sampling popularity / --logq on with --model-family lightgcn is not "
                                  "implemented: the LightGCN trainer keeps its uniform mini-batch negatives")
    if args.world_size > 1:
        raise NotImplementedError(f"--negative-sampling popularity / --logq on with --world-size {args.world_size} is "
                                  "not implemented: the sharded trainers draw uniform negatives (--world-size 1)")
    if not pop:
        raise ValueError("--logq on needs --negative-sampling popularity: the correction is the log of the sampling "
                         "distribution, which the uniform samplers do not carry")
    if not (args.popularity_power >= 0 and args.popularity_power != float("inf")):
        raise ValueError("--popularity-power must be finite and >= 0")
    if args.loss != "softmax":
        if args.logq == "on":
            raise ValueError(f"--logq on with --loss {args.loss}: the correction is the sampled softmax's; no "
                             "correction exists for the pairwise losses")
        if not args.fast_sampler:
            raise ValueError(f"--negative-sampling popularity with --loss {args.loss} needs --fast-sampler: the "
                             "weighted negatives are drawn by the device sampler")
        return False
    return args.logq != "off"


def build_model(cfg: Config, n_users: int, n_items: int, feat_dim: int):
    if cfg.model_family == "gat_pyg":
        return model_mod.PyGGAT(n_users, n_items, item_feat_dim=feat_dim, hidden=cfg.hidden_dim, layers=cfg.layers,
                                heads=cfg.heads, attn_dropout=cfg.attn_dropout,
                                edge_dim=1 if getattr(cfg, "edge_features", "none") == "rating" else None)
    if cfg.model_family == "gatv2_pyg":
        return model_mod.PyGGATv2(n_users, n_items, item_feat_dim=feat_dim, hidden=cfg.hidden_dim, layers=cfg.layers,
                                  heads=cfg.heads, attn_dropout=cfg.attn_dropout, share_weights=cfg.share_weights)
    m = model_mod.CustomGAT(n_users, n_items, item_feat_dim=feat_dim, hidden=cfg.hidden_dim, layers=cfg.layers)
    for layer in m.layers:
        layer.drop.p = cfg.attn_dropout
    return m


def epoch_step(model, opt, item_feats, edge_index, n_users: int, u, i, j, loss: str = "bpr", edge_attr=None,
               softmax=None, shared=None):
    """One epoch's optimisation step on one GPU (train_gat_custom.py:349-362, identical
    train_gat_pyg.py:307-323): the training forward over the whole graph, the BPR/BCE loss of
    the epoch's sampled triples, zero_grad, backward, ``opt.step()``.  Returns the loss.
    ``PPGAT_BPR_OVERLAP=1`` starts the loss backward's triple sort (it needs the triples only)
    on a side stream before the forward (hip_ops.bpr_prepare; measured no faster at config 2,
    DESIGN.md section 4).  ``softmax`` = (cand [S, M + 1], temperature): the sampled-softmax loss of
    those candidates (column 0 the positive of u) instead; ``loss``, i and j are then not used.
    Either tuple may end with a logQ correction table (fp32 [n_items]) for its loss.
    ``shared`` = (pool [P], history, temperature): the shared-negatives softmax loss of the positives i
    against that pool, ``history`` (the device sampler) excluded; ``loss`` and j are then not used."""
    if shared is not None:
        pool, history, temperature, *corr = shared
        Z = model(item_feats, edge_index) if edge_attr is None else model(item_feats, edge_index, edge_attr)
        lo = model_mod.shared_softmax_loss(Z, n_users, u, i, pool, temperature, history=history,
                                           correction=corr[0] if corr else None)
        opt.zero_grad()
        lo.backward()
        opt.step()
        return lo
    if softmax is not None:
        cand, temperature, *corr = softmax
        Z = model(item_feats, edge_index) if edge_attr is None else model(item_feats, edge_index, edge_attr)
        lo = model_mod.softmax_loss(Z, n_users, u, cand, temperature, correction=corr[0] if corr else None)
        opt.zero_grad()
        lo.backward()
        opt.step()
        return lo
    prep = None
    if os.environ.get("PPGAT_BPR_OVERLAP", "0") == "1":
        C = model.user_emb.weight.size(1)
        prep = model_mod.hip_ops.bpr_prepare(n_users + model.n_items, n_users, model.n_items, C, u, i, j)
    Z = model(item_feats, edge_index) if edge_attr is None else model(item_feats, edge_index, edge_attr)
    lo = model_mod.bpr_loss(Z, n_users, u, i, j, loss, prepared=prep)
    opt.zero_grad()
    lo.backward()
    opt.step()
    return lo


def user_csr(train_pos_idx: Dict[int, np.ndarray], n_users: int):
    """(ptr [n_users + 1], items) over the train lists in user order, each list in its own order."""
    lens = np.array([len(train_pos_idx.get(uu, ())) for uu in range(n_users)], dtype=np.int64)
    ptr = np.concatenate([[0], np.cumsum(lens)])
    flat = np.concatenate([np.asarray(train_pos_idx[uu], dtype=np.int64) for uu in range(n_users) if lens[uu]] or
                          [np.zeros(0, dtype=np.int64)])
    return ptr, flat


FULL_EVAL_NOTE = ("Evaluation ranks the held-out positive against every item outside the user's train history "
                  "(full ranking, no sampled negatives).")


def evaluate(args, model, cfg, item_feats, edge_index, tr, eval_pos, dev_sampler, seed, edge_attr=None):
    """One evaluation under --eval-mode: the reference's sampled protocol, or the full ranking."""
    if args.eval_mode == "full":
        return evaluation.eval_full(model, cfg, item_feats, edge_index, tr, eval_pos, sampler=dev_sampler,
                                    edge_attr=edge_attr)
    return evaluation.eval_sampled(model, cfg, item_feats, edge_index, tr, eval_pos, fast=args.fast_eval,
                                   sampler=dev_sampler if args.device_eval else None, seed=seed, edge_attr=edge_attr)


def raw_id_maps(cfg: Config, synthetic: Optional[str], n_users: int, n_items: int):
    """(user_ids [n_users], item_ids [n_items]): the raw id of each node index, from the node maps
    load_inputs read (config 2's synthetic graph has no raw ids: the indices themselves)."""
    if synthetic == "cfg2":
        return np.arange(n_users).astype(str), np.arange(n_items).astype(str)
    if synthetic:
        maps = data.node_maps_from_interactions(data.synthetic_interactions_small(seed=0))
    else:
        with open(_local(cfg.graphs_prefix) / "node_maps.json") as f:
            maps = json.load(f)
    u2i, i2i = data.index_maps(maps)
    user_ids, item_ids = np.full(n_users, "", dtype=object), np.full(n_items, "", dtype=object)
    for raw, idx in u2i.items():
        user_ids[idx] = raw
    for raw, idx in i2i.items():
        item_ids[idx] = raw
    return user_ids.astype(str), item_ids.astype(str)


def write_recommendations(args, cfg: Config, model, item_feats, edge_index, tr, n_users: int, n_items: int,
                          dev_sampler, device, edge_attr=None):
    """--recommend-out: the --recommend-k best items outside each user's train history for EVERY
    user (evaluation.recommend_topk on the model's final embeddings), written as an .npz with
    ``users`` [n_users], ``items`` [n_users, K] (-1 = fewer than K eligible), ``scores`` and the
    raw ids ``user_ids`` / ``item_ids``.  Returns the run record's "recommendations" entry."""
    if dev_sampler is None:
        ptr, flat = user_csr(tr, n_users)
        dev_sampler = sampler_mod.BPRSampler(ptr, flat, n_items, device=device)
    with torch.no_grad():
        Z = model(item_feats, edge_index) if edge_attr is None else model(item_feats, edge_index, edge_attr)
    k = int(args.recommend_k)
    idx, sc = evaluation.recommend_topk(Z[:n_users], Z[n_users:n_users + n_items], None, k=k, sampler=dev_sampler)
    idx, sc = idx.cpu().numpy(), sc.cpu().numpy()
    user_ids, item_ids = raw_id_maps(cfg, args.synthetic, n_users, n_items)
    path = Path(args.recommend_out)
    path.parent.mkdir(parents=True, exist_ok=True)
    with open(path, "wb") as f:
        np.savez(f, users=np.arange(n_users, dtype=np.int64), items=idx, scores=sc, user_ids=user_ids,
                 item_ids=item_ids)
    return {"path": str(path), "k": k, f"coverage@{k}": float(len(np.unique(idx[idx >= 0]))) / float(n_items)}


def write_attention(args, cfg: Config, model, item_feats, edge_index, n_users: int, n_items: int, edge_attr=None):
    """--attention-out: for every user, the --attention-k most-attended in-neighbours of the last
    layer (evaluation.attention_topk; in a user-item graph a user's in-neighbours are the items
    it interacted with), written as an .npz with ``users`` [n_users], ``items`` [n_users, K] (item
    ids, -1 = fewer than K in-edges; a neighbour that is not an item node is -1 too), ``weights``
    (head-mean attention, 0 in the pads) and ``count``.  Returns the run record's "attention" entry."""
    k = int(args.attention_k)
    src, w, cnt = evaluation.attention_topk(model, item_feats, edge_index, k, layer=-1, edge_attr=edge_attr)
    src, w, cnt = src[:n_users].cpu().numpy(), w[:n_users].cpu().numpy(), cnt[:n_users].cpu().numpy()
    items = np.where((src >= n_users) & (src < n_users + n_items), src - n_users, -1).astype(np.int64)
    path = Path(args.attention_out)
    path.parent.mkdir(parents=True, exist_ok=True)
    with open(path, "wb") as f:
        np.savez(f, users=np.arange(n_users, dtype=np.int64), items=items, weights=w, count=cnt)
    return {"path": str(path), "k": k, "layer": cfg.layers - 1, "mean_count": float(cnt.mean()) if len(cnt) else 0.0}


def main_lightgcn(args):
    """train_lightgcn.py main(): the mini-batch loop over every positive x neg_per_pos
    (:313-336), sampled evaluation each epoch, best-val checkpoint on ndcg@20, reload, test."""
    cfg = LGCNConfig(project_id=args.project_id, region=args.region, staging_prefix=args.staging_prefix,
                     graphs_prefix=args.graphs_prefix, models_prefix=args.models_prefix, embed_dim=args.embed_dim,
                     n_layers=3 if args.layers is None else args.layers, lr=1e-3 if args.lr is None else args.lr,
                     l2=1e-4 if args.l2 is None else args.l2, epochs=50 if args.epochs is None else args.epochs,
                     batch_size=args.batch_size, neg_per_pos=args.neg_per_pos, seed=args.seed,
                     eval_neg_k=args.eval_neg_k)
    if args.world_size > 1:
        raise NotImplementedError("--model-family lightgcn runs on one GPU")
    full = args.eval_mode == "full"
    if args.deterministic:
        enable_determinism(cfg.seed)
    set_seed(cfg.seed)
    if not torch.cuda.is_available():
        raise RuntimeError("this trainer runs the HIP kernels: a ROCm GPU is required")
    device = torch.device("cuda")
    run_id = f"lgcn_d{cfg.embed_dim}_{int(time.time())}"
    if args.structured_logs:
        log_event("run_start", run_id=run_id, model_family="lightgcn", config={**cfg.__dict__, "device": str(device)})
    gat_cfg = Config(project_id=args.project_id, region=args.region, staging_prefix=args.staging_prefix,
                     graphs_prefix=args.graphs_prefix, embeddings_prefix=args.embeddings_prefix,
                     models_prefix=args.models_prefix, item_features=args.item_features)
    tr, va, te, n_users, n_items, _ = load_inputs(gat_cfg, args.synthetic)
    # the adjacency and --exact-sampler follow the dict's own order, as the reference does; the device
    # sampler enumerates users ascending (the same enumeration whenever the dict is in user order)
    print(f"[LGCN] n_users={n_users}, n_items={n_items}")
    adj_idx, adj_vals = lightgcn_mod.build_adj(n_users, n_items, tr)
    model = lightgcn_mod.LightGCN(n_users, n_items, cfg.embed_dim, adj_idx, adj_vals, n_layers=cfg.n_layers).to(device)
    opt = optim_mod.Adam(model.parameters(), lr=cfg.lr, weight_decay=cfg.l2)
    out_dir = _local(cfg.models_prefix)
    (out_dir / "checkpoints").mkdir(parents=True, exist_ok=True)
    best_path = out_dir / "checkpoints" / f"{run_id}.pt"
    metrics_path = out_dir / f"metrics_{run_id}.json"
    best = -1.0
    val_metrics: Dict[str, float] = {}
    ptr, flat = user_csr(tr, n_users)
    dev_sampler = sampler_mod.BPRSampler(ptr, flat, n_items, device=device)
    n_batches = dev_sampler.n_batches(cfg.neg_per_pos, cfg.batch_size)
    for epoch in range(1, cfg.epochs + 1):
        model.train()
        total = torch.zeros((), dtype=torch.float32, device=device)
        if args.exact_sampler:
            batches = (tuple(torch.from_numpy(a).long().to(device) for a in b)
                       for b in data.sample_lightgcn_batches(tr, n_items, cfg.neg_per_pos, cfg.batch_size))
        else:
            batches = (dev_sampler.sample_positives(cfg.neg_per_pos, cfg.batch_size, b, seed=cfg.seed + epoch,
                                                    check=False) for b in range(n_batches))
        nb = 0
        for u, i, j in batches:
            total += lightgcn_mod.train_step(model, opt, u, i, j).detach()
            nb += 1
        avg_loss = float(total.item()) / max(1, nb)
        print(f"[LGCN][Epoch {epoch}] train_bpr_loss={avg_loss:.4f}")
        model.eval()
        val_metrics = evaluate(args, model, cfg, None, None, tr, va, dev_sampler, cfg.seed + epoch)
        print(f"[LGCN][Epoch {epoch}] val: {val_metrics}")
        if args.structured_logs:
            log_event("epoch_end", run_id=run_id, epoch=epoch, loss=avg_loss, val=val_metrics)
        if val_metrics.get("ndcg@20", 0.0) > best:
            best = val_metrics.get("ndcg@20", 0.0)
            torch.save({"state_dict": model.state_dict(), "config": cfg.__dict__}, best_path)
            print("[LGCN] Saved new best checkpoint")
    ckpt = torch.load(best_path, map_location=device, weights_only=True)
    model.load_state_dict(ckpt["state_dict"])
    model.eval()
    test_metrics = evaluate(args, model, cfg, None, None, tr, te, dev_sampler, cfg.seed)
    print(f"[LGCN] test: {test_metrics}")
    out = {"best_val_ndcg@20": float(best), "val": val_metrics, "test": test_metrics, "config": cfg.__dict__,
           "notes": "Evaluation uses sampled 1000 negatives/user."}
    if full:
        out["config"] = {**cfg.__dict__, "eval_mode": "full"}
        out["notes"] = FULL_EVAL_NOTE
    if args.recommend_out:
        out["recommendations"] = write_recommendations(args, cfg, model, None, None, tr, n_users, n_items,
                                                       dev_sampler, device)
    with open(metrics_path, "w") as f:
        json.dump(out, f, indent=2)
    print(f"[LGCN] Complete. Wrote {best_path} and {metrics_path}")
    if args.structured_logs:
        log_event("run_complete", run_id=run_id, best_val_ndcg20=float(best), test=test_metrics,
                  artifacts={"checkpoint": str(best_path), "metrics": str(metrics_path)})
    return out


class _GlobalRows(torch.nn.Module):
    """A row-sharded model seen as the single-GPU one by eval_sampled / export: forward returns
    every node's rows on every rank (an all_gather; evaluation only, not the training path)."""

    def __init__(self, sharded, to_global):
        super().__init__()
        self.sharded, self.to_global = sharded, to_global
        self.n_users, self.n_items = sharded.n_users, sharded.n_items

    def forward(self, item_feats, edge_index=None):
        return self.to_global(self.sharded(item_feats), self.sharded.dg, self.sharded.comm)


def _init_distributed(args):
    """torch.distributed from torchrun's env (RANK / WORLD_SIZE / LOCAL_RANK / MASTER_*): one
    process per GPU; several ranks may share a GPU (gloo tests)."""
    import torch.distributed as tdist
    world = int(os.environ.get("WORLD_SIZE", args.world_size))
    if world != args.world_size:
        raise RuntimeError(f"--world-size {args.world_size} but WORLD_SIZE={world} (launch with torchrun)")
    rank = int(os.environ.get("RANK", 0))
    local = int(os.environ.get("LOCAL_RANK", rank))
    device = torch.device("cuda", local % max(torch.cuda.device_count(), 1))
    torch.cuda.set_device(device)
    kw = {"device_id": device} if args.backend == "nccl" else {}
    tdist.init_process_group(args.backend, rank=rank, world_size=world, **kw)
    return rank, world, device


def build_parser():
    ap = argparse.ArgumentParser(description="Train GAT (MI355X-native)")
    ap.add_argument("--project-id", default="local")
    ap.add_argument("--region", default="us-central1")
    ap.add_argument("--staging-prefix", default="data/staging")
    ap.add_argument("--graphs-prefix", default="data/graphs")
    ap.add_argument("--embeddings-prefix", default="data/embeddings")
    ap.add_argument("--models-prefix", default="models/gat")
    ap.add_argument("--model-family", choices=["gat_pyg", "gat_custom", "lightgcn", "gatv2_pyg"], default="gat_pyg",
                    help="gatv2_pyg: PyGGAT with GATv2Conv layers (dynamic attention), one GPU")
    ap.add_argument("--share-weights", action="store_true", help="gatv2_pyg: GATv2Conv(share_weights=True)")
    ap.add_argument("--edge-features", choices=["none", "rating"], default="none",
                    help="gat_pyg on one GPU: rating feeds (r - 1) / 4 of each train interaction to "
                         "GATConv(edge_dim=1) as its edge feature")
    ap.add_argument("--hidden-dim", type=int, default=128)
    ap.add_argument("--layers", type=int, default=None, help="default 2 (GAT), 3 (lightgcn)")
    ap.add_argument("--heads", type=int, default=1)
    ap.add_argument("--attn-dropout", type=float, default=0.1)
    ap.add_argument("--epochs", type=int, default=None, help="default 20 (GAT), 50 (lightgcn)")
    ap.add_argument("--lr", type=float, default=None, help="default 1e-3")
    ap.add_argument("--l2", type=float, default=None, help="Adam weight decay, default 1e-4")
    ap.add_argument("--embed-dim", type=int, default=64, help="lightgcn: embedding width (64, 128 or 256)")
    ap.add_argument("--batch-size", type=int, default=8192, help="lightgcn: triples per mini-batch")
    ap.add_argument("--neg-per-pos", type=int, default=5, help="lightgcn: negatives per train interaction")
    ap.add_argument("--exact-sampler", action="store_true",
                    help="lightgcn: the reference's Python random stream (data.sample_lightgcn_batches) instead "
                         "of the device sampler")
    ap.add_argument("--samples-per-epoch", type=int, default=200_000)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--eval-neg-k", type=int, default=1000)
    ap.add_argument("--item-features", choices=["fused", "txt"], default="fused")
    ap.add_argument("--loss", choices=["bpr", "bce", "softmax"], default="bpr",
                    help="softmax: the sampled softmax of each positive against --negatives device-sampled "
                         "negatives (GAT families, one GPU)")
    ap.add_argument("--negatives", type=int, default=16,
                    help="--loss softmax: negatives per positive; the default 16 is a convention, not a tuned value "
                         "(unused with --shared-negatives)")
    ap.add_argument("--shared-negatives", type=int, default=0, metavar="P",
                    help="--loss softmax: score every positive of an epoch against one pool of P items drawn per "
                         "epoch (the user's train history excluded) instead of --negatives per-positive ones; "
                         "0 = off")
    ap.add_argument("--temperature", type=float, default=1.0,
                    help="--loss softmax: logits are <user, item> / temperature")
    ap.add_argument("--negative-sampling", choices=["uniform", "popularity"], default="uniform",
                    help="popularity: negatives (BPR/BCE j with --fast-sampler, the softmax candidates, the shared "
                         "pool) drawn in proportion to (train count)^--popularity-power (GAT families, one GPU)")
    ap.add_argument("--popularity-power", type=float, default=0.75)
    ap.add_argument("--logq", choices=["auto", "on", "off"], default="auto",
                    help="--loss softmax: subtract the log of each sampled negative's expected count from its logit; "
                         "auto = on exactly when --negative-sampling popularity")
    ap.add_argument("--deterministic", action="store_true")
    ap.add_argument("--structured-logs", action="store_true")
    ap.add_argument("--fast-eval", action="store_true", help="vectorised negative sampling (same distribution)")
    ap.add_argument("--device-eval", action="store_true",
                    help="eval candidates drawn on the GPU (ppgat_eval_sample: same rule, counter-based stream)")
    ap.add_argument("--fast-sampler", action="store_true",
                    help="BPR triples drawn on the GPU (ppgat_bpr_sample: same rule, counter-based stream)")
    ap.add_argument("--synthetic", choices=["cfg1", "cfg2"], default=None)
    ap.add_argument("--world-size", type=int, default=1,
                    help="ranks (one process per GPU, launched by torchrun); > 1 shards the model (dist.py)")
    ap.add_argument("--backend", choices=["nccl", "gloo"], default="nccl",
                    help="torch.distributed backend (nccl = RCCL on ROCm; gloo only for tests)")
    ap.add_argument("--partition", choices=["auto", "replicated", "halo"], default="auto",
                    help="auto: users sharded / items replicated for U-I graphs, halo otherwise")
    ap.add_argument("--eval-mode", choices=["sampled", "full"], default="sampled",
                    help="sampled: the reference's 1 positive + --eval-neg-k negatives; full: the positive against "
                         "every item outside the user's train history (ppgat_full_rank), one GPU")
    ap.add_argument("--recommend-out", default=None, metavar="PATH",
                    help="after the test evaluation, write every user's --recommend-k best items outside the train "
                         "history (ppgat_full_topk) to this .npz; one GPU")
    ap.add_argument("--recommend-k", type=int, default=20)
    ap.add_argument("--attention-out", default=None, metavar="PATH",
                    help="after training, write every user's --attention-k most-attended items of the last layer "
                         "(ppgat_attention_topk) to this .npz; one GPU, GAT families only")
    ap.add_argument("--attention-k", type=int, default=10)
    ap.add_argument("--fanout", type=int, default=0, metavar="F",
                    help="train each epoch on a sampled graph: at most F in-neighbours per destination, drawn "
                         "uniformly without replacement on the GPU (1..64; 0 = off, the whole graph).  Evaluation "
                         "and the exports keep the whole graph.  GAT families, one GPU")
    ap.add_argument("--fanout-items", type=int, default=None, metavar="F2",
                    help="--fanout: the cap of the item destinations instead of F (0..64)")
    ap.add_argument("--resample-every", type=int, default=1, metavar="K",
                    help="--fanout: draw a new sampled graph every K epochs")
    ap.add_argument("--subgraph-batch", type=int, default=0, metavar="B",
                    help="--fanout: cut the epoch's triples into batches of B and take one optimiser step per batch, "
                         "on the --layers-hop sampled subgraph of the batch's users and items alone (0 = off: one "
                         "step per epoch).  Evaluation and the exports keep the whole graph.  GAT families, one GPU")
    ap.add_argument("--sparse-adam", action="store_true",
                    help="--subgraph-batch: lazy row-sparse Adam on the user table (ppgat_adam_rows): each batch "
                         "updates its own user rows alone; untouched rows get no momentum step and no weight decay")
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    check_edge_features(args)
    check_softmax_loss(args)
    check_subgraph_batch(args)
    check_sparse_adam(args)
    check_fanout(args)
    logq = check_negative_sampling(args)
    if args.recommend_out and args.world_size > 1:
        raise NotImplementedError("--recommend-out runs on one GPU (--world-size 1): the lists are made from the "
                                  "whole user and item tables")
    if args.attention_out and args.world_size > 1:
        raise NotImplementedError("--attention-out runs on one GPU (--world-size 1): the sharded models return no "
                                  "attention weights")
    if args.attention_out and args.model_family == "lightgcn":
        raise NotImplementedError("--attention-out with --model-family lightgcn is not implemented: LightGCN has no "
                                  "attention weights")
    if args.attention_out and not 1 <= args.attention_k <= 32:
        raise ValueError(f"--attention-k {args.attention_k}: expected 1..32")
    full = args.eval_mode == "full"
    if full and args.world_size > 1:
        raise NotImplementedError("--eval-mode full runs on one GPU (the sharded trainers evaluate sampled)")
    if args.model_family == "gatv2_pyg" and args.world_size > 1:
        raise NotImplementedError("--model-family gatv2_pyg runs on one GPU (the sharded model is PyGGAT)")
    if args.model_family == "lightgcn":
        return main_lightgcn(args)
    args.layers = 2 if args.layers is None else args.layers
    args.epochs = 20 if args.epochs is None else args.epochs
    cfg = Config(project_id=args.project_id, region=args.region, staging_prefix=args.staging_prefix,
                 graphs_prefix=args.graphs_prefix, embeddings_prefix=args.embeddings_prefix,
                 models_prefix=args.models_prefix, hidden_dim=args.hidden_dim, layers=args.layers, heads=args.heads,
                 attn_dropout=args.attn_dropout, epochs=args.epochs, samples_per_epoch=args.samples_per_epoch,
                 seed=args.seed, eval_neg_k=args.eval_neg_k, item_features=args.item_features, loss=args.loss,
                 model_family=args.model_family, share_weights=args.share_weights,
                 edge_features=args.edge_features, negatives=args.negatives, temperature=args.temperature,
                 negative_sampling=args.negative_sampling, popularity_power=args.popularity_power, logq=args.logq)
    if args.lr is not None:
        cfg.lr = args.lr
    if args.l2 is not None:
        cfg.l2 = args.l2
    if args.deterministic:
        enable_determinism(cfg.seed)
    set_seed(cfg.seed)
    if not torch.cuda.is_available():
        raise RuntimeError("this trainer runs the HIP kernels: a ROCm GPU is required")
    rank, world, device = 0, 1, torch.device("cuda")
    if args.world_size > 1:
        if cfg.model_family != "gat_pyg":
            raise NotImplementedError("--world-size > 1: the sharded model is PyGGAT (--model-family gat_pyg)")
        rank, world, device = _init_distributed(args)
    lead = rank == 0
    tag = {"gat_pyg": "GAT-PYG", "gatv2_pyg": "GATV2-PYG"}.get(cfg.model_family, "GAT-CUSTOM")
    run_id = f"{cfg.model_family}_d{cfg.hidden_dim}_{int(time.time())}"
    if world > 1:  # one run id (checkpoint / metrics names) for every rank: rank 0's
        import torch.distributed as tdist
        ids = [run_id]
        tdist.broadcast_object_list(ids, src=0)
        run_id = ids[0]
    if args.structured_logs:
        log_event("run_start", run_id=run_id, model_family=cfg.model_family,
                  config={**cfg.__dict__, "device": str(device)})
    tr, va, te, n_users, n_items, feats_np = load_inputs(cfg, args.synthetic)
    print(f"[{tag}] n_users={n_users}, n_items={n_items}")
    if args.shared_negatives > n_items:
        raise ValueError(f"--shared-negatives {args.shared_negatives} exceeds the catalogue ({n_items} items)")
    edge_index = data.build_edge_index(n_users, n_items, tr).to(device)
    item_feats = torch.tensor(feats_np, dtype=torch.float32).to(device)
    assert item_feats.shape[0] == n_items
    ea_np = load_edge_attr(cfg, args.synthetic, tr)
    edge_attr = torch.from_numpy(ea_np).to(device) if ea_np is not None else None  # one tensor for the whole run
    model = build_model(cfg, n_users, n_items, item_feats.size(1)).to(device)
    sharded = None
    if world > 1:
        # every rank built the same full model (same seed); each keeps its shard
        import importlib
        dist_mod = importlib.import_module(model_mod.__name__.rsplit(".", 1)[0] + ".dist")
        comm = dist_mod.Comm()
        part = args.partition
        if part == "auto":
            part = "replicated"
        if part == "replicated":
            dg = dist_mod.build_replicated_graph(edge_index, n_users + n_items, n_users, world, rank)
            sharded = dist_mod.ReplicatedPyGGAT(model, dg, comm)
            loss_fn, to_global = dist_mod.replicated_bpr_loss, dist_mod.replicated_rows_to_global
        else:
            dg = dist_mod.build_halo_graph(edge_index, n_users + n_items, n_users, world, rank)
            sharded = dist_mod.HaloPyGGAT(model, dg, comm)
            loss_fn, to_global = dist_mod.halo_bpr_loss, dist_mod.halo_rows_to_global
        eval_model = _GlobalRows(sharded, to_global)
        opt = torch.optim.Adam(sharded.parameters(), lr=cfg.lr, weight_decay=cfg.l2)
    else:
        eval_model = model
        if args.sparse_adam:  # n_id is ascending (neighbors.Subgraph): no sort per batch
            opt = optim_mod.Adam(model.parameters(), lr=cfg.lr, weight_decay=cfg.l2, rows="ascending")
        else:
            opt = torch.optim.Adam(model.parameters(), lr=cfg.lr, weight_decay=cfg.l2)
    out_dir = _local(cfg.models_prefix)
    (out_dir / "checkpoints").mkdir(parents=True, exist_ok=True)
    best_path = out_dir / "checkpoints" / f"{run_id}.pt"
    metrics_path = out_dir / f"metrics_{run_id}.json"
    best = -1.0
    val_metrics: Dict[str, float] = {}
    dev_sampler = None
    if args.fast_sampler or args.device_eval or full or cfg.loss == "softmax":
        ptr, flat = user_csr(tr, n_users)
        weights = None
        if cfg.negative_sampling == "popularity":  # from the train interactions
            weights = sampler_mod.BPRSampler.popularity_weights(ptr, flat, n_items, cfg.popularity_power)
        dev_sampler = sampler_mod.BPRSampler(ptr, flat, n_items, device=device, item_weights=weights)
    ssm_corr = dev_sampler.correction(cfg.negatives) if logq and args.shared_negatives == 0 else None
    nb_sampler = sub_sampler = None
    if args.fanout > 0:  # one GPU (refused above otherwise)
        fanout_of = None
        if args.fanout_items is not None:  # users keep --fanout (-1 would keep all), items take F2
            fanout_of = torch.full((n_users + n_items,), args.fanout, dtype=torch.int32, device=device)
            fanout_of[n_users:] = args.fanout_items
        if args.subgraph_batch > 0:  # a sample per batch, restricted to the batch's neighbourhood
            sub_sampler = neighbors_mod.SubgraphSampler(edge_index, n_users + n_items, cfg.layers, args.fanout,
                                                        seed=cfg.seed, fanout_of=fanout_of, n_users=n_users)
        else:
            nb_sampler = neighbors_mod.NeighborSampler(edge_index, n_users + n_items, args.fanout, seed=cfg.seed,
                                                       fanout_of=fanout_of)
    step_edges, step_attr = edge_index, edge_attr
    for epoch in range(1, cfg.epochs + 1):
        model.train()
        if nb_sampler is not None and (epoch - 1) % args.resample_every == 0:
            step_edges, eid, _ = nb_sampler.epoch(epoch - 1)
            step_attr = edge_attr.index_select(0, eid) if edge_attr is not None else None
        if args.fast_sampler:
            u, i, j = dev_sampler.sample(cfg.samples_per_epoch, seed=cfg.seed,
                                         offset=(epoch - 1) * cfg.samples_per_epoch)
        else:
            u_arr, i_arr, j_arr = data.sample_bpr_epoch(tr, n_items, cfg.samples_per_epoch)
            u = torch.from_numpy(u_arr).long().to(device)
            i = torch.from_numpy(i_arr).long().to(device)
            j = torch.from_numpy(j_arr).long().to(device)
        if sharded is None:
            softmax = shared = None
            if cfg.loss == "softmax" and args.shared_negatives > 0:  # one pool for the epoch's positives
                shared = (dev_sampler.sample_pool(args.shared_negatives, cfg.seed + epoch), dev_sampler,
                          cfg.temperature)
                if logq:  # the pool's inclusion probabilities depend on how many draws it took
                    shared += (dev_sampler.pool_correction(),)
            elif cfg.loss == "softmax":  # the negatives always come from the device sampler
                softmax = (dev_sampler.train_candidates(u, i, cfg.negatives, seed=cfg.seed + epoch), cfg.temperature)
                if logq:
                    softmax += (ssm_corr,)
            if sub_sampler is not None:
                lo, *sub_stats = subgraph_epoch(model, opt, item_feats, sub_sampler, epoch, args.subgraph_batch,
                                                n_users, u, i, j, cfg.loss, edge_attr=edge_attr, softmax=softmax,
                                                sparse_grad=args.sparse_adam)
                loss_val = float(lo.item())
                if args.sparse_adam:  # the loss is on the host: the row-contract flag costs no wait of its own
                    opt.check_rows()
            else:
                loss_val = float(epoch_step(model, opt, item_feats, step_edges, n_users, u, i, j, cfg.loss,
                                            edge_attr=step_attr, softmax=softmax, shared=shared).item())
        else:
            # each rank: its own users' triples (the sum over ranks is the reference's mean),
            # dense gradients all-reduced, user rows updated by their owner
            sharded.train()
            Zl = sharded(item_feats)
            loss = loss_fn(Zl, sharded.dg, sharded.comm, u, i, j, n_users, n_items, loss=cfg.loss,
                           plan_key=epoch)  # one triple draw per epoch, the same epoch on every rank
            opt.zero_grad()
            loss.backward()
            sharded.allreduce_grads()
            opt.step()
            tot = loss.detach().clone()
            sharded.comm.all_reduce_(tot)
            loss_val = float(tot.item())
        if lead:
            print(f"[{tag}][Epoch {epoch}] loss={loss_val:.4f} ({cfg.loss})")
        eval_model.eval()
        val_metrics = evaluate(args, eval_model, cfg, item_feats, edge_index, tr, va, dev_sampler, cfg.seed + epoch,
                               edge_attr=edge_attr)
        if lead:
            print(f"[{tag}][Epoch {epoch}] val: {val_metrics}")
        if args.structured_logs and lead:
            sampled = {"sampled_edges": int(step_edges.size(1))} if nb_sampler is not None else {}
            if sub_sampler is not None:
                sampled = {"batches": sub_stats[0], "mean_sub_nodes": sub_stats[1], "mean_sub_edges": sub_stats[2]}
            log_event("epoch_end", run_id=run_id, epoch=epoch, loss=loss_val, val=val_metrics, **sampled)
        if val_metrics.get("ndcg@20", 0.0) > best:
            best = val_metrics.get("ndcg@20", 0.0)
            sd = model.state_dict() if sharded is None else sharded.full_state_dict()  # collective when sharded
            if lead:
                torch.save({"state_dict": sd, "config": cfg.__dict__}, best_path)
                print(f"[{tag}] Saved new best checkpoint")
    if world > 1:
        import torch.distributed as tdist
        tdist.barrier()  # rank 0's checkpoint is on disk
    ckpt = torch.load(best_path, map_location=device, weights_only=True)
    model.load_state_dict(ckpt["state_dict"])
    if sharded is not None:
        with torch.no_grad():
            ids = torch.as_tensor(sharded.dg.own_user_ids(), dtype=torch.int64, device=model.user_emb.weight.device)
            sharded.user_emb_local.copy_(model.user_emb.weight.index_select(0, ids))
    eval_model.eval()
    test_metrics = evaluate(args, eval_model, cfg, item_feats, edge_index, tr, te, dev_sampler, cfg.seed,
                            edge_attr=edge_attr)
    if lead:
        print(f"[{tag}] test: {test_metrics}")
    out = {"best_val_ndcg@20": float(best), "val": val_metrics, "test": test_metrics, "config": cfg.__dict__,
           "notes": f"One-backward-per-epoch with S sampled BPR triples; features={cfg.item_features}; "
                    f"loss={cfg.loss}"}
    if cfg.loss == "softmax" and args.shared_negatives > 0:
        out["notes"] += (f" ({args.shared_negatives} negatives shared across each epoch's positives, train history "
                         f"excluded, temperature {cfg.temperature}; --negatives unused)")
    elif cfg.loss == "softmax":
        out["notes"] += f" ({cfg.negatives} sampled negatives per positive, temperature {cfg.temperature})"
    if cfg.negative_sampling == "popularity":
        out["notes"] += (f"; negatives drawn in proportion to (train count)^{cfg.popularity_power}, logQ correction "
                         f"{'on' if logq else 'off'}")
    if sub_sampler is not None:
        out["notes"] += (f"; --subgraph-batch {args.subgraph_batch}: one optimiser step per batch of triples, on the "
                         f"{cfg.layers}-hop fan-out {args.fanout} subgraph of the batch's users and items")
    if args.sparse_adam:
        out["notes"] += ("; --sparse-adam: lazy row-sparse Adam on the user table -- user rows outside a batch's "
                         "subgraph are untouched by its step: no momentum coasting and no weight decay for them")
    if full:
        out["config"] = {**cfg.__dict__, "eval_mode": "full"}
        out["notes"] += "; " + FULL_EVAL_NOTE
    if args.recommend_out:  # one GPU (refused above otherwise)
        out["recommendations"] = write_recommendations(args, cfg, model, item_feats, edge_index, tr, n_users, n_items,
                                                       dev_sampler, device, edge_attr=edge_attr)
    if args.attention_out:  # one GPU (refused above otherwise)
        out["attention"] = write_attention(args, cfg, model, item_feats, edge_index, n_users, n_items,
                                           edge_attr=edge_attr)
    if world > 1:
        import torch.distributed as tdist
        tdist.destroy_process_group()
        if not lead:
            return out
    with open(metrics_path, "w") as f:
        json.dump(out, f, indent=2)
    print(f"[{tag}] Complete. Wrote {best_path} and {metrics_path}")
    if args.structured_logs:
        log_event("run_complete", run_id=run_id, best_val_ndcg20=float(best), test=test_metrics,
                  artifacts={"checkpoint": str(best_path), "metrics": str(metrics_path)})
    return out


if __name__ == "__main__":
    main()
