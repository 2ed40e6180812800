"""Counterpart of tools/export_item_embeddings.py main() (GCS out of scope: local paths).

Rebuilds train_pos / edge_index exactly as in training (:91-114), the model from the
checkpoint's config (:127-137), runs one eval-mode no-grad forward and saves
``Z[n_users:]`` as float32 .npy (:139-145).  Reference checkpoints
``{"state_dict", "config"}`` load directly (same keys).
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

if __package__ in (None, ""):
    import importlib
    sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
    _pkg = importlib.import_module("plotpointe-gat-recommendation_amd")
    data, evaluation, model_mod = _pkg.data, importlib.import_module(_pkg.__name__ + ".evaluation"), _pkg.model
else:
    from . import data, evaluation
    from . import model as model_mod


def model_from_checkpoint(family: str, ckpt: dict, n_users: int, n_items: int, feat_dim: int):
    c = ckpt.get("config", {})
    if family == "gat_pyg":
        m = model_mod.PyGGAT(n_users, n_items, item_feat_dim=feat_dim, hidden=c.get("hidden_dim", 128),
                             layers=c.get("layers", 2), heads=c.get("heads", 1),
                             attn_dropout=c.get("attn_dropout", 0.1),
                             edge_dim=1 if c.get("edge_features", "none") == "rating" else None)
    else:
        m = model_mod.CustomGAT(n_users, n_items, item_feat_dim=feat_dim, hidden=c.get("hidden_dim", 128),
                                layers=c.get("layers", 2))
    m.load_state_dict(ckpt["state_dict"])
    return m


def main(argv=None):
    ap = argparse.ArgumentParser(description="Export item embeddings from GAT checkpoint")
    ap.add_argument("--model-family", choices=["gat_pyg", "gat_custom"], required=True)
    ap.add_argument("--checkpoint", required=True)
    ap.add_argument("--staging-prefix", required=True)
    ap.add_argument("--graphs-prefix", required=True)
    ap.add_argument("--embeddings-prefix", required=True)
    ap.add_argument("--item-features", choices=["fused", "txt"], default="fused")
    ap.add_argument("--out-local", default="tmp/item_embeddings.npy")
    args = ap.parse_args(argv)
    import pandas as pd
    device = torch.device("cuda")
    inter = pd.read_parquet(Path(args.staging_prefix) / "interactions.parquet")
    with open(Path(args.graphs_prefix) / "node_maps.json") as f:
        maps = json.load(f)
    feat_name = "fused_interacted.npy" if args.item_features == "fused" else "txt_interacted.npy"
    feats = np.load(Path(args.embeddings_prefix) / feat_name)
    u2i, i2i = data.index_maps(maps)
    tr, _, _ = data.map_splits_to_index(*data.build_splits(inter), u2i, i2i)
    n_users, n_items = int(maps["n_users"]), int(maps["n_items"])
    edge_index = data.build_edge_index(n_users, n_items, tr).to(device)
    item_feats = torch.tensor(feats, dtype=torch.float32).to(device)
    assert item_feats.shape[0] == n_items
    ckpt = torch.load(args.checkpoint, map_location=device, weights_only=True)
    m = model_from_checkpoint(args.model_family, ckpt, n_users, n_items, item_feats.size(1)).to(device)
    edge_attr = None
    if ckpt.get("config", {}).get("edge_features", "none") == "rating":  # a model trained with --edge-features rating
        edge_attr = torch.from_numpy(data.edge_attr_rating(tr, inter, u2i, i2i)).to(device)
    I = evaluation.export_item_embeddings(m, item_feats, edge_index, edge_attr=edge_attr)
    Path(args.out_local).parent.mkdir(parents=True, exist_ok=True)
    np.save(args.out_local, I)
    print(f"[EXPORT] Wrote item embeddings: {args.out_local} shape={I.shape}")
    return I


if __name__ == "__main__":
    main()
