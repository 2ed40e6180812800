#!/usr/bin/env python3
"""Generate tests/golden/lightgcn_small.npz from the REAL reference code.

Run in the build container only (the reference never travels to the GPU box):

    python tests/golden/make_golden_lightgcn.py

It imports /root/reference/scripts/train_lightgcn.py with ``google.cloud.storage`` (imported
at module top, never used by the math) stubbed, as make_golden.py does, and writes data only:

  scenario   300 users (the last 5 without interactions), 120 items; every 7th user has 17-39
             interactions, the rest 1-7; user 3 repeats an interaction; d = 64, K = 3,
             set_seed(42)
  contents   train_pos_idx in CSR form (user_ptr, user_items); the reference's build_adj output;
             the first 3 batches of sample_bpr_batches(neg_per_pos=5, batch_size=256) under
             random.seed(42); per batch the parameters BEFORE it (batch 0: the initial weights;
             then the reference's own loop: Adam lr 1e-3, weight decay 1e-4), the reference's
             fp32 loss, and loss / dE_user / dE_item recomputed in float64 (dense A, autograd)
             at those parameters.
"""
from __future__ import annotations

import importlib.util
import random
import sys
import types
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
REF = Path("/root/reference")
N_USERS, N_ITEMS, ISO_USERS, D, K = 300, 120, 5, 64, 3
NEG_PER_POS, BATCH, N_BATCHES = 5, 256, 3


def load_reference():
    google = sys.modules.setdefault("google", types.ModuleType("google"))
    cloud = types.ModuleType("google.cloud")
    storage = types.ModuleType("google.cloud.storage")
    storage.Client = object
    cloud.storage = storage
    google.cloud = cloud
    sys.modules["google.cloud"] = cloud
    sys.modules["google.cloud.storage"] = storage
    spec = importlib.util.spec_from_file_location("ref_train_lightgcn", REF / "scripts" / "train_lightgcn.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def scenario():
    rng = np.random.default_rng(2024)
    tr = {}
    for u in range(N_USERS - ISO_USERS):
        d = int(rng.integers(17, 40)) if u % 7 == 0 else int(rng.integers(1, 8))
        tr[u] = rng.choice(N_ITEMS, size=d, replace=False).astype(np.int64)
    tr[3] = np.concatenate([tr[3], tr[3][:1]])  # a repeated interaction
    return tr


def main():
    ref = load_reference()
    tr = scenario()
    ref.set_seed(42)
    adj_idx, adj_vals = ref.build_adj(N_USERS, N_ITEMS, tr)
    model = ref.LightGCN(N_USERS, N_ITEMS, D, adj_idx, adj_vals)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=1e-4)
    out = {"n_users": N_USERS, "n_items": N_ITEMS, "embed_dim": D, "n_layers": K, "neg_per_pos": NEG_PER_POS,
           "batch_size": BATCH,
           "user_ptr": np.concatenate([[0], np.cumsum([len(tr.get(u, ())) for u in range(N_USERS)])]).astype(np.int64),
           "user_items": np.concatenate([tr[u] for u in range(N_USERS) if u in tr]).astype(np.int64),
           "adj_indices": adj_idx.numpy(), "adj_values": adj_vals.numpy()}  # b0_E_* are the initial weights
    A64 = torch.zeros(N_USERS + N_ITEMS, N_USERS + N_ITEMS, dtype=torch.float64)
    A64.index_put_((adj_idx[0], adj_idx[1]), adj_vals.double(), accumulate=True)
    random.seed(42)
    gen = ref.sample_bpr_batches(tr, N_ITEMS, NEG_PER_POS, BATCH)
    for b in range(N_BATCHES):
        u_arr, i_arr, j_arr = next(gen)
        out[f"b{b}_u"], out[f"b{b}_i"], out[f"b{b}_j"] = u_arr, i_arr, j_arr
        out[f"b{b}_E_user"] = model.E_user.weight.detach().numpy().copy()
        out[f"b{b}_E_item"] = model.E_item.weight.detach().numpy().copy()
        # float64 at the stored parameters
        eu = model.E_user.weight.detach().double().requires_grad_(True)
        ei = model.E_item.weight.detach().double().requires_grad_(True)
        x = acc = torch.cat([eu, ei])
        for _ in range(K):
            x = A64 @ x
            acc = acc + x
        acc = acc / (K + 1)
        U, I = acc[:N_USERS], acc[N_USERS:]
        u, i, j = (torch.from_numpy(a).long() for a in (u_arr, i_arr, j_arr))
        l64 = -torch.log(torch.sigmoid((U[u] * I[i]).sum(-1) - (U[u] * I[j]).sum(-1)) + 1e-8).mean()
        l64.backward()
        out[f"b{b}_loss64"] = np.float64(l64.item())
        out[f"b{b}_dE_user64"], out[f"b{b}_dE_item64"] = eu.grad.numpy(), ei.grad.numpy()
        # the reference's own step (train_lightgcn.py:319-334)
        U_emb, I_emb = model.propagate(K)
        pos = (U_emb[u] * I_emb[i]).sum(dim=-1)
        neg = (U_emb[u] * I_emb[j]).sum(dim=-1)
        loss = -torch.log(torch.sigmoid(pos - neg) + 1e-8).mean()
        opt.zero_grad()
        loss.backward()
        ge = (model.E_user.weight.grad.double() - eu.grad).norm(dim=1)
        gn = eu.grad.norm(dim=1)
        print(f"batch {b}: loss fp32 {loss.item():.8f} fp64 {l64.item():.10f}; reference fp32 dE_user per-row rel "
              f"{float((ge[gn > 0] / gn[gn > 0]).max()):.2e}, isolated rows max "
              f"{float(model.E_user.weight.grad[N_USERS - ISO_USERS:].abs().max()):.1e}")
        out[f"b{b}_loss32"] = np.float32(loss.item())
        opt.step()
    path = HERE / "lightgcn_small.npz"
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({path.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
