#!/usr/bin/env python3
"""The shared-negatives softmax loss on the config-2 stand-in (data.synthetic_ui_graph(seed=42)):
S = 200,000 samples, C in {64, 128}, one pool of P in {256, 1024, 4096} items, the train history
excluded, eager.

  (a) loss forward + backward alone: ``hip_ops.shared_softmax_loss`` against the same loss in fp32
      torch ops on the same GPU (index_select, matmul, masked_fill with the precomputed dense mask,
      logsumexp, autograd), after checking that the two agree (loss and gradient), and against
      ``hip_ops.softmax_loss`` at M = 16 and 64 private negatives, all alternating in one process;
      the forward product's fp32-equivalent TFLOP/s (2 S P C / forward time) beside
      ``evaluation.full_rank`` on the same product shape (S entries against a P-item table);
  (b) the whole two-layer PyGGAT step (train.epoch_step) with BPR, the sampled softmax at M = 16
      and the shared pool at P = 1024.

Method: everything warmed up; timing windows alternate between the contenders, each window timed
with device events around a batch of calls that fills >= ``--window-s``; the median of
``--windows`` windows is reported with their spread (max - min) / median.  Prints one JSON line
and writes it to ``--out`` (default profiles/shared_softmax_bench.json).
"""
import argparse
import gc
import importlib
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
pkg = importlib.import_module("plotpointe-gat-recommendation_amd")
hip_ops = importlib.import_module(pkg.__name__ + ".hip_ops")
train = importlib.import_module(pkg.__name__ + ".train")

S = 200_000
WIDTHS = [64, 128]
POOLS = [256, 1024, 4096]
PRIVATE = [16, 64]
WINDOW_S, WINDOWS = 0.3, 5


def window(fn, seconds: float, calls: int):
    """(seconds per call, calls) by device events over ``calls`` calls, doubled until the window is filled."""
    while True:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        dt = a.elapsed_time(b) / 1e3
        if dt >= seconds:
            return dt / calls, calls
        calls *= 2


def alternate(fns: dict, seconds: float, windows: int):
    got = {k: [] for k in fns}
    calls = {k: 2 for k in fns}
    for _ in range(windows):
        for k, fn in fns.items():
            t, calls[k] = window(fn, seconds, calls[k])
            got[k].append(t)
    out = {}
    for k, v in got.items():
        med = statistics.median(v)
        out[k] = {"median_ms": 1e3 * med, "spread": (max(v) - min(v)) / med, "windows_ms": [1e3 * t for t in v]}
    return out


def note(msg):
    print(f"[shared_softmax_bench] {msg}", file=sys.stderr, flush=True)


def dense_mask(smp, u, pos, pool):
    """bool [S, P] on the device: pool[j] is the sample's positive or in its user's train history."""
    owner = torch.repeat_interleave(torch.arange(smp.n_users, device=u.device), smp.ptr[1:] - smp.ptr[:-1])
    items = smp.items[:smp.nnz].long()
    k = torch.searchsorted(pool, items).clamp_max(pool.numel() - 1)
    hit = pool[k] == items
    seen = torch.zeros(smp.n_users, pool.numel(), dtype=torch.bool, device=u.device)  # [n_users, P]
    seen[owner[hit], k[hit]] = True
    return seen[u] | (pool.unsqueeze(0) == pos.unsqueeze(1))


def torch_loss(Z, n_users, u, pos, pool, mask, tau):
    U = Z.index_select(0, u)
    s0 = (U * Z.index_select(0, n_users + pos)).sum(-1) / tau
    s = (U @ Z.index_select(0, n_users + pool).T / tau).masked_fill(mask, float("-inf"))
    return (torch.logsumexp(torch.cat([s0.unsqueeze(1), s], 1), dim=1) - s0).mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window-s", type=float, default=WINDOW_S)
    ap.add_argument("--windows", type=int, default=WINDOWS)
    ap.add_argument("--small", action="store_true", help="a 3,000-user graph, S = 20,000 (rehearsal of the tool, not a result)")
    ap.add_argument("--no-step", action="store_true", help="skip (b), the whole training step")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "shared_softmax_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("shared_softmax_bench: a ROCm GPU is required (nothing here is measured on the host)")
    dev = torch.device("cuda", 0)
    g = (pkg.data.synthetic_ui_graph(n_users=3000, n_items=800, n_interactions=40_000, seed=5) if args.small
         else pkg.data.synthetic_ui_graph(seed=42))
    n_samples = 20_000 if args.small else S
    pools = [p for p in POOLS if p <= g.n_items]
    n = g.n_users + g.n_items
    tr = g.train_pos_idx()
    ei = pkg.data.build_edge_index(g.n_users, g.n_items, tr).to(dev)
    feats = torch.from_numpy(pkg.data.synthetic_item_features(g.n_items, 128)).to(dev)
    ptr, flat = train.user_csr(tr, g.n_users)
    smp = pkg.sampler.BPRSampler(ptr, flat, g.n_items, device=dev)
    u, i, j = smp.sample(n_samples, seed=42)
    cands = {M: smp.eval_candidates(u, i, M, seed=42) for M in PRIVATE}
    rng = np.random.default_rng(0)
    res = {"workload": {"nodes": n, "users": g.n_users, "items": g.n_items, "edges": int(ei.size(1)),
                        "samples": n_samples, "small": bool(args.small)},
           "method": f"median of {args.windows} alternating windows of >= {args.window_s} s, device events; "
                     "spread = (max - min) / median; eager", "loss_alone": [], "step": None}

    # (a) the loss alone
    for C in WIDTHS:
        Z = torch.from_numpy((0.1 * rng.standard_normal((n, C))).astype(np.float32)).to(dev).requires_grad_(True)
        for P in pools:
            pool = smp.sample_pool(P, seed=7)
            mask = dense_mask(smp, u, i, pool)

            def shared():
                Z.grad = None
                hip_ops.shared_softmax_loss(Z, g.n_users, u, i, pool, 1.0, history=smp).backward()

            def shared_fwd():
                with torch.no_grad():
                    hip_ops.shared_softmax_loss(Z, g.n_users, u, i, pool, 1.0, history=smp)

            def dense():
                Z.grad = None
                torch_loss(Z, g.n_users, u, i, pool, mask, 1.0).backward()

            Zu, Ip, ip = Z.detach()[:g.n_users], Z.detach().index_select(0, g.n_users + pool), i % P

            def rank():
                pkg.evaluation.full_rank(Zu, Ip, u, ip)

            fns = {"shared": shared, "torch": dense, "shared_fwd": shared_fwd, "full_rank": rank}
            for M in PRIVATE:
                fns[f"private_M{M}"] = (lambda c: lambda: (setattr(Z, "grad", None), hip_ops.softmax_loss(
                    Z, g.n_users, u, c, 1.0).backward()))(cands[M])
            shared()
            lf, gf = float(hip_ops.shared_softmax_loss(Z, g.n_users, u, i, pool, 1.0, history=smp).detach()), Z.grad.clone()
            dense()
            lt, gt = float(torch_loss(Z, g.n_users, u, i, pool, mask, 1.0).detach()), Z.grad.clone()
            agree = {"loss_rel": abs(lf - lt) / abs(lt), "grad_max_rel": float((gf - gt).abs().max() / gt.abs().max()),
                     "masked_fraction": float(mask.float().mean())}
            assert agree["loss_rel"] <= 1e-5 and agree["grad_max_rel"] <= 1e-4, agree
            del gf, gt
            for _ in range(2):
                for f in fns.values():
                    f()
            torch.cuda.synchronize()
            t = alternate(fns, args.window_s, args.windows)
            flop = 2.0 * n_samples * P * C
            row = {"channels": C, "pool": P, "agreement": agree, "times": t,
                   "torch_over_shared": t["torch"]["median_ms"] / t["shared"]["median_ms"],
                   "forward_TFLOPs_fp32_equivalent": flop / (t["shared_fwd"]["median_ms"] / 1e3) / 1e12,
                   "full_rank_TFLOPs_same_shape": flop / (t["full_rank"]["median_ms"] / 1e3) / 1e12}
            note(f"C={C} P={P} " + json.dumps({k: round(v["median_ms"], 4) for k, v in t.items()}) +
                 f" fwd {row['forward_TFLOPs_fp32_equivalent']:.1f} TF, full_rank {row['full_rank_TFLOPs_same_shape']:.1f} TF")
            res["loss_alone"].append(row)
            del mask
            gc.collect()
            torch.cuda.empty_cache()
        del Z
    hip_ops.check_bpr_indices()

    # (b) the whole step
    if not args.no_step:
        torch.manual_seed(42)
        model = pkg.PyGGAT(g.n_users, g.n_items, item_feat_dim=128, hidden=128, layers=2, heads=1, attn_dropout=0.1).to(dev)
        model.train()
        opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=1e-4)
        pool = smp.sample_pool(min(1024, g.n_items), seed=7)
        steps = {"bpr": lambda: train.epoch_step(model, opt, feats, ei, g.n_users, u, i, j, "bpr"),
                 "softmax_M16": lambda: train.epoch_step(model, opt, feats, ei, g.n_users, u, i, j, softmax=(cands[16], 1.0)),
                 f"shared_P{pool.numel()}": lambda: train.epoch_step(model, opt, feats, ei, g.n_users, u, i, j,
                                                                      shared=(pool, smp, 1.0))}
        for _ in range(3):
            for f in steps.values():
                f()
        torch.cuda.synchronize()
        t = alternate(steps, args.window_s, args.windows)
        note(f"step {json.dumps({k: round(v['median_ms'], 4) for k, v in t.items()})}")
        res["step"] = {"model": "PyGGAT(hidden=128, layers=2, heads=1, attn_dropout=0.1), torch Adam, eager", "times": t,
                       "extra_ms_over_bpr": {k: v["median_ms"] - t["bpr"]["median_ms"] for k, v in t.items()}}
    line = json.dumps(res)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
