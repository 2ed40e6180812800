#!/usr/bin/env python3
"""The sampled-softmax loss on the config-2 stand-in (data.synthetic_ui_graph(seed=42)): S = 200,000
samples, C = 128, M in {1, 4, 16, 64} negatives per positive, eager.

  (a) loss forward + backward alone: ``hip_ops.softmax_loss`` against the same loss in fp32 torch
      ops on the same GPU (index_select, a batched dot, logsumexp, autograd), after checking that
      the two agree (loss and gradient);
  (b) the whole two-layer PyGGAT step (train.epoch_step) with the softmax loss at each M, against
      the BPR step, in the same process;
  (c) a bytes model counted from shapes beside the times: rows requested by the forward and by
      each backward side, and the sort's traffic.

Method: everything warmed up; timing windows alternate between the contenders, each window timed
with device events around a batch of calls that fills >= ``--window-s``; the median of
``--windows`` windows is reported with their spread (max - min) / median.  Prints one JSON line
and writes it to ``--out`` (default profiles/softmax_loss_bench.json).
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

S, C = 200_000, 128
NEGATIVES = [1, 4, 16, 64]
WINDOW_S, WINDOWS = 0.5, 5


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
    print(f"[softmax_loss_bench] {msg}", file=sys.stderr, flush=True)


def bytes_model(n_rows: int, n_samples: int, M: int, channels: int) -> dict:
    """Requested bytes per pass, from shapes alone (no cache model: the 131 MB table is Infinity-Cache
    resident, so most of the row requests never reach HBM)."""
    K1, row = M + 1, 4 * channels
    R = n_samples * K1
    bits = max(1, int(n_rows).bit_length())
    passes = -(-bits // 10)
    per_record = 4 + 8 + 8          # a pass: the histogram reads the key, the scatter reads and writes the pair
    b = {
        "forward_rows": n_samples * (K1 + 1) * row,          # Z[u_t] and K1 candidate rows
        "forward_ids_coef": n_samples * 8 + R * (8 + 3 * 4),  # u, cand; the score out, in, c out
        "backward_user_rows": R * row,                        # the candidates again (recomputed, not kept)
        "backward_item_rows": R * row,                        # Z[u_t] once per record
        "backward_records": 2 * R * (4 + 4 + 8),              # per side: coef, the sorted pair / id
        "backward_write": n_rows * row,
        "sort": passes * per_record * (R + n_samples),
        "sort_passes": passes,
    }
    b["total"] = sum(v for k, v in b.items() if k != "sort_passes")
    return b


def torch_loss(Z, n_users, u, cand, tau):
    zu = Z.index_select(0, u)
    zc = Z.index_select(0, (n_users + cand).reshape(-1)).view(cand.size(0), cand.size(1), -1)
    s = torch.bmm(zc, zu.unsqueeze(-1)).squeeze(-1) / tau
    return (torch.logsumexp(s, dim=1) - s[:, 0]).mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window-s", type=float, default=WINDOW_S)
    ap.add_argument("--windows", type=int, default=WINDOWS)
    ap.add_argument("--small", action="store_true", help="a 3,000-user graph, S = 20,000 (rehearsal of the tool, not a result)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "softmax_loss_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("softmax_loss_bench: a ROCm GPU is required (nothing here is measured on the host)")
    dev = torch.device("cuda", 0)
    g = (pkg.data.synthetic_ui_graph(n_users=3000, n_items=800, n_interactions=40_000, seed=5) if args.small
         else pkg.data.synthetic_ui_graph(seed=42))
    n_samples = 20_000 if args.small else S
    n = g.n_users + g.n_items
    tr = g.train_pos_idx()
    ei = pkg.data.build_edge_index(g.n_users, g.n_items, tr).to(dev)
    feats = torch.from_numpy(pkg.data.synthetic_item_features(g.n_items, 128)).to(dev)
    ptr, flat = train.user_csr(tr, g.n_users)
    smp = pkg.sampler.BPRSampler(ptr, flat, g.n_items, device=dev)
    u, i, j = smp.sample(n_samples, seed=42)
    cands = {M: smp.eval_candidates(u, i, M, seed=42) for M in NEGATIVES}
    rng = np.random.default_rng(0)
    Z = torch.from_numpy((0.1 * rng.standard_normal((n, C))).astype(np.float32)).to(dev).requires_grad_(True)
    res = {"workload": {"nodes": n, "users": g.n_users, "items": g.n_items, "edges": int(ei.size(1)),
                        "samples": n_samples, "channels": C, "small": bool(args.small)},
           "method": f"median of {args.windows} alternating windows of >= {args.window_s} s, device events; "
                     "spread = (max - min) / median; eager", "loss_alone": [], "step": None}

    # (a) the loss alone
    for M in NEGATIVES:
        cand = cands[M]

        def fused():
            Z.grad = None
            hip_ops.softmax_loss(Z, g.n_users, u, cand, 1.0).backward()

        def eager():
            Z.grad = None
            torch_loss(Z, g.n_users, u, cand, 1.0).backward()

        fused()
        lf, gf = float(hip_ops.softmax_loss(Z, g.n_users, u, cand, 1.0)), Z.grad.clone()
        eager()
        lt, gt = float(torch_loss(Z, g.n_users, u, cand, 1.0)), Z.grad.clone()
        agree = {"loss_rel": abs(lf - lt) / abs(lt), "grad_max_rel": float((gf - gt).abs().max() / gt.abs().max())}
        assert agree["loss_rel"] <= 1e-5 and agree["grad_max_rel"] <= 1e-4, agree
        del gf, gt
        for _ in range(2):
            fused(); eager()
        torch.cuda.synchronize()
        t = alternate({"fused": fused, "torch": eager}, args.window_s, args.windows)
        note(f"M={M} loss fwd+bwd {json.dumps({k: round(v['median_ms'], 4) for k, v in t.items()})}")
        bm = bytes_model(n, n_samples, M, C)
        res["loss_alone"].append({"negatives": M, "agreement": agree, "forward_backward": t,
                                  "torch_over_fused": t["torch"]["median_ms"] / t["fused"]["median_ms"],
                                  "bytes_model": bm,
                                  "requested_GBps_fused": bm["total"] / 1e9 / (t["fused"]["median_ms"] / 1e3)})
        gc.collect()
        torch.cuda.empty_cache()
    hip_ops.check_bpr_indices()

    # (b) the whole step
    torch.manual_seed(42)
    model = pkg.PyGGAT(g.n_users, g.n_items, item_feat_dim=128, hidden=C, layers=2, heads=1, attn_dropout=0.1).to(dev)
    model.train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=1e-4)
    steps = {"bpr": lambda: train.epoch_step(model, opt, feats, ei, g.n_users, u, i, j, "bpr")}
    for M in NEGATIVES:
        steps[f"softmax_M{M}"] = (lambda c: lambda: train.epoch_step(model, opt, feats, ei, g.n_users, u, i, j,
                                                                     softmax=(c, 1.0)))(cands[M])
    for _ in range(3):
        for f in steps.values():
            f()
    torch.cuda.synchronize()
    t = alternate(steps, args.window_s, args.windows)
    note(f"step {json.dumps({k: round(v['median_ms'], 4) for k, v in t.items()})}")
    res["step"] = {"model": "PyGGAT(hidden=128, layers=2, heads=1, attn_dropout=0.1), torch Adam, eager", "times": t,
                   "over_bpr": {k: v["median_ms"] / t["bpr"]["median_ms"] for k, v in t.items()},
                   "extra_ms_over_bpr": {k: v["median_ms"] - t["bpr"]["median_ms"] for k, v in t.items()}}
    res["spread_max"] = max([v["spread"] for v in t.values()] +
                            [v["spread"] for r in res["loss_alone"] for v in r["forward_backward"].values()])
    line = json.dumps(res)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
