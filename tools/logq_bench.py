#!/usr/bin/env python3
"""Popularity-weighted negative sampling and the logQ correction on the config-2 stand-in
(data.synthetic_ui_graph(seed=42)): S = 200,000 samples, weights = (train count)^0.75, eager.

  (a) the draws: the weighted candidate draw (``BPRSampler.train_candidates``: a binary search of
      the uint64 CDF per draw) against the uniform one (``eval_candidates``) at M = 16 and M = 64, the
      weighted BPR triples against the uniform ones, and the pool draw (weighted: raw draws + the
      first-occurrence scan in torch ops; uniform: a torch permutation) at P = 1024;
  (b) both losses at d = 128, forward + backward and forward alone, corrected against uncorrected on
      the SAME candidates / pool (M = 16, P = 1024), so the difference is the correction;
  (c) the whole two-layer PyGGAT step (train.epoch_step): BPR, the sampled softmax at M = 16 and the
      shared pool at P = 1024, each uniform-uncorrected and popularity-corrected.

Method: everything warmed up; timing windows alternate between the contenders, each window timed
with device events around a batch of calls that fills >= ``--window-s``; the median of
``--windows`` windows is reported with their spread (max - min) / median.  Prints one JSON line
and writes it to ``--out`` (default profiles/logq_bench.json).
"""
import argparse
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
C = 128
PRIVATE = [16, 64]
POOL = 1024
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
    print(f"[logq_bench] {msg}", file=sys.stderr, flush=True)


def short(t):
    return json.dumps({k: round(v["median_ms"], 4) for k, v in t.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window-s", type=float, default=WINDOW_S)
    ap.add_argument("--windows", type=int, default=WINDOWS)
    ap.add_argument("--small", action="store_true", help="a 3,000-user graph, S = 20,000 (rehearsal of the tool, not a result)")
    ap.add_argument("--no-step", action="store_true", help="skip (c), the whole training step")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "logq_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("logq_bench: a ROCm GPU is required (nothing here is measured on the host)")
    dev = torch.device("cuda", 0)
    g = (pkg.data.synthetic_ui_graph(n_users=3000, n_items=800, n_interactions=40_000, seed=5) if args.small
         else pkg.data.synthetic_ui_graph(seed=42))
    n_samples = 20_000 if args.small else S
    P = min(POOL, g.n_items // 2)
    n = g.n_users + g.n_items
    tr = g.train_pos_idx()
    ei = pkg.data.build_edge_index(g.n_users, g.n_items, tr).to(dev)
    feats = torch.from_numpy(pkg.data.synthetic_item_features(g.n_items, 128)).to(dev)
    ptr, flat = train.user_csr(tr, g.n_users)
    weights = pkg.sampler.BPRSampler.popularity_weights(ptr, flat, g.n_items, 0.75)
    uni = pkg.sampler.BPRSampler(ptr, flat, g.n_items, device=dev)
    pop = pkg.sampler.BPRSampler(ptr, flat, g.n_items, device=dev, item_weights=weights)
    u, i, j = uni.sample(n_samples, seed=42)
    q = pop.w.astype(np.float64) / pop.total
    res = {"workload": {"nodes": n, "users": g.n_users, "items": g.n_items, "edges": int(ei.size(1)),
                        "samples": n_samples, "channels": C, "pool": P, "small": bool(args.small),
                        "items_of_weight_0": int((pop.w == 0).sum()), "largest_q": float(q.max()),
                        "cdf_bytes": int(pop.cdf.numel() * 8),
                        "binary_search_steps": int(np.ceil(np.log2(g.n_items)))},
           "method": f"median of {args.windows} alternating windows of >= {args.window_s} s, device events; "
                     "spread = (max - min) / median; eager"}

    # (a) the draws
    fns = {}
    for M in PRIVATE:
        fns[f"uniform_candidates_M{M}"] = (lambda m: lambda: uni.eval_candidates(u, i, m, seed=1, check=False))(M)
        fns[f"weighted_candidates_M{M}"] = (lambda m: lambda: pop.train_candidates(u, i, m, seed=1, check=False))(M)
    fns["uniform_triples"] = lambda: uni.sample(n_samples, seed=1, check=False)
    fns["weighted_triples"] = lambda: pop.sample(n_samples, seed=1, check=False)
    fns["weighted_raw_draws"] = lambda: pop.weighted_draws(n_samples, seed=1)
    fns[f"uniform_pool_P{P}"] = lambda: uni.sample_pool(P, seed=1)
    fns[f"weighted_pool_P{P}"] = lambda: pop.sample_pool(P, seed=1)
    for _ in range(2):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    t = alternate(fns, args.window_s, args.windows)
    note("draws " + short(t))
    pop.sample_pool(P, seed=1)
    # rejection: how many draws a negative takes on average (history + the positive are refused)
    res["draws"] = {"times": t, "pool_tries": pop.pool_tries,
                    "weighted_over_uniform": {f"M{M}": t[f"weighted_candidates_M{M}"]["median_ms"] /
                                              t[f"uniform_candidates_M{M}"]["median_ms"] for M in PRIVATE},
                    "ns_per_weighted_negative": {f"M{M}": 1e6 * t[f"weighted_candidates_M{M}"]["median_ms"] /
                                                 (n_samples * M) for M in PRIVATE}}

    # (b) the losses alone, corrected against uncorrected on the same inputs
    rng = np.random.default_rng(0)
    Z = torch.from_numpy((0.1 * rng.standard_normal((n, C))).astype(np.float32)).to(dev).requires_grad_(True)
    cand = pop.train_candidates(u, i, 16, seed=42)
    corr = pop.correction(16)
    pool = pop.sample_pool(P, seed=7)
    pcorr = pop.pool_correction()

    def bwd(loss_fn):
        def run():
            Z.grad = None
            loss_fn().backward()
        return run

    def fwd(loss_fn):
        def run():
            with torch.no_grad():
                loss_fn()
        return run

    losses = {"softmax_M16": lambda: hip_ops.softmax_loss(Z, g.n_users, u, cand, 1.0),
              "softmax_M16_logq": lambda: hip_ops.softmax_loss(Z, g.n_users, u, cand, 1.0, correction=corr),
              f"shared_P{P}": lambda: hip_ops.shared_softmax_loss(Z, g.n_users, u, i, pool, 1.0, history=pop),
              f"shared_P{P}_logq": lambda: hip_ops.shared_softmax_loss_corrected(Z, g.n_users, u, i, pool, 1.0,
                                                                                 history=pop, correction=pcorr)}
    fns = {}
    for k, f in losses.items():
        fns[k] = bwd(f)
        fns[k + "_fwd"] = fwd(f)
    for _ in range(2):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    hip_ops.check_bpr_indices()
    t = alternate(fns, args.window_s, args.windows)
    note("losses " + short(t))
    res["losses"] = {"times": t, "values": {k: float(f().detach()) for k, f in losses.items()},
                     "extra_ms": {"softmax_M16": t["softmax_M16_logq"]["median_ms"] - t["softmax_M16"]["median_ms"],
                                  f"shared_P{P}": t[f"shared_P{P}_logq"]["median_ms"] - t[f"shared_P{P}"]["median_ms"]},
                     # what the correction adds to the traffic: one 4-byte gather per negative logit
                     # (private), one P-vector per call read once per streamed tile (shared)
                     "model_bytes": {"softmax_M16_gather": 4 * n_samples * 16, "shared_gather": 4 * P}}
    del Z
    hip_ops.check_bpr_indices()

    # (c) the whole step
    if not args.no_step:
        torch.manual_seed(42)
        model = pkg.PyGGAT(g.n_users, g.n_items, item_feat_dim=128, hidden=128, layers=2, heads=1, attn_dropout=0.1).to(dev)
        model.train()
        opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=1e-4)
        ucand = uni.eval_candidates(u, i, 16, seed=42)
        upool = uni.sample_pool(P, seed=7)
        step = lambda **kw: train.epoch_step(model, opt, feats, ei, g.n_users, u, i, j, "bpr", **kw)  # noqa: E731
        steps = {"bpr": lambda: step(),
                 "softmax_M16_uniform": lambda: step(softmax=(ucand, 1.0)),
                 "softmax_M16_popularity_logq": lambda: step(softmax=(cand, 1.0, corr)),
                 f"shared_P{P}_uniform": lambda: step(shared=(upool, uni, 1.0)),
                 f"shared_P{P}_popularity_logq": lambda: step(shared=(pool, pop, 1.0, pcorr))}
        for _ in range(3):
            for f in steps.values():
                f()
        torch.cuda.synchronize()
        t = alternate(steps, args.window_s, args.windows)
        note("step " + short(t))
        res["step"] = {"model": "PyGGAT(hidden=128, layers=2, heads=1, attn_dropout=0.1), torch Adam, eager", "times": t,
                       "extra_ms_over_bpr": {k: v["median_ms"] - t["bpr"]["median_ms"] for k, v in t.items()}}
        hip_ops.check_bpr_indices()
    line = json.dumps(res)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
