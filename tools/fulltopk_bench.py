#!/usr/bin/env python3
"""Full-catalogue top-K at config-2 size: for every one of the 192,403 users of the config-2
stand-in (data.synthetic_ui_graph(seed=42): its train histories) the k best of the 63,001 items
outside the user's history, d in {64, 128}, k in {20, 100} -- the fused kernel
(evaluation.recommend_topk -> ppgat_full_topk) against two comparators in the same session:

(a) ``torch``: the same lists in torch ops: chunked fp32 ``U[chunk] @ I.T``, the history set to
    -inf by index, ``torch.topk(k)``;
(b) ``full_rank``: ppgat_full_rank on the same users (one random positive each).  It forms the
    identical product with a compare-and-count epilogue, so it is the floor: the time over (b)
    is what the selection costs.

Method (tools/fullrank_bench.py's): every path warmed up; timing windows of >= 0.5 s alternate
between the three paths, the median of >= 5 windows is reported with the windows' spread.
Everything is device-resident: ids, CSR, workspace, outputs and the baseline's per-chunk mask
indices are made before any window.  Before timing, the kernel's lists must agree with (a):
wherever two lists differ, BOTH must lie inside the fp64 band of
tau(i, j) = (d + 8) 2^-24 (|u|^T|i| + |u|^T|j|) (fp64 on the device for the differing rows): no
history item, neighbours in order to within tau, and no left-out item better than the last by
more than tau -- i.e. the difference is a near-tie that fp32 cannot decide (or an exact fp32 tie,
which torch.topk may order either way).

Prints one JSON line per run.  ``--profile-run``: a few calls of each path and nothing else, for
``rocprofv3 --kernel-trace --stats -- python tools/fulltopk_bench.py --profile-run`` (and, in a
run of its own, ``--pmc`` with ``--kernel-only``).
"""
import argparse
import ctypes
import importlib
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
pkg = importlib.import_module("plotpointe-gat-recommendation_amd")
from lightgcn_bench import alternate  # noqa: E402  (the windowed timer)

WIDTHS = (64, 128)
KS = (20, 100)
CHUNK = 8192  # baseline: users per score block (8192 x 63001 fp32 = 2.1 GB)


def note(msg):
    print(f"[fulltopk_bench] {msg}", file=sys.stderr, flush=True)


class TopK:
    """ppgat_full_topk with everything device-resident (evaluation.recommend_topk minus the
    per-call allocations)."""

    def __init__(self, U, I, users, smp, k):
        self.lib = pkg._lib.load()
        self.U, self.I, self.users, self.smp, self.k = U, I, users, smp, k
        n = users.numel()
        self.idx = torch.empty(n, k, dtype=torch.int32, device=U.device)
        self.sc = torch.empty(n, k, dtype=torch.float32, device=U.device)
        nbytes = ctypes.c_size_t(0)
        pkg._lib.check(self.lib.ppgat_full_topk_workspace_bytes(n, I.size(0), U.size(1), k, ctypes.byref(nbytes)), "ws")
        self.nbytes = int(nbytes.value)
        self.ws = torch.empty(self.nbytes, dtype=torch.uint8, device=U.device)
        self.stream = pkg._lib.stream_handle(U.device)

    def __call__(self):
        U, I = self.U, self.I
        pkg._lib.check(self.lib.ppgat_full_topk(U.data_ptr(), U.stride(0), U.size(0), I.data_ptr(), I.stride(0), I.size(0),
                                                U.size(1), self.users.data_ptr(), self.users.numel(),
                                                self.smp.ptr.data_ptr(), self.smp.items.data_ptr(), self.k,
                                                self.idx.data_ptr(), self.sc.data_ptr(), self.ws.data_ptr(), self.nbytes,
                                                self.stream), "full_topk")
        return self.idx


class FullRank:
    """ppgat_full_rank on the same users: the identical product, a count for an epilogue."""

    def __init__(self, U, I, users, pos, smp):
        self.lib = pkg._lib.load()
        self.U, self.I, self.users, self.pos, self.smp = U, I, users, pos, smp
        self.rank = torch.empty(users.numel(), dtype=torch.int32, device=U.device)
        self.ties = torch.empty_like(self.rank)
        self.stream = pkg._lib.stream_handle(U.device)

    def __call__(self):
        U, I = self.U, self.I
        pkg._lib.check(self.lib.ppgat_full_rank(U.data_ptr(), U.stride(0), U.size(0), I.data_ptr(), I.stride(0),
                                                I.size(0), U.size(1), self.users.data_ptr(), self.pos.data_ptr(),
                                                self.users.numel(), self.smp.ptr.data_ptr(), self.smp.items.data_ptr(),
                                                self.rank.data_ptr(), self.ties.data_ptr(), None, 0, self.stream),
                       "full_rank")
        return self.rank


def history_coords(smp, u, dev):
    """(rows, cols) of the history entries of the users ``u`` (row = position in u)."""
    lens = smp.ptr[u + 1] - smp.ptr[u]
    rows = torch.repeat_interleave(torch.arange(u.numel(), device=dev), lens)
    start = torch.repeat_interleave(smp.ptr[u] - (torch.cumsum(lens, 0) - lens), lens)
    cols = smp.items[torch.arange(rows.numel(), device=dev) + start].long()
    return rows, cols


class TorchBaseline:
    """The same lists in torch ops: per chunk of users one fp32 score block, the history set to
    -inf BY INDEX, torch.topk."""

    def __init__(self, U, I, users, smp, k):
        self.U, self.It, self.users, self.k = U, I.t().contiguous(), users, k
        n = users.numel()
        self.idx = torch.empty(n, k, dtype=torch.int64, device=U.device)
        self.sc = torch.empty(n, k, dtype=torch.float32, device=U.device)
        self.chunks = []
        for a in range(0, n, CHUNK):
            b = min(a + CHUNK, n)
            self.chunks.append((a, b) + history_coords(smp, users[a:b], U.device))

    def __call__(self):
        for a, b, rows, cols in self.chunks:
            S = self.U[self.users[a:b]] @ self.It
            S[rows, cols] = float("-inf")
            torch.topk(S, self.k, dim=1, out=(self.sc[a:b], self.idx[a:b]))
        return self.idx


def band_check(U, I, users, smp, rows, lists, d):
    """Each list of ``lists`` ([n, k] item ids), on the rows ``rows``, inside the fp64 band."""
    scale = (d + 8) * 2.0 ** -24
    U64, I64t = U.double(), I.double().t().contiguous()
    A64, B64t = U64.abs(), I64t.abs()
    dev = U.device
    for a in range(0, rows.numel(), 256):
        e = rows[a:a + 256]
        u = users[e]
        S, A = U64[u] @ I64t, A64[u] @ B64t
        elig = torch.ones_like(S, dtype=torch.bool)
        hr, hc = history_coords(smp, u, dev)
        elig[hr, hc] = False
        ar = torch.arange(e.numel(), device=dev).unsqueeze(1)
        for L in lists:
            L = L[e].long()
            if int((L < 0).sum()) or not bool(elig[ar, L].all()):
                raise RuntimeError(f"fulltopk_bench: a list holds a pad or a history item (d = {d})")
            s, t = S[ar, L], A[ar, L]
            if not bool((s[:, :-1] >= s[:, 1:] - scale * (t[:, :-1] + t[:, 1:])).all()):
                raise RuntimeError(f"fulltopk_bench: a list is out of order beyond the fp64 band (d = {d})")
            left = elig.clone()
            left[ar, L] = False
            tau = scale * (A + t[:, -1:])
            if bool((left & (S > s[:, -1:] + tau)).any()):
                raise RuntimeError(f"fulltopk_bench: a left-out item beats a list's last beyond the fp64 band (d = {d})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--profile-run", action="store_true")
    ap.add_argument("--kernel-only", action="store_true", help="with --profile-run: skip the torch baseline (PMC passes)")
    ap.add_argument("--window-s", type=float, default=0.5)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="a 3,000-user graph (rehearsal of the tool, not a result)")
    ap.add_argument("--out", default=None, help="also write the JSON record to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("fulltopk_bench: a ROCm GPU is required (nothing here is measured on the host)")
    dev = torch.device("cuda", 0)
    g = (pkg.data.synthetic_ui_graph(n_users=3000, n_items=800, n_interactions=40_000, seed=5) if args.small
         else pkg.data.synthetic_ui_graph(seed=42))
    smp = pkg.sampler.BPRSampler(g.user_ptr, g.user_items, g.n_items, device=dev)
    rng = np.random.default_rng(42)
    users = torch.arange(g.n_users, device=dev)
    pos = torch.from_numpy(rng.integers(0, g.n_items, g.n_users)).to(dev)
    out = {"workload": {"users": g.n_users, "items": g.n_items, "history_entries": int(g.user_ptr[-1]),
                        "small": bool(args.small)},
           "method": f"median of {args.windows} alternating windows of >= {args.window_s} s; "
                     "spread = (max - min) / median", "cases": {}}
    for d in WIDTHS:
        gen = torch.Generator(device="cpu").manual_seed(d)
        U = (torch.randn(g.n_users, d, generator=gen) * 0.1).to(dev)
        I = (torch.randn(g.n_items, d, generator=gen) * 0.1).to(dev)
        floor = FullRank(U, I, users, pos, smp)
        for k in KS:
            new, base = TopK(U, I, users, smp, k), TorchBaseline(U, I, users, smp, k)
            if args.profile_run:
                for _ in range(5):
                    new()
                    floor()
                for _ in range(0 if args.kernel_only else 2):
                    base()
                torch.cuda.synchronize()
                continue
            ln, lb = new().clone(), base().clone()
            differ = torch.nonzero((ln.long() != lb).any(1)).flatten()
            if differ.numel():
                band_check(U, I, users, smp, differ[:20000], (ln, lb), d)
            note(f"d={d} k={k}: {differ.numel()} of {ln.size(0)} lists differ between the paths, all inside the fp64 band")
            for _ in range(3):
                new(); base(); floor()
            t = alternate({"kernel": new, "torch": base, "full_rank": floor}, args.window_s, args.windows)
            ms, bms, fms = t["kernel"]["median_ms"], t["torch"]["median_ms"], t["full_rank"]["median_ms"]
            spread = max(v["spread"] for v in t.values())
            out["cases"][f"d{d}_k{k}"] = {
                "d": d, "k": k, "kernel_ms": ms, "torch_ms": bms, "full_rank_ms": fms,
                "ratio_torch_over_kernel": bms / ms, "ratio_kernel_over_full_rank": ms / fms,
                "selection_overhead_ms": ms - fms, "spread_between_windows": spread,
                "overhead_exceeds_spread": bool(ms / fms - 1.0 > spread), "users_per_s": g.n_users / (ms * 1e-3),
                "workspace_MB": new.nbytes / 2 ** 20, "lists_differing_between_paths": int(differ.numel()),
                "timing": t}
            del new, base
            torch.cuda.empty_cache()
        del floor, U, I
        torch.cuda.empty_cache()
    if args.profile_run:
        out = {"profile_run": True, "kernel_calls_each": 5, "baseline_calls_each": 0 if args.kernel_only else 2,
               "widths": list(WIDTHS), "ks": list(KS)}
    line = json.dumps(out)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
