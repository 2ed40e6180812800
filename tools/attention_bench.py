#!/usr/bin/env python3
"""Attention weights on the config-2 stand-in (data.synthetic_ui_graph(seed=42): 255,404 nodes,
2,608,620 edges), 128 input features:
  weights   one GATConv layer's alpha [E, H] by ppgat_attention in both orders ("slot": CSR slot
            order, "edge": edge_index column order -- a scatter of 4 H bytes per edge) against the
            same weights in fp32 torch ops on the same GPU (gathers, scatter_reduce(amax),
            index_add_), from the same node scores;
  gatv2     likewise ppgat_dynatt_attention against torch ops, from the same projections;
  topk      hip_ops.attention_topk at k = 10 against a torch sort-based selection (one stable
            sort by value, one by destination, the first k of every segment);
  flagged   a forward with return_attention_weights=True against one without.

Method: everything warmed up; timing windows of >= 0.5 s alternate between the paths, the median
of 5 windows is reported with the windows' spread (max - min) / median.  Before any timing the
kernel and the torch restatement must agree (max |alpha - alpha_torch| over the destination's
largest weight <= 1e-5) and the two selections must pick the same edges.  Bytes are counted from
shapes (``weight_bytes``).  Prints one JSON line.
"""
import argparse
import importlib
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
pkg = importlib.import_module("plotpointe-gat-recommendation_amd")
hip_ops = importlib.import_module(pkg.__name__ + ".hip_ops")
_launch = importlib.import_module(pkg.__name__ + "._launch")

F_IN, SLOPE, K = 128, 0.2, 10
WINDOW_S, WINDOWS = 0.5, 5


def weight_bytes(n: int, e: int, H: int, C: int = 0):
    """Requested bytes of one weights pass, from shapes: per edge the source index, the source's
    scores (v1: 4 H; GATv2: its x_l row, 4 H C) and the 4 H bytes written (order "edge": plus the
    edge id); per node the destination's scores (GATv2: its x_r row) and state once."""
    per_edge = 4 + (4 * H * C if C else 4 * H) + 4 * H
    per_node = (4 * H * C if C else 4 * H) + 8 * H
    return {"slot": e * per_edge + n * per_node, "edge": e * (per_edge + 4) + n * per_node}


def torch_v1(ss, sd, src, dst, n, H):
    e = torch.nn.functional.leaky_relu(ss.index_select(0, src) + sd.index_select(0, dst), SLOPE)
    return _softmax(e, dst, n, H)


def torch_v2(xl, xr, att, src, dst, n, H, C):
    t = xl.view(n, H, C).index_select(0, src) + xr.view(n, H, C).index_select(0, dst)
    return _softmax((torch.nn.functional.leaky_relu(t, SLOPE) * att.view(1, H, C)).sum(-1), dst, n, H)


def _softmax(e, dst, n, H):
    idx = dst[:, None].expand(-1, H)
    mx = torch.full((n, H), -torch.inf, device=e.device).scatter_reduce(0, idx, e, "amax", include_self=True)
    ex = torch.exp(e - mx.index_select(0, dst))
    den = torch.zeros(n, H, device=e.device).index_add_(0, dst, ex) + 1e-16
    return ex / den.index_select(0, dst)


def torch_topk(alpha_edge, dst, rowptr, n, k):
    """[N, k] edge ids (-1 pads): value descending, edge id ascending within a destination."""
    v = alpha_edge.mean(1) if alpha_edge.size(1) > 1 else alpha_edge[:, 0]
    o1 = torch.sort(v, descending=True, stable=True).indices          # ties keep ascending edge id
    o2 = torch.sort(dst[o1], stable=True).indices
    order = o1[o2]                                                    # by destination, then value desc, id asc
    start = rowptr[:-1].long()
    deg = rowptr[1:].long() - start
    pos = start[:, None] + torch.arange(k, device=v.device)[None, :]
    ok = torch.arange(k, device=v.device)[None, :] < deg[:, None]
    return torch.where(ok, order[pos.clamp_max(max(order.numel() - 1, 0))], torch.full_like(pos, -1))


def agree(a, b, dst, n):
    H = a.size(1)
    mx = torch.zeros(n, H, device=a.device, dtype=torch.float64).scatter_reduce(
        0, dst[:, None].expand(-1, H), b.double(), "amax", include_self=True)
    return float(((a.double() - b.double()).abs() / mx.index_select(0, dst)).max())


def window(fn, seconds: float) -> float:
    torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    while True:
        for _ in range(4):
            fn()
        n += 4
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if dt >= seconds:
            return dt / n


def alternate(fns: dict, seconds: float, windows: int):
    for fn in fns.values():
        for _ in range(3):
            fn()
    got = {k: [] for k in fns}
    for _ in range(windows):
        for k, fn in fns.items():
            got[k].append(window(fn, seconds))
    out = {}
    for k, v in got.items():
        med = statistics.median(v)
        out[k] = {"median_ms": 1e3 * med, "spread": (max(v) - min(v)) / med}
    return out


def note(msg):
    print(f"[attention_bench] {msg}", file=sys.stderr, flush=True)


def with_rates(t: dict, nbytes: dict):
    for order in ("slot", "edge"):
        t[order]["requested_TBps"] = nbytes[order] / (t[order]["median_ms"] / 1e3) / 1e12
    t["edge_over_slot"] = t["edge"]["median_ms"] / t["slot"]["median_ms"]
    t["torch_over_edge"] = t["torch_ops"]["median_ms"] / t["edge"]["median_ms"]
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window-s", type=float, default=WINDOW_S)
    ap.add_argument("--windows", type=int, default=WINDOWS)
    ap.add_argument("--small", action="store_true", help="a 3,000-user graph (rehearsal of the tool, not a result)")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("attention_bench: a ROCm GPU is required (nothing here is measured on the host)")
    dev = torch.device("cuda", 0)
    g = (pkg.data.synthetic_ui_graph(n_users=3000, n_items=800, n_interactions=40_000, seed=5) if args.small
         else pkg.data.synthetic_ui_graph(seed=42))
    n = g.n_users + g.n_items
    ei = pkg.data.build_edge_index(g.n_users, g.n_items, g.train_pos_idx()).to(dev)
    E = int(ei.size(1))
    src, dst = ei[0].contiguous(), ei[1].contiguous()
    graph = hip_ops.graph_cache.get(ei, n)
    rng = np.random.default_rng(0)
    x = torch.from_numpy((0.5 * rng.standard_normal((n, F_IN))).astype(np.float32)).to(dev)
    res = {"workload": {"nodes": n, "edges": E, "in_features": F_IN, "small": bool(args.small)},
           "method": f"median of {args.windows} alternating windows of >= {args.window_s} s; spread = (max - min) / "
                     "median; eager", "weights": [], "gatv2": [], "topk": [], "flagged_forward": []}
    run = lambda fns: alternate(fns, args.window_s, args.windows)

    for H, C in ((1, 128), (2, 128)):
        torch.manual_seed(42)
        conv = pkg.GATConv(F_IN, C, heads=H, concat=False, add_self_loops=False).to(dev).eval()
        with torch.no_grad():
            h = hip_ops.mm_nn(x, conv.lin.weight.detach().contiguous(), 1, H * C)
            ss, sd = hip_ops.node_scores(h, conv.att_src.detach().view(H, C).contiguous(),
                                         conv.att_dst.detach().view(H, C).contiguous(), H, C)
            _, m, inv_l, _ = hip_ops.gat_fwd(graph, h, ss, sd, None, H, C, 0, SLOPE, 0.0, 0, want_agg=False)
            a_edge = hip_ops.attention_weights(graph, ss, sd, m, inv_l, H, 0, SLOPE)
            a_slot = hip_ops.attention_weights(graph, ss, sd, m, inv_l, H, 0, SLOPE, order="slot")
            fig = agree(a_edge, torch_v1(ss, sd, src, dst, n, H), dst, n)
            note(f"v1 H={H}: kernel vs torch ops {fig:.3e}")
            if fig > 1e-5 or not torch.equal(a_edge[graph.csr_eid.long()], a_slot):
                raise RuntimeError(f"attention_bench: ppgat_attention and the torch restatement disagree ({fig})")
            out = torch.empty(E, H, device=dev)
            t = run({"slot": lambda: _launch.attention(graph, ss, sd, m, inv_l, H, 0, SLOPE, 0, out),
                     "edge": lambda: _launch.attention(graph, ss, sd, m, inv_l, H, 0, SLOPE, 1, out),
                     "torch_ops": lambda: torch_v1(ss, sd, src, dst, n, H)})
            res["weights"].append({"heads": H, "agreement": fig, "bytes": weight_bytes(n, E, H),
                                   **with_rates(t, weight_bytes(n, E, H))})
            note(f"v1 H={H}: {json.dumps({k: round(v['median_ms'], 4) for k, v in t.items() if isinstance(v, dict)})}")

            # the selection, on this layer's weights
            eid, val, cnt = hip_ops.attention_topk(graph, a_slot, K)
            ref = torch_topk(a_edge, dst, graph.rowptr, n, K)
            same = bool(torch.equal(eid.long(), ref))
            note(f"topk H={H}: kernel and sort-based selection pick the same edges: {same}")
            if not same:
                raise RuntimeError("attention_bench: attention_topk and the sort-based selection disagree")
            tk = run({"attention_topk": lambda: hip_ops.attention_topk(graph, a_slot, K),
                      "torch_sort": lambda: torch_topk(a_edge, dst, graph.rowptr, n, K)})
            tk["torch_over_kernel"] = tk["torch_sort"]["median_ms"] / tk["attention_topk"]["median_ms"]
            res["topk"].append({"heads": H, "k": K, "max_in_degree": int(graph.in_degree().max()), **tk})

            ff = run({"plain": lambda: conv(x, ei), "flagged": lambda: conv(x, ei, return_attention_weights=True)})
            ff["flagged_over_plain"] = ff["flagged"]["median_ms"] / ff["plain"]["median_ms"]
            res["flagged_forward"].append({"layer": "GATConv", "heads": H, "channels": C, **ff})
        del conv, h, a_edge, a_slot, out
        torch.cuda.empty_cache()

    for H, C in ((1, 128), (2, 128)):
        torch.manual_seed(42)
        conv = pkg.GATv2Conv(F_IN, C, heads=H, concat=False, add_self_loops=False).to(dev).eval()
        with torch.no_grad():
            xl = hip_ops.linear(x, conv.lin_l.weight, conv.lin_l.bias)
            xr = hip_ops.linear(x, conv.lin_r.weight, conv.lin_r.bias)
            att = conv.att.detach().view(H, C).contiguous()
            o, m, inv_l = torch.empty(n, C, device=dev), torch.empty(n, H, device=dev), torch.empty(n, H, device=dev)
            _launch.dynatt_fwd(graph, xl, xr, att, None, H, C, SLOPE, 0.0, 0, None, o, m, inv_l)
            a_edge = hip_ops.gatv2_attention_weights(graph, xl, xr, att, m, inv_l, H, C, SLOPE)
            fig = agree(a_edge, torch_v2(xl, xr, att, src, dst, n, H, C), dst, n)
            note(f"gatv2 H={H}: kernel vs torch ops {fig:.3e}")
            if fig > 1e-5:
                raise RuntimeError(f"attention_bench: ppgat_dynatt_attention and the torch restatement disagree ({fig})")
            out = torch.empty(E, H, device=dev)
            t = run({"slot": lambda: _launch.dynatt_attention(graph, xl, xr, att, m, inv_l, H, C, SLOPE, 0, out),
                     "edge": lambda: _launch.dynatt_attention(graph, xl, xr, att, m, inv_l, H, C, SLOPE, 1, out),
                     "torch_ops": lambda: torch_v2(xl, xr, att, src, dst, n, H, C)})
            res["gatv2"].append({"heads": H, "channels": C, "agreement": fig, "bytes": weight_bytes(n, E, H, C),
                                 **with_rates(t, weight_bytes(n, E, H, C))})
            note(f"gatv2 H={H}: {json.dumps({k: round(v['median_ms'], 4) for k, v in t.items() if isinstance(v, dict)})}")
            ff = run({"plain": lambda: conv(x, ei), "flagged": lambda: conv(x, ei, return_attention_weights=True)})
            ff["flagged_over_plain"] = ff["flagged"]["median_ms"] / ff["plain"]["median_ms"]
            res["flagged_forward"].append({"layer": "GATv2Conv", "heads": H, "channels": C, **ff})
        del conv, xl, xr, a_edge, out
        torch.cuda.empty_cache()

    line = json.dumps(res)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
