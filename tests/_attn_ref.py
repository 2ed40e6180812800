"""References for the attention-weight tests: the per-edge softmax weights alpha [E, H] of the three
layer families restated in torch on the CPU -- in float64 (the reference) and, by the same code
run in float32, the plain restatement whose own error sets the tests' tolerance -- the
per-destination top-k by np.lexsort, the error metric, and the degree-ladder test graph.  CPU
torch and numpy only; no import of the package.

    v1, PyG mode     e = leaky_relu((s_src[j] + s_dst[i]) [+ edge_term[k]])
                     alpha = exp(e - max_i) / (sum over the in-edges of i of exp(e - max_i) + 1e-16)
    v1, custom mode  alpha = exp(clamp(leaky_relu(z), -10, 10)) / (sum over the in-edges + 1e-9)
    GATv2            e = att_h . leaky_relu(x_l[j] + x_r[i]), then as PyG mode (_gatv2_ref._alpha)
"""
from __future__ import annotations

import numpy as np
import torch

from _gatv2_ref import _alpha as _gatv2_alpha

MODE_PYG, MODE_CUSTOM = 0, 1
N_NODES = 400
# node d of the ladder has in-degree LADDER[d]; every other node has none
LADDER = (0, 1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 600)
FLOOR = 2.0 ** -24


def ladder_graph(seed: int = 0) -> np.ndarray:
    """edge_index int64 [2, E] (row 0 sources, row 1 destinations) of the degree ladder, columns
    shuffled: destination d < 16 receives exactly LADDER[d] edges from sources drawn with
    replacement among all N_NODES nodes (so the longer rows repeat edges), the first edge of every
    row with at least two being the self-loop d -> d and the second a copy of the third (a
    guaranteed duplicate from 3 edges on)."""
    rng = np.random.default_rng(seed)
    src, dst = [], []
    for d, deg in enumerate(LADDER):
        s = rng.integers(0, N_NODES, deg)
        if deg >= 2:
            s[0] = d
        if deg >= 3:
            s[1] = s[2]
        src.append(s)
        dst.append(np.full(deg, d, np.int64))
    ei = np.stack([np.concatenate(src), np.concatenate(dst)]).astype(np.int64)
    return np.ascontiguousarray(ei[:, rng.permutation(ei.shape[1])])


def _t(a, dtype):
    return (a.detach().cpu() if torch.is_tensor(a) else torch.as_tensor(np.asarray(a))).to(dtype)


def _edges(ei):
    ei = torch.as_tensor(np.asarray(ei.cpu() if torch.is_tensor(ei) else ei)).long()
    return ei[0], ei[1]


def v1_alpha(s_src, s_dst, ei, mode: int, slope: float = 0.2, edge_term=None, dtype=torch.float64):
    """alpha [E, H] in edge_index column order from the node scores [N, H] (and ``edge_term`` [E, H]
    in the same column order), every operation in ``dtype``."""
    src, dst = _edges(ei)
    ss, sd = _t(s_src, dtype), _t(s_dst, dtype)
    n, H = sd.shape
    z = ss[src] + sd[dst]
    if edge_term is not None:
        z = z + _t(edge_term, dtype)
    e = torch.nn.functional.leaky_relu(z, slope)
    if mode == MODE_CUSTOM:
        ex = torch.exp(e.clamp(-10.0, 10.0))
        den = torch.zeros(n, H, dtype=dtype).index_add_(0, dst, ex) + 1e-9
        return ex / den[dst]
    mx = torch.full((n, H), -torch.inf, dtype=dtype)
    mx = mx.scatter_reduce(0, dst[:, None].expand(-1, H), e, "amax", include_self=True)
    ex = torch.exp(e - mx[dst])
    den = torch.zeros(n, H, dtype=dtype).index_add_(0, dst, ex) + 1e-16
    return ex / den[dst]


def v2_alpha(xl, xr, att, ei, heads: int, slope: float = 0.2, dtype=torch.float64):
    """alpha [E, H] of the GATv2 layer from its projections [N, H * C] and att [H, C], in ``dtype``."""
    src, dst = _edges(ei)
    xl, xr, att = _t(xl, dtype), _t(xr, dtype), _t(att, dtype).view(heads, -1)
    n, C = xl.size(0), att.size(1)
    return _gatv2_alpha(xl.view(n, heads, C), xr.view(n, heads, C), att, src, dst, n, slope)[2]


def gat_layer_alpha(x, W, att_src, att_dst, ei, heads: int, mode: int, slope: float = 0.2, edge_term=None,
                    dtype=torch.float64):
    """alpha [E, H] of a whole v1 layer: h = x W^T, the node scores, v1_alpha.  Returns (alpha, h)."""
    x, W = _t(x, dtype), _t(W, dtype)
    h3 = (x @ W.t()).view(x.size(0), heads, -1)
    s_src = (h3 * _t(att_src, dtype).view(1, heads, -1)).sum(-1)
    s_dst = (h3 * _t(att_dst, dtype).view(1, heads, -1)).sum(-1)
    return v1_alpha(s_src, s_dst, ei, mode, slope, edge_term, dtype), h3


def aggregate(alpha, h3, ei, bias=None):
    """out [N, C] = mean_h sum_k alpha_k h[src_k] (+ bias), in alpha's dtype."""
    src, dst = _edges(ei)
    agg = torch.zeros_like(h3).index_add_(0, dst, alpha.unsqueeze(-1) * h3[src])
    out = agg.mean(1)
    return out if bias is None else out + _t(bias, out.dtype)


def model_alphas(sd: dict, item_feats, ei, n_layers: int, heads: int, family: str, slope: float = 0.2,
                 dtype=torch.float64):
    """The per-layer alpha [E, H] of PyGGAT ("gat_pyg"), CustomGAT ("gat_custom") or PyGGATv2
    ("gatv2_pyg") in eval mode, every operation in ``dtype``: ``sd`` the model's state_dict."""
    P = {k: _t(v, dtype) for k, v in sd.items()}
    x = torch.cat([P["user_emb.weight"], _t(item_feats, dtype) @ P["item_proj.weight"].t() + P["item_proj.bias"]], 0)
    out = []
    for l in range(n_layers):
        if family == "gatv2_pyg":
            p = f"convs.{l}."
            xl = x @ P[p + "lin_l.weight"].t() + P[p + "lin_l.bias"]
            xr = x @ P[p + "lin_r.weight"].t() + P[p + "lin_r.bias"]
            alpha = v2_alpha(xl, xr, P[p + "att"], ei, heads, slope, dtype)
            x = aggregate(alpha, xl.view(x.size(0), heads, -1), ei, P[p + "bias"])
        elif family == "gat_pyg":
            p = f"convs.{l}."
            alpha, h3 = gat_layer_alpha(x, P[p + "lin.weight"], P[p + "att_src"], P[p + "att_dst"], ei, heads, MODE_PYG,
                                        slope, None, dtype)
            x = aggregate(alpha, h3, ei, P[p + "bias"])
        else:
            p = f"layers.{l}."
            alpha, h3 = gat_layer_alpha(x, P[p + "lin.weight"], P[p + "a_src"], P[p + "a_dst"], ei, 1, MODE_CUSTOM,
                                        slope, None, dtype)
            x = aggregate(alpha, h3, ei)
        out.append(alpha)
    return out


def brute_alpha(logit_fn, ei, n: int, heads: int, eps: float, subtract_max: bool) -> np.ndarray:
    """alpha [E, H] by a Python loop over the destinations in float64: ``logit_fn(k, h)`` is the
    logit of edge column k and head h (already clamped in custom mode)."""
    src, dst = (np.asarray(a) for a in _edges(ei))
    out = np.zeros((len(dst), heads))
    for i in range(n):
        ks = np.flatnonzero(dst == i)
        for h in range(heads):
            e = np.array([logit_fn(int(k), h) for k in ks], np.float64)
            if e.size == 0:
                continue
            ex = np.exp(e - (e.max() if subtract_max else 0.0))
            out[ks, h] = ex / (ex.sum() + eps)
    return out


def dest_max(alpha64, ei, n: int):
    """[N, H]: the largest float64 weight of every destination (0 without in-edges)."""
    _, dst = _edges(ei)
    a = _t(alpha64, torch.float64)
    mx = torch.zeros(n, a.size(1), dtype=torch.float64)
    return mx.scatter_reduce(0, dst[:, None].expand(-1, a.size(1)), a, "amax", include_self=True)


def metric(alpha, alpha64, ei, n: int) -> float:
    """max over (edge, head) of |alpha - alpha64| / (the largest float64 weight of the edge's
    destination); both in edge_index column order."""
    _, dst = _edges(ei)
    a, r = _t(alpha, torch.float64), _t(alpha64, torch.float64)
    if r.numel() == 0:
        return 0.0
    return float(((a - r).abs() / dest_max(r, ei, n)[dst]).max())


def bound(restatement_metric: float) -> float:
    """The tests' tolerance: four times the float32 restatement's own figure, floored at 2^-24."""
    return max(4.0 * restatement_metric, FLOOR)


def topk_ref(val, ei, n: int, k: int):
    """(eid [N, k] int32, value [N, k] float32, count [N] int32): per destination the k in-edges with
    the largest head mean of ``val`` [E, H] (edge_index column order), by np.lexsort((eid, -value)):
    value descending, edge id ascending; -1 / 0 past the in-degree.  The head mean is formed as the
    kernel forms it, (sum over the heads in order) * float32(1 / H), in float32."""
    _, dst = (np.asarray(a) for a in _edges(ei))
    v = np.asarray(val, np.float32)
    H = v.shape[1]
    mean = v[:, 0].copy()
    for h in range(1, H):
        mean = (mean + v[:, h]).astype(np.float32)
    mean = (mean * np.float32(1.0 / H)).astype(np.float32)
    eid = np.full((n, k), -1, np.int32)
    out = np.zeros((n, k), np.float32)
    cnt = np.zeros(n, np.int32)
    for i in range(n):
        ks = np.flatnonzero(dst == i)
        order = ks[np.lexsort((ks, -mean[ks].astype(np.float64)))][:k]
        eid[i, :len(order)] = order
        out[i, :len(order)] = mean[order]
        cnt[i] = len(order)
    return eid, out, cnt
