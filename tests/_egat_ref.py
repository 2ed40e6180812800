"""Float64 restatement of GATConv with edge features (PyG GATConv with concat=False,
add_self_loops=False, edge_dim=D) for the tests: the forward with PyG's un-collapsed edge term under
autograd, the explicit backward formulas the kernels implement (dv and the two edge parameters'
gradients included), the per-row term scale of dx, the LeakyReLU-kink condition, the 2-layer model
stack, and the recipe's inputs.  CPU torch only; no import of the package.

    h = x W^T [N, H, C]      s_src = <h, att_src>   s_dst = <h, att_dst>            [N, H]
    a_e[k, h] = sum_c lin_edge(edge_attr[k])[h, c] att_edge[h, c]                    [E, H]
    z = s_src[src] + s_dst[dst] + a_e     e = leaky_relu(z)
    alpha = exp(e - max_i) / (sum_in-edges exp(e - max_i) + 1e-16)
    out_i = mean_h sum_k mask_k alpha_k h[src_k] + bias
"""
from __future__ import annotations

import numpy as np
import torch

from _gatv2_ref import N_NODES, make_graph, rel, scaled_rows  # noqa: F401  (the shared graph and figures)

K_IN = 128
SHAPES = [(1, 32), (1, 64), (1, 128), (2, 64), (4, 128)]
EDGE_DIMS = [1, 3]
CASES = [(H, C, D) for (H, C) in SHAPES for D in EDGE_DIMS]
NAMES = ("x", "W", "att_src", "att_dst", "lin_edge", "att_edge", "bias", "G", "edge_attr")


def inputs(n: int, n_edges: int, heads: int, channels: int, edge_dim: int, k_in: int = K_IN, seed: int = 1) -> dict:
    """fp32 numpy inputs of the tests' recipe, drawn in the order of NAMES."""
    rng = np.random.default_rng(seed)
    f = lambda s, *shape: (s * rng.standard_normal(shape)).astype(np.float32)
    H, C, D = heads, channels, edge_dim
    out = {"x": f(0.5, n, k_in), "W": f(k_in ** -0.5, H * C, k_in), "att_src": f(0.2, H, C), "att_dst": f(0.2, H, C),
           "lin_edge": f(0.5, H * C, D), "att_edge": f(0.2, H, C), "bias": f(0.1, C), "G": f(1.0, n, C)}
    out["edge_attr"] = rng.random((n_edges, D)).astype(np.float32)
    return out


def _f64(a):
    return (a.detach() if torch.is_tensor(a) else torch.as_tensor(np.asarray(a))).double().cpu()


def _edges(ei):
    ei = torch.as_tensor(np.asarray(ei.cpu() if torch.is_tensor(ei) else ei)).long()
    return ei[0], ei[1]


def edge_term(lin_edge, att_edge, edge_attr, heads: int):
    """PyG's un-collapsed a_e [E, H] = (lin_edge(edge_attr).view(E, H, C) * att_edge).sum(-1)."""
    E = edge_attr.size(0)
    C = lin_edge.size(0) // heads
    ea = edge_attr.view(E, -1)
    return ((ea @ lin_edge.t()).view(E, heads, C) * att_edge.view(1, heads, C)).sum(-1)


def collapsed_v(lin_edge, att_edge, heads: int):
    """v [H, D] = sum_c att_edge[h, c] lin_edge[h C + c, :]."""
    C = lin_edge.size(0) // heads
    return (lin_edge.view(heads, C, -1) * att_edge.view(heads, C, 1)).sum(1)


def _attention(h3, att_src, att_dst, a_e, src, dst, n, slope):
    H = h3.size(1)
    s_src, s_dst = (h3 * att_src.view(1, H, -1)).sum(-1), (h3 * att_dst.view(1, H, -1)).sum(-1)
    z = s_src[src] + s_dst[dst]
    if a_e is not None:
        z = z + a_e
    e = torch.nn.functional.leaky_relu(z, slope)
    mx = torch.full((n, H), -torch.inf, dtype=e.dtype)
    mx = mx.scatter_reduce(0, dst[:, None].expand(-1, H), e.detach(), "amax", include_self=True)
    ex = torch.exp(e - mx[dst])
    den = torch.zeros(n, H, dtype=e.dtype).index_add_(0, dst, ex) + 1e-16
    return s_src, s_dst, z, ex / den[dst]


def forward(x, W, att_src, att_dst, lin_edge, att_edge, bias, ei, edge_attr, heads: int, slope: float = 0.2,
            mask=None):
    """out [N, C], differentiable in every float64 tensor argument.  ``edge_attr`` None: no edge
    term (PyG skips it).  ``mask`` [E, H]: the dropout multipliers (None: all ones)."""
    src, dst = _edges(ei)
    n, C = x.size(0), W.size(0) // heads
    h3 = (x @ W.t()).view(n, heads, C)
    a_e = None if edge_attr is None else edge_term(lin_edge, att_edge, edge_attr, heads)
    _, _, _, alpha = _attention(h3, att_src, att_dst, a_e, src, dst, n, slope)
    am = alpha if mask is None else alpha * mask
    agg = torch.zeros(n, heads, C, dtype=x.dtype).index_add_(0, dst, am.unsqueeze(-1) * h3[src])
    out = agg.mean(1)
    return out if bias is None else out + bias


GRADS = ("dx", "dW", "datt_src", "datt_dst", "dlin_edge", "datt_edge", "dbias")


def autograd_grads(P: dict, ei, heads: int, slope: float = 0.2, mask=None) -> dict:
    """out and GRADS of sum(out * G) by float64 autograd through the un-collapsed layer."""
    L = {k: _f64(P[k]).requires_grad_(True) for k in ("x", "W", "att_src", "att_dst", "lin_edge", "att_edge", "bias")}
    out = forward(L["x"], L["W"], L["att_src"], L["att_dst"], L["lin_edge"], L["att_edge"], L["bias"], ei,
                  _f64(P["edge_attr"]), heads, slope, None if mask is None else _f64(mask))
    (out * _f64(P["G"])).sum().backward()
    g = lambda k: L[k].grad if L[k].grad is not None else torch.zeros_like(L[k])
    return {"out": out.detach(), "dx": g("x"), "dW": g("W"), "datt_src": g("att_src"), "datt_dst": g("att_dst"),
            "dlin_edge": g("lin_edge"), "datt_edge": g("att_edge"), "dbias": g("bias")}


def formulas(P: dict, ei, heads: int, slope: float = 0.2, mask=None) -> dict:
    """The layer and its backward by the explicit formulas the kernels implement, in float64:
      dalpha = mask <g_i, h_j> / H        D_i = sum_k alpha dalpha      dz = alpha (dalpha - D_i) e'(z)
      ds_src_j = sum_out-edges dz         ds_dst_i = sum_in-edges dz
      dh_j = sum_out-edges mask alpha g_i / H + ds_src_j att_src + ds_dst_j att_dst
      dx = dh W     dW = dh^T x     datt_src[h] = sum_j ds_src[j, h] h[j, h]   (datt_dst likewise)
      dv[h, d] = sum_k dz[k, h] edge_attr[k, d]
      dlin_edge[h C + c, d] = att_edge[h, c] dv[h, d]     datt_edge[h, c] = sum_d lin_edge[h C + c, d] dv[h, d]
    plus scale_x [N]: the 2-norm of the magnitudes of the terms row j of dx sums (before they cancel),
    kink_ratio: min over (edge, head) of |z| / (|s_src| + |s_dst| + |a_e|), and a_e / a_e_collapsed."""
    Q = {k: _f64(v) for k, v in P.items()}
    x, W, G, ea = Q["x"], Q["W"], Q["G"], Q["edge_attr"]
    src, dst = _edges(ei)
    n, H = x.size(0), heads
    C = W.size(0) // H
    a_s, a_d, a_ed = Q["att_src"].view(H, C), Q["att_dst"].view(H, C), Q["att_edge"].view(H, C)
    E = src.numel()
    ea = ea.view(E, -1)
    h3 = (x @ W.t()).view(n, H, C)
    a_e = edge_term(Q["lin_edge"], a_ed, ea, H)
    v = collapsed_v(Q["lin_edge"], a_ed, H)
    s_src, s_dst, z, alpha = _attention(h3, a_s, a_d, a_e, src, dst, n, slope)
    mk = torch.ones(E, H, dtype=torch.float64) if mask is None else _f64(mask)
    hj, gi = h3[src], G[dst].unsqueeze(1)
    agg = torch.zeros(n, H, C, dtype=torch.float64).index_add_(0, dst, (mk * alpha).unsqueeze(-1) * hj)
    out = agg.mean(1) + Q["bias"]
    dalpha = mk * (gi * hj).sum(-1) / H
    Dn = torch.zeros(n, H, dtype=torch.float64).index_add_(0, dst, alpha * dalpha)
    ep = torch.where(z > 0, torch.ones_like(z), torch.full_like(z, slope))
    dz = alpha * (dalpha - Dn[dst]) * ep
    zn = lambda *s: torch.zeros(*s, dtype=torch.float64)
    ds_src, ds_dst = zn(n, H).index_add_(0, src, dz), zn(n, H).index_add_(0, dst, dz)
    msg = (mk * alpha / H).unsqueeze(-1) * gi
    dh = zn(n, H, C).index_add_(0, src, msg) + ds_src.unsqueeze(-1) * a_s + ds_dst.unsqueeze(-1) * a_d
    dhf = dh.reshape(n, H * C)
    dv = dz.t() @ ea
    # magnitudes of what row j of dh sums, pushed through |W|
    dz_mag = alpha * (dalpha.abs() + Dn[dst].abs()) * ep
    mag = zn(n, H, C).index_add_(0, src, msg.abs()) + zn(n, H).index_add_(0, src, dz_mag).unsqueeze(-1) * a_s.abs() \
        + zn(n, H).index_add_(0, dst, dz_mag).unsqueeze(-1) * a_d.abs()
    zmag = s_src[src].abs() + s_dst[dst].abs() + a_e.abs()
    return {
        "out": out, "dx": dhf @ W, "dW": dhf.t() @ x,
        "datt_src": (ds_src.unsqueeze(-1) * h3).sum(0), "datt_dst": (ds_dst.unsqueeze(-1) * h3).sum(0),
        "dv": dv, "dlin_edge": (a_ed.unsqueeze(-1) * dv.unsqueeze(1)).reshape(H * C, -1),
        "datt_edge": (Q["lin_edge"].view(H, C, -1) * dv.unsqueeze(1)).sum(-1), "dbias": G.sum(0),
        "scale_x": (mag.reshape(n, H * C) @ W.abs()).norm(dim=1),
        "kink_ratio": float((z.abs() / zmag.clamp_min(1e-300)).min()) if E else float("inf"),
        "a_e": a_e, "a_e_collapsed": ea @ v.t(), "z_absmax": float(z.abs().max()) if E else 0.0,
    }


def model_forward(sd: dict, item_feats, ei, edge_attr, n_layers: int, heads: int):
    """PyGGAT(edge_dim=D).forward in float64: cat(user_emb, item_proj(feats)) through the conv stack,
    the same ``edge_attr`` feeding every layer.  ``sd``: float64 tensors under the state_dict keys."""
    x = torch.cat([sd["user_emb.weight"], item_feats @ sd["item_proj.weight"].t() + sd["item_proj.bias"]], 0)
    for l in range(n_layers):
        p = f"convs.{l}."
        x = forward(x, sd[p + "lin.weight"], sd[p + "att_src"].view(heads, -1), sd[p + "att_dst"].view(heads, -1),
                    sd[p + "lin_edge.weight"], sd[p + "att_edge"].view(heads, -1), sd[p + "bias"], ei, edge_attr, heads)
    return x
