"""Float64 restatement of the GATv2 layer (PyG GATv2Conv with concat=False, add_self_loops=False,
edge_dim=None, residual=False) for the tests: the forward with autograd, the explicit backward
formulas the kernels implement, the per-row term scales the row-wise gradient bounds use, and the
test graph.  CPU torch only; no import of the package.

    t_ij  = x_l[j] + x_r[i]                         e_ij = sum_c att[h,c] leaky_relu(t_ij[c])
    alpha = exp(e - max_i) / (sum_in-edges exp(e - max_i) + 1e-16)
    out_i = mean_h sum_j mask_ij alpha_ij x_l[j] + bias
"""
from __future__ import annotations

import numpy as np
import torch

N_NODES = 900
SHAPES = [(1, 32), (1, 64), (1, 128), (2, 64), (2, 128), (4, 64), (4, 128)]
IN_DEGREES = {0: 700, 2: 256, 3: 257, 4: 16, 5: 17, 6: 1, 7: 3, 8: 1, 9: 0}


def make_graph(seed: int = 0) -> np.ndarray:
    """edge_index int64 [2, E] of the GATv2 test graph, columns shuffled:
    node 0 receives 700 edges (a three-piece destination hub at max_edges 256), node 1 emits 700
    (source hub), nodes 2..6 have in-degree exactly 256, 257, 16, 17, 1 (piece boundary,
    short/long boundary, single-in-edge softmax), 11 -> 7 three times, the self-loop 8 -> 8, a
    skewed background among nodes 0..879 whose destinations are all >= 10, and nodes 880..899
    without any edge."""
    rng = np.random.default_rng(seed)
    src = np.floor(880 * rng.random(9000) ** 2).astype(np.int64)
    dst = np.floor(880 * rng.random(9000) ** 6).astype(np.int64)
    keep = dst >= 10
    parts = [(src[keep], dst[keep])]
    parts.append((rng.integers(0, 880, 700), np.zeros(700, np.int64)))                    # into node 0
    parts.append((np.ones(700, np.int64), 10 + rng.permutation(870)[:700]))              # out of node 1
    for node, deg in ((2, 256), (3, 257), (4, 16), (5, 17), (6, 1)):
        parts.append((rng.integers(10, 880, deg), np.full(deg, node, np.int64)))
    parts.append((np.array([11, 11, 11]), np.array([7, 7, 7])))
    parts.append((np.array([8]), np.array([8])))
    ei = np.stack([np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])]).astype(np.int64)
    return np.ascontiguousarray(ei[:, rng.permutation(ei.shape[1])])


def inputs(n: int, heads: int, channels: int, seed: int = 1):
    """fp32 numpy (x_l, x_r, att, bias, G) of the tests' recipe."""
    rng = np.random.default_rng(seed)
    f = lambda s, *shape: (s * rng.standard_normal(shape)).astype(np.float32)
    return (f(0.5, n, heads * channels), f(0.5, n, heads * channels), f(0.2, heads, channels), f(0.1, channels),
            f(1.0, n, channels))


def _f64(a):
    return (a.detach() if torch.is_tensor(a) else torch.as_tensor(np.asarray(a))).double().cpu()


def _edges(ei):
    ei = torch.as_tensor(np.asarray(ei.cpu() if torch.is_tensor(ei) else ei)).long()
    return ei[0], ei[1]


def _alpha(xl3, xr3, att, src, dst, n, slope):
    H = att.size(0)
    t = xl3[src] + xr3[dst]                                                    # [E, H, C]
    e = (torch.nn.functional.leaky_relu(t, slope) * att.unsqueeze(0)).sum(-1)  # [E, H]
    mx = torch.full((n, H), -torch.inf, dtype=e.dtype)
    mx = mx.scatter_reduce(0, dst[:, None].expand(-1, H), e.detach(), "amax", include_self=True)
    ex = torch.exp(e - mx[dst])
    den = torch.zeros(n, H, dtype=e.dtype).index_add_(0, dst, ex) + 1e-16
    return t, e, ex / den[dst]


def forward(xl, xr, att, bias, ei, heads: int, slope: float = 0.2, mask=None):
    """out [N, C]; differentiable in xl, xr, att, bias (float64 tensors).  ``mask`` [E, H]: the
    dropout multipliers (None: all ones)."""
    src, dst = _edges(ei)
    n, C = xl.size(0), xl.size(1) // heads
    xl3, xr3 = xl.view(n, heads, C), xr.view(n, heads, C)
    _, _, alpha = _alpha(xl3, xr3, att.view(heads, C), src, dst, n, slope)
    am = alpha if mask is None else alpha * mask
    agg = torch.zeros(n, heads, C, dtype=xl.dtype).index_add_(0, dst, am.unsqueeze(-1) * xl3[src])
    out = agg.mean(1)
    return out if bias is None else out + bias


def autograd_grads(xl, xr, att, bias, G, ei, heads: int, slope: float = 0.2, mask=None):
    """(out, dxl, dxr, datt, dbias) of sum(out * G) by float64 autograd (xl, xr two leaves)."""
    a, b, c, d = (_f64(v).requires_grad_(True) for v in (xl, xr, att, bias))
    out = forward(a, b, c, d, ei, heads, slope, None if mask is None else _f64(mask))
    (out * _f64(G)).sum().backward()
    return out.detach(), a.grad, b.grad, c.grad.view(heads, -1), d.grad


def formulas(xl, xr, att, bias, G, ei, heads: int, slope: float = 0.2, mask=None):
    """The layer and its backward by the explicit formulas, in float64, with the term scales:
    dict(out, dxl, dxr, datt, dbias, scale_l, scale_r, scale_shared [N], e_absmax).
      dalpha = mask (g_i . x_l[j]) / H         D_i = sum_j alpha dalpha
      de     = alpha (dalpha - D_i)            dt  = de att (.) leaky'(t)
      dx_l[j] = sum_i mask alpha g_i / H + dt  dx_r[i] = sum_j dt
      datt   = sum_ij de leaky_relu(t)         dbias = sum_i g_i
    scale_l[j] = | sum over j's out-edges of |mask alpha g / H| + alpha (|dalpha| + |D|) |att (.) leaky'| |_2,
    scale_r[i] the second term over i's in-edges."""
    xl, xr, att, G = _f64(xl), _f64(xr), _f64(att), _f64(G)
    src, dst = _edges(ei)
    n, H = xl.size(0), heads
    C = xl.size(1) // H
    xl3, xr3, att = xl.view(n, H, C), xr.view(n, H, C), att.view(H, C)
    mk = torch.ones(src.numel(), H, dtype=torch.float64) if mask is None else _f64(mask)
    t, e, alpha = _alpha(xl3, xr3, att, src, dst, n, slope)
    xlj, gh = xl3[src], G[dst].unsqueeze(1)                                    # [E, H, C], [E, 1, C]
    agg = torch.zeros(n, H, C, dtype=torch.float64).index_add_(0, dst, (mk * alpha).unsqueeze(-1) * xlj)
    out = agg.mean(1) + (0 if bias is None else _f64(bias))
    dalpha = mk * (gh * xlj).sum(-1) / H
    D = torch.zeros(n, H, dtype=torch.float64).index_add_(0, dst, alpha * dalpha)
    de = alpha * (dalpha - D[dst])
    lp = torch.where(t > 0, torch.ones_like(t), torch.full_like(t, slope)) * att.unsqueeze(0)  # att (.) leaky'(t)
    dt = de.unsqueeze(-1) * lp
    msg = (mk * alpha / H).unsqueeze(-1) * gh
    z = lambda: torch.zeros(n, H, C, dtype=torch.float64)
    s_att = (alpha * (dalpha.abs() + D[dst].abs())).unsqueeze(-1) * lp.abs()
    sv_l, sv_r = z().index_add_(0, src, msg.abs() + s_att).view(n, -1), z().index_add_(0, dst, s_att).view(n, -1)
    return {
        "out": out,
        "dxl": z().index_add_(0, src, msg + dt).view(n, H * C),
        "dxr": z().index_add_(0, dst, dt).view(n, H * C),
        "datt": (de.unsqueeze(-1) * torch.nn.functional.leaky_relu(t, slope)).sum(0),
        "dbias": G.sum(0),
        "scale_l": sv_l.norm(dim=1),
        "scale_r": sv_r.norm(dim=1),
        "scale_shared": (sv_l + sv_r).norm(dim=1),  # x_r is x_l: the row sums both sets of terms
        "e_absmax": float(e.abs().max()) if e.numel() else 0.0,
    }


def rel(a, b) -> float:
    """Whole-tensor relative error |a - b|_2 / |b|_2 in float64."""
    a, b = _f64(a).reshape(-1), _f64(b).reshape(-1)
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def scaled_rows(a, b, scale):
    """(max over the rows with scale > 0 of |a_i - b_i|_2 / scale_i, max |a| over the rows with
    scale == 0): the row-wise gradient figure and what must be exactly 0."""
    a, b, s = _f64(a), _f64(b), _f64(scale)
    err = (a - b).norm(dim=1)
    nz = s > 0
    worst = float((err[nz] / s[nz]).max()) if nz.any() else 0.0
    zmax = float(a[~nz].abs().max()) if (~nz).any() else 0.0
    return worst, zmax


def self_check(heads: int = 2, channels: int = 8, p_mask: bool = True):
    """The explicit formulas against float64 autograd on a small random graph with repeated edges,
    a self-loop and an isolated node; returns the largest relative difference."""
    rng = np.random.default_rng(3)
    n, E = 40, 300
    ei = np.stack([rng.integers(0, n - 1, E), rng.integers(0, n - 1, E)])
    ei[:, :3] = np.array([[5, 5, 7], [6, 6, 7]])
    xl, xr, att, bias, G = inputs(n, heads, channels, seed=4)
    mask = torch.from_numpy(np.where(rng.random((E, heads)) < 0.3, 0.0, 1 / 0.7)) if p_mask else None
    out, dxl, dxr, datt, dbias = autograd_grads(xl, xr, att, bias, G, ei, heads, 0.2, mask)
    f = formulas(xl, xr, att, bias, G, ei, heads, 0.2, mask)
    return max(rel(f["out"], out), rel(f["dxl"], dxl), rel(f["dxr"], dxr), rel(f["datt"], datt),
               rel(f["dbias"], dbias))
