"""Drop-in GAT layers backed by the fused HIP kernels.

``GATConv``        -- torch_geometric.nn.GATConv as the reference constructs it
                      (scripts/train_gat_pyg.py:77: heads=H, dropout=p,
                      add_self_loops=False, concat=False); same constructor names,
                      ``forward(x, edge_index)``, and state_dict keys
                      (``lin.weight`` [H*C, F], ``att_src``/``att_dst`` [1, H, C],
                      ``bias`` [C]; the older ``lin_src.weight``/``lin_dst.weight`` keys load too).
                      ``edge_dim=D`` (1..16) adds PyG's ``lin_edge.weight`` [H*C, D] and
                      ``att_edge`` [1, H, C] and ``forward(x, edge_index, edge_attr)``.
``GATv2Conv``      -- torch_geometric.nn.GATv2Conv (dynamic attention) under the same options,
                      PyG's constructor names and state_dict keys (``att``, ``lin_l.*``,
                      ``lin_r.*``, ``bias``); runs as ``hip_ops.gatv2_aggregate`` after two
                      ``hip_ops.linear`` projections.
``SimpleGATLayer`` -- scripts/train_gat_custom.py:63-93, same constructor
                      ``(in_dim, out_dim, attn_dropout=0.1)``, same parameter creation
                      order (so a seeded construction yields the reference's weights)
                      and keys (``lin.weight``, ``a_src``, ``a_dst``).

``GATConv`` and ``SimpleGATLayer`` run the layer as ``hip_ops.gat_layer``, entirely in
``libppgat.so``: ``h = lin(x)`` on the fp32 matrix cores with the node attention terms in the GEMM epilogue, the fused
edge kernels, and a backward that folds the attention terms into the projection GEMMs;
multi-head layers wider than their input (config 5) run aggregate-then-transform
(``hip_ops.GATLayerX``: x_j gathered once per edge, one transform GEMM).  Dropout on alpha is the counter-hash mask of
include/ppgat.h, drawn fresh per training forward from torch's CPU generator.

``forward(..., return_attention_weights=True)`` returns PyG's tuple ``(out, (edge_index, alpha))``
with alpha [E, H] fp32 in edge_index column order, detached.  alpha is the softmax weight BEFORE
the dropout mask, in train mode too: each destination's weights sum to 1 and the result is
deterministic.  (PyG >= 2.3 returns the weights after dropout in train mode; in eval mode the two
agree.)  ``out`` comes from the same call as without the flag; alpha from a second, no-grad
forward over the unfused primitives (``layer.attention``), so the flag costs about one more
forward.
"""
from __future__ import annotations

import math

import torch

from . import _launch, _lib
from .hip_ops import (EDGE_MAX_DIM, check_edge_attr, gat_layer, gat_layer_attention, gatv2_aggregate,
                      gatv2_layer_attention, gatv2_supported, graph_cache, join_rows, linear)


def _dropout_seed() -> int:
    return int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())


def _glorot_(t: torch.Tensor):
    """PyG inits.glorot: U(+-sqrt(6 / (size(-2) + size(-1))))."""
    a = math.sqrt(6.0 / (t.size(-2) + t.size(-1)))
    with torch.no_grad():
        t.uniform_(-a, a)
    return t


class GATConv(torch.nn.Module):
    """MI355X-native ``GATConv`` (PyG semantics)."""

    def __init__(self, in_channels: int, out_channels: int, heads: int = 1, concat: bool = True,
                 negative_slope: float = 0.2, dropout: float = 0.0, add_self_loops: bool = True,
                 edge_dim=None, fill_value="mean", bias: bool = True, residual: bool = False, **kwargs):
        super().__init__()
        if isinstance(in_channels, (tuple, list)):
            raise NotImplementedError("bipartite (tuple) in_channels not implemented")
        if concat:
            raise NotImplementedError("GATConv(concat=True) not implemented; the reference uses concat=False")
        if add_self_loops:
            raise NotImplementedError("GATConv(add_self_loops=True) not implemented; the reference passes False")
        if edge_dim is not None:
            if int(edge_dim) < 1:
                raise ValueError(f"edge_dim={edge_dim}: expected at least 1")
            if int(edge_dim) > EDGE_MAX_DIM:
                raise NotImplementedError(f"edge_dim={edge_dim} not implemented (edge_dim <= {EDGE_MAX_DIM})")
            edge_dim = int(edge_dim)
        if residual:
            raise NotImplementedError("residual=True not implemented")
        if not _launch.supported_channels(out_channels):
            raise NotImplementedError(f"out_channels={out_channels}: fused kernels take C in 4*2^k <= 256")
        if heads > 8:
            raise NotImplementedError("heads > 8 not implemented")
        self.in_channels, self.out_channels, self.heads = in_channels, out_channels, heads
        self.concat, self.negative_slope, self.dropout = concat, negative_slope, dropout
        self.add_self_loops, self.edge_dim = add_self_loops, edge_dim
        self.lin = torch.nn.Linear(in_channels, heads * out_channels, bias=False)
        self.att_src = torch.nn.Parameter(torch.empty(1, heads, out_channels))
        self.att_dst = torch.nn.Parameter(torch.empty(1, heads, out_channels))
        self.bias = torch.nn.Parameter(torch.empty(out_channels)) if bias else None
        # the edge parameters after the existing ones, created without drawing from the generator
        # (reset_parameters initialises them last): a seeded construction gives the same lin /
        # att_src / att_dst as the layer without edge_dim
        if edge_dim is not None:
            self.lin_edge = torch.nn.utils.skip_init(torch.nn.Linear, edge_dim, heads * out_channels, bias=False)
            self.att_edge = torch.nn.Parameter(torch.empty(1, heads, out_channels))
        else:
            self.lin_edge = None
            self.register_parameter("att_edge", None)
        self.reset_parameters()

    def reset_parameters(self):
        _glorot_(self.lin.weight)
        _glorot_(self.att_src)
        _glorot_(self.att_dst)
        if self.bias is not None:
            torch.nn.init.zeros_(self.bias)
        if self.lin_edge is not None:
            _glorot_(self.lin_edge.weight)
            _glorot_(self.att_edge)

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                              error_msgs):
        # older PyG: lin_src / lin_dst share one weight (in_channels is an int)
        old = prefix + "lin_src.weight"
        if old in state_dict and prefix + "lin.weight" not in state_dict:
            state_dict[prefix + "lin.weight"] = state_dict.pop(old)
            state_dict.pop(prefix + "lin_dst.weight", None)
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                                      error_msgs)

    def _edge_args(self, edge_attr, n_edges: int, device) -> dict:
        """gat_layer's edge arguments: ``edge_attr`` as the caller passed it (the staging cache keys
        on that tensor object) and v [H, D], v[h, d] = sum_c att_edge[h, c] lin_edge.weight[h C + c, d]
        -- an elementwise product and a sum, so autograd turns dv into both parameters' gradients."""
        if edge_attr is None:  # PyG skips the term in the same way
            return {}
        if self.edge_dim is None:
            raise ValueError("edge_attr given to a GATConv built without edge_dim")
        check_edge_attr(edge_attr, n_edges, device)
        D = 1 if edge_attr.dim() == 1 else edge_attr.size(1)
        if D != self.edge_dim:
            raise ValueError(f"edge_attr: {D} features per edge, but edge_dim={self.edge_dim}")
        w = self.lin_edge.weight.view(self.heads, self.out_channels, self.edge_dim)
        v = (w * self.att_edge.view(self.heads, self.out_channels, 1)).sum(1)
        return {"edge_v": v, "edge_attr": edge_attr}

    def attention(self, x: torch.Tensor, edge_index: torch.Tensor, edge_attr=None, x_items=None,
                  order: str = "edge") -> torch.Tensor:
        """alpha [E, H] of forward(x, edge_index, edge_attr) -- of forward_segments with ``x_items`` --
        before the dropout mask, whatever the training flag: fp32, no gradient, row k for column k of
        edge_index (``order="slot"``: CSR slot order, what hip_ops.attention_topk reads).  A forward of
        its own (hip_ops.gat_layer_attention)."""
        n = x.size(0) + (x_items.size(0) if x_items is not None else 0)
        graph = graph_cache.get(edge_index, n)
        with torch.no_grad():
            ea = self._edge_args(edge_attr, graph.n_edges, x.device)
        return gat_layer_attention(x, self.lin.weight, self.att_src, self.att_dst, graph, self.heads,
                                   self.out_channels, _lib.MODE_PYG, float(self.negative_slope), x_items=x_items,
                                   order=order, **ea)

    def forward(self, x: torch.Tensor, edge_index: torch.Tensor, edge_attr=None,
                return_attention_weights=None) -> torch.Tensor:
        """``return_attention_weights=True``: ``(out, (edge_index, alpha))``, alpha [E, H] before the
        dropout mask (see the module docstring); costs a second forward."""
        graph = graph_cache.get(edge_index, x.size(0))
        p = float(self.dropout) if self.training else 0.0
        seed = _dropout_seed() if p > 0 else 0
        out = gat_layer(x, self.lin.weight, self.att_src, self.att_dst, self.bias, graph, self.heads,
                        self.out_channels, _lib.MODE_PYG, float(self.negative_slope), p, seed,
                        **self._edge_args(edge_attr, graph.n_edges, x.device))
        if return_attention_weights:
            return out, (edge_index, self.attention(x, edge_index, edge_attr))
        return out

    def forward_segments(self, x: torch.Tensor, x_items: torch.Tensor, edge_index: torch.Tensor,
                         edge_attr=None, return_attention_weights=None) -> torch.Tensor:
        """forward(cat(x, x_items), edge_index, edge_attr) without materialising the concatenation
        (the model's node features, train_gat_pyg.py:79-82)."""
        graph = graph_cache.get(edge_index, x.size(0) + x_items.size(0))
        p = float(self.dropout) if self.training else 0.0
        seed = _dropout_seed() if p > 0 else 0
        out = gat_layer(x, self.lin.weight, self.att_src, self.att_dst, self.bias, graph, self.heads,
                        self.out_channels, _lib.MODE_PYG, float(self.negative_slope), p, seed, x_items=x_items,
                        **self._edge_args(edge_attr, graph.n_edges, x.device))
        if return_attention_weights:
            return out, (edge_index, self.attention(x, edge_index, edge_attr, x_items=x_items))
        return out

    def __repr__(self):
        return (f"{self.__class__.__name__}({self.in_channels}, {self.out_channels}, heads={self.heads}, "
                f"backend=hip)")


class GATv2Conv(torch.nn.Module):
    """MI355X-native ``torch_geometric.nn.GATv2Conv`` (dynamic attention, Brody et al.) with the
    options ``GATConv`` above supports: ``e_ij = att . leaky_relu(lin_l(x)_j + lin_r(x)_i)``,
    softmax per destination, dropout on alpha, head mean, bias.  PyG's constructor names and
    defaults, and its state_dict keys (``att`` [1, H, C], ``lin_l.weight`` [H*C, F],
    ``lin_l.bias`` [H*C], ``lin_r.*`` -- the same module as ``lin_l`` with ``share_weights`` --
    and ``bias`` [C]).  The projections run through ``hip_ops.linear``, the rest in the fused
    kernels of ``hip_ops.gatv2_aggregate``."""

    def __init__(self, in_channels: int, out_channels: int, heads: int = 1, concat: bool = True,
                 negative_slope: float = 0.2, dropout: float = 0.0, add_self_loops: bool = True,
                 edge_dim=None, fill_value="mean", bias: bool = True, share_weights: bool = False,
                 residual: bool = False, **kwargs):
        super().__init__()
        if isinstance(in_channels, (tuple, list)):
            raise NotImplementedError("bipartite (tuple) in_channels not implemented")
        if concat:
            raise NotImplementedError("GATv2Conv(concat=True) not implemented; pass concat=False")
        if add_self_loops:
            raise NotImplementedError("GATv2Conv(add_self_loops=True) not implemented; pass False")
        if edge_dim is not None:
            raise NotImplementedError("edge_dim (edge features) not implemented")
        if residual:
            raise NotImplementedError("residual=True not implemented")
        if not gatv2_supported(int(heads), int(out_channels)):
            raise NotImplementedError(f"GATv2Conv(heads={heads}, out_channels={out_channels}) not implemented: "
                                      "(H, C) in (1,32) (1,64) (1,128) (2,64) (2,128) (4,64) (4,128)")
        self.in_channels, self.out_channels, self.heads = in_channels, out_channels, heads
        self.concat, self.negative_slope, self.dropout = concat, negative_slope, dropout
        self.add_self_loops, self.edge_dim, self.fill_value = add_self_loops, edge_dim, fill_value
        self.share_weights, self.residual = share_weights, residual
        self.lin_l = torch.nn.Linear(in_channels, heads * out_channels, bias=bias)
        self.lin_r = self.lin_l if share_weights else torch.nn.Linear(in_channels, heads * out_channels, bias=bias)
        self.att = torch.nn.Parameter(torch.empty(1, heads, out_channels))
        self.bias = torch.nn.Parameter(torch.empty(out_channels)) if bias else None
        self.reset_parameters()

    def reset_parameters(self):
        for lin in (self.lin_l,) if self.share_weights else (self.lin_l, self.lin_r):
            _glorot_(lin.weight)
            if lin.bias is not None:
                torch.nn.init.zeros_(lin.bias)
        _glorot_(self.att)
        if self.bias is not None:
            torch.nn.init.zeros_(self.bias)

    def _aggregate(self, x: torch.Tensor, edge_index: torch.Tensor, want_alpha=None):
        graph = graph_cache.get(edge_index, x.size(0))
        p = float(self.dropout) if self.training else 0.0
        seed = _dropout_seed() if p > 0 else 0
        xl = linear(x, self.lin_l.weight, self.lin_l.bias)
        xr = xl if self.share_weights else linear(x, self.lin_r.weight, self.lin_r.bias)
        out = gatv2_aggregate(xl, xr, self.att, self.bias, graph, self.heads, self.out_channels,
                              float(self.negative_slope), p, seed)
        if want_alpha:  # from the projections at hand: a second aggregate, no second projection
            return out, (edge_index, gatv2_layer_attention(xl, xr, self.att, graph, self.heads, self.out_channels,
                                                           float(self.negative_slope)))
        return out

    def attention(self, x: torch.Tensor, edge_index: torch.Tensor, order: str = "edge") -> torch.Tensor:
        """alpha [E, H] of forward(x, edge_index) before the dropout mask, whatever the training flag:
        fp32, no gradient, row k for column k of edge_index (``order="slot"``: CSR slot order).  A
        forward of its own: ``linear`` and hip_ops.gatv2_layer_attention."""
        graph = graph_cache.get(edge_index, x.size(0))
        with torch.no_grad():
            xl = linear(x, self.lin_l.weight, self.lin_l.bias)
            xr = xl if self.share_weights else linear(x, self.lin_r.weight, self.lin_r.bias)
        return gatv2_layer_attention(xl, xr, self.att, graph, self.heads, self.out_channels,
                                     float(self.negative_slope), order=order)

    def forward(self, x: torch.Tensor, edge_index: torch.Tensor, return_attention_weights=None) -> torch.Tensor:
        """``return_attention_weights=True``: ``(out, (edge_index, alpha))``, alpha [E, H] before the
        dropout mask (see the module docstring); costs a second aggregate."""
        return self._aggregate(x, edge_index, return_attention_weights)

    def forward_segments(self, x: torch.Tensor, x_items: torch.Tensor, edge_index: torch.Tensor,
                         return_attention_weights=None) -> torch.Tensor:
        """forward(cat(x, x_items), edge_index); the two blocks are joined without a copy when they
        lie back to back (the model's node table), else concatenated."""
        return self._aggregate(join_rows(x, x_items), edge_index, return_attention_weights)

    def __repr__(self):
        return (f"{self.__class__.__name__}({self.in_channels}, {self.out_channels}, heads={self.heads}, "
                f"share_weights={self.share_weights}, backend=hip)")


class SimpleGATLayer(torch.nn.Module):
    """MI355X-native ``SimpleGATLayer`` (scripts/train_gat_custom.py:63-93)."""

    def __init__(self, in_dim: int, out_dim: int, attn_dropout: float = 0.1):
        super().__init__()
        if not _launch.supported_channels(out_dim):
            raise NotImplementedError(f"out_dim={out_dim}: fused kernels take C in 4*2^k <= 256")
        # creation/initialisation order identical to the reference (RNG-consuming calls)
        self.lin = torch.nn.Linear(in_dim, out_dim, bias=False)
        self.a_src = torch.nn.Parameter(torch.empty(out_dim))
        self.a_dst = torch.nn.Parameter(torch.empty(out_dim))
        torch.nn.init.xavier_uniform_(self.lin.weight)
        torch.nn.init.xavier_uniform_(self.a_src.unsqueeze(0))
        torch.nn.init.xavier_uniform_(self.a_dst.unsqueeze(0))
        self.leaky = torch.nn.LeakyReLU(0.2)
        self.drop = torch.nn.Dropout(attn_dropout)
        self.out_dim = out_dim

    def attention(self, x: torch.Tensor, edge_index: torch.Tensor, x_items=None, order: str = "edge") -> torch.Tensor:
        """alpha [E, 1] of forward(x, edge_index) -- of forward_segments with ``x_items`` -- before the
        dropout mask, whatever the training flag: exp(clamp(leaky_relu(z), -10, 10)) / (sum + 1e-9),
        fp32, no gradient, row k for column k of edge_index (``order="slot"``: CSR slot order).  A
        forward of its own (hip_ops.gat_layer_attention)."""
        n = x.size(0) + (x_items.size(0) if x_items is not None else 0)
        graph = graph_cache.get(edge_index, n)
        return gat_layer_attention(x, self.lin.weight, self.a_src, self.a_dst, graph, 1, self.out_dim,
                                   _lib.MODE_CUSTOM, float(self.leaky.negative_slope), x_items=x_items, order=order)

    def forward(self, x: torch.Tensor, edge_index: torch.Tensor, return_attention_weights=None) -> torch.Tensor:
        """``return_attention_weights=True``: ``(out, (edge_index, alpha))``, alpha [E, 1] before the
        dropout mask (see the module docstring); costs a second forward."""
        graph = graph_cache.get(edge_index, x.size(0))
        p = float(self.drop.p) if self.training else 0.0
        seed = _dropout_seed() if p > 0 else 0
        out = gat_layer(x, self.lin.weight, self.a_src, self.a_dst, None, graph, 1, self.out_dim, _lib.MODE_CUSTOM,
                        float(self.leaky.negative_slope), p, seed)
        if return_attention_weights:
            return out, (edge_index, self.attention(x, edge_index))
        return out

    def forward_segments(self, x: torch.Tensor, x_items: torch.Tensor, edge_index: torch.Tensor,
                         return_attention_weights=None) -> torch.Tensor:
        """forward(cat(x, x_items), edge_index) without materialising the concatenation."""
        graph = graph_cache.get(edge_index, x.size(0) + x_items.size(0))
        p = float(self.drop.p) if self.training else 0.0
        seed = _dropout_seed() if p > 0 else 0
        out = gat_layer(x, self.lin.weight, self.a_src, self.a_dst, None, graph, 1, self.out_dim, _lib.MODE_CUSTOM,
                        float(self.leaky.negative_slope), p, seed, x_items=x_items)
        if return_attention_weights:
            return out, (edge_index, self.attention(x, edge_index, x_items=x_items))
        return out
