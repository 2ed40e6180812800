"""Recommender models around the drop-in layers, same structure and state_dict keys
as the reference so checkpoints ({"state_dict", "config"}) load both ways:

``PyGGAT``    -- scripts/train_gat_pyg.py:68-88  (user_emb, item_proj, convs.{l})
``CustomGAT`` -- scripts/train_gat_custom.py:96-115 (user_emb, item_proj, layers.{l})
``PyGGATv2``  -- PyGGAT with ``GATv2Conv`` layers (dynamic attention); no reference script

node_features = cat(user_emb.weight, item_proj(item_feats)); L stacked layers with no
nonlinearity in between (train_gat_pyg.py:86-87).  forward() hands the two row blocks to
the first layer separately (``forward_segments``), so the concatenation is never
materialised; ``node_features`` still returns it for callers that want it.  The two blocks
live back to back in one node table (``node_table``: the user embedding's storage is its
first rows, the item projection writes the rest), so a layer that does need them as one
tensor (the aggregate-then-transform layer of config 5) gets it without a copy.
"""
from __future__ import annotations

import os

import torch

from . import hip_ops
from .conv import GATConv, GATv2Conv, SimpleGATLayer


def node_table(model: torch.nn.Module, n_items: int) -> torch.Tensor:
    """[n_users + n_items, hidden]: rows [0, n_users) ARE model.user_emb.weight's storage
    (re-pointed here once, values kept; optimisers hold the same Parameter object), rows
    [n_users, N) take the item projection each forward.  Rebuilt if the weight moved (.to(),
    a new device) or the item count changed."""
    w = model.user_emb.weight
    t = getattr(model, "_node_rows", None)
    if (t is None or t.device != w.device or t.dtype != w.dtype or t.shape != (w.size(0) + n_items, w.size(1))
            or w.data_ptr() != t.data_ptr()):
        t = torch.empty(w.size(0) + n_items, w.size(1), dtype=w.dtype, device=w.device)
        t[:w.size(0)].copy_(w.detach())
        w.data = t[:w.size(0)]
        model._node_rows = t
    return t


class _TableGuard(torch.autograd.Function):
    """Identity on the node table's item rows, whose backward checks that no later forward
    rewrote them.  The item projection writes them through a raw pointer each forward (no
    version-counter bump: a bump would trip autograd's view checks on the table's views), so a
    graph whose backward runs after another forward -- its layers saved those rows -- would
    otherwise take the new rows' values silently; here it raises instead.  (One forward in
    flight per model: the node table is a per-model buffer.)"""

    @staticmethod
    def forward(ctx, v, holder, gen: int):
        ctx.holder, ctx.gen = holder, gen
        return v.view_as(v)

    @staticmethod
    def backward(ctx, g):
        if ctx.holder[0]._node_rows_gen != ctx.gen:
            raise RuntimeError("ppgat node table: the item rows this graph saved were rewritten by a later "
                               "forward of the same model; run backward before the next forward "
                               "(or PPGAT_NODE_TABLE=0)")
        return g, None, None


def _unalias_state(module, state_dict, prefix, local_metadata):
    """state_dict hook: the user embedding shares the node table's storage; hand out its own copy
    (torch.save would otherwise write the whole table)."""
    k = prefix + "user_emb.weight"
    v = state_dict.get(k)
    if v is not None and v.untyped_storage().nbytes() > v.numel() * v.element_size():
        state_dict[k] = v.clone()


def _stack(model, item_proj, item_feats, layers, edge_index, edge_attr=None):
    """``edge_attr`` (GATConv layers built with edge_dim): the same tensor feeds every layer."""
    ea = {} if edge_attr is None else {"edge_attr": edge_attr}
    user_w = model.user_emb.weight
    if user_w.is_cuda and os.environ.get("PPGAT_NODE_TABLE", "1") != "0":
        table = node_table(model, item_feats.size(0))
        v = hip_ops.linear(item_feats, item_proj.weight, item_proj.bias, out=table[user_w.size(0):])
        gen = getattr(model, "_node_rows_gen", 0) + 1
        model._node_rows_gen = gen
        if torch.is_grad_enabled() and v.requires_grad:
            v = _TableGuard.apply(v, [model], gen)
    else:
        v = hip_ops.linear(item_feats, item_proj.weight, item_proj.bias)
    if len(layers) == 0:
        return torch.cat([user_w, v], dim=0)
    x = layers[0].forward_segments(user_w, v, edge_index, **ea)
    for layer in list(layers)[1:]:
        x = layer(x, edge_index, **ea)
    return x


def forward_subgraph(model, item_feats, sub, edge_attr=None, sparse_grad=False):
    """The layer stack on a ``neighbors.Subgraph``: ``Z_s [N_s, d]``, row k the embedding of node
    ``sub.n_id[k]`` (exact at the seeds when ``hops`` = the number of layers: a seed's output reads
    its sampled neighbourhood to that depth and no further).  Only the subgraph's nodes are touched:
    user rows are ``user_emb.weight.index_select(0, n_id[:n_users_s])``, item rows the projection of
    the subgraph's items alone -- the node-side saving -- and the node table of ``_stack`` is not
    used.  The embedding gradient arrives through ``index_select``'s backward; ``n_id`` is unique,
    so each row is added once.  ``edge_attr``: the PARENT graph's [E, D] tensor, gathered by
    ``sub.eid`` here.  ``sparse_grad=True``: the user rows come from ``hip_ops.embedding_rows``, whose
    gradient for ``user_emb.weight`` is row-sparse over ``n_id[:n_users_s]`` (no zero-filled
    [n_users, d] gradient) -- for ``optim.Adam``'s lazy row step.  ``n_id`` is V ascending, so those
    indices are strictly ascending and in range: ``optim.Adam(rows="ascending")`` is sound for them."""
    layers = model.convs if hasattr(model, "convs") else model.layers
    nu = sub.n_users_s
    if sparse_grad:
        xu = hip_ops.embedding_rows(model.user_emb.weight, sub.n_id[:nu])
    else:
        xu = model.user_emb.weight.index_select(0, sub.n_id[:nu])
    if sub.n_nodes > nu:
        feats = item_feats.index_select(0, sub.n_id[nu:] - model.n_users)
        xv = hip_ops.linear(feats, model.item_proj.weight, model.item_proj.bias)
    else:
        xv = xu.new_zeros((0, xu.size(1)))
    x = torch.cat([xu, xv], dim=0)
    ea = {} if edge_attr is None else {"edge_attr": edge_attr.index_select(0, sub.eid)}
    for layer in layers:
        x = layer(x, sub.edge_index_s, **ea)
    return x


def layer_attention(model, layers, item_feats, edge_index, edge_attr=None, order: str = "edge", only=None):
    """The attention weights of a model's layer stack: a list with one [E, H] fp32 tensor per layer
    (``only``: that layer alone, the stack run no further), alpha before the dropout mask, row k
    for column k of ``edge_index`` (``order="slot"``: CSR slot order).  Runs in eval mode under
    no_grad -- the weights a served model would use -- and puts every module's training flag
    back afterwards.  Per layer the weights cost a second forward (``layer.attention``)."""
    ea = {} if edge_attr is None else {"edge_attr": edge_attr}
    n = len(layers)
    if only is not None:
        if not -n <= only < n:
            raise IndexError(f"layer {only} of a {n}-layer model")
        only = only % n
    flags = [(mod, mod.training) for mod in model.modules()]
    model.eval()
    try:
        with torch.no_grad():
            x = model.node_features(item_feats)
            out = []
            for l, layer in enumerate(layers):
                if only is None or l == only:
                    out.append(layer.attention(x, edge_index, order=order, **ea))
                if l == n - 1 or l == only:
                    break
                x = layer(x, edge_index, **ea)
    finally:
        for mod, was in flags:
            mod.training = was
    return out


class PyGGAT(torch.nn.Module):
    def __init__(self, n_users: int, n_items: int, item_feat_dim: int, hidden: int, layers: int, heads: int,
                 attn_dropout: float, edge_dim=None):
        super().__init__()
        self.n_users, self.n_items = n_users, n_items
        self.edge_dim = edge_dim
        self.user_emb = torch.nn.Embedding(n_users, hidden)
        torch.nn.init.normal_(self.user_emb.weight, std=0.1)
        self.item_proj = torch.nn.Linear(item_feat_dim, hidden)
        self.convs = torch.nn.ModuleList()
        for _ in range(layers):
            self.convs.append(GATConv(hidden, hidden, heads=heads, dropout=attn_dropout, add_self_loops=False,
                                      concat=False, edge_dim=edge_dim))
        self._register_state_dict_hook(_unalias_state)

    def node_features(self, item_feats: torch.Tensor) -> torch.Tensor:
        u = self.user_emb.weight
        v = hip_ops.linear(item_feats, self.item_proj.weight, self.item_proj.bias)
        return torch.cat([u, v], dim=0)

    def forward(self, item_feats: torch.Tensor, edge_index: torch.Tensor, edge_attr=None) -> torch.Tensor:
        return _stack(self, self.item_proj, item_feats, self.convs, edge_index, edge_attr)

    def forward_subgraph(self, item_feats: torch.Tensor, sub, edge_attr=None, sparse_grad=False) -> torch.Tensor:
        """``Z_s [N_s, hidden]`` on a ``neighbors.Subgraph`` (model.forward_subgraph)."""
        return forward_subgraph(self, item_feats, sub, edge_attr, sparse_grad)

    def attention(self, item_feats: torch.Tensor, edge_index: torch.Tensor, edge_attr=None, order: str = "edge"):
        """One [E, H] attention tensor per layer (layer_attention)."""
        return layer_attention(self, self.convs, item_feats, edge_index, edge_attr, order)


class PyGGATv2(torch.nn.Module):
    """``PyGGAT`` with GATv2's dynamic attention: the same user_emb / item_proj / convs.{l}
    structure, each conv a ``GATv2Conv(hidden, hidden, heads, concat=False, add_self_loops=False)``."""

    def __init__(self, n_users: int, n_items: int, item_feat_dim: int, hidden: int, layers: int, heads: int,
                 attn_dropout: float, share_weights: bool = False):
        super().__init__()
        self.n_users, self.n_items = n_users, n_items
        self.user_emb = torch.nn.Embedding(n_users, hidden)
        torch.nn.init.normal_(self.user_emb.weight, std=0.1)
        self.item_proj = torch.nn.Linear(item_feat_dim, hidden)
        self.convs = torch.nn.ModuleList()
        for _ in range(layers):
            self.convs.append(GATv2Conv(hidden, hidden, heads=heads, dropout=attn_dropout, add_self_loops=False,
                                        concat=False, share_weights=share_weights))
        self._register_state_dict_hook(_unalias_state)

    def node_features(self, item_feats: torch.Tensor) -> torch.Tensor:
        u = self.user_emb.weight
        v = hip_ops.linear(item_feats, self.item_proj.weight, self.item_proj.bias)
        return torch.cat([u, v], dim=0)

    def forward(self, item_feats: torch.Tensor, edge_index: torch.Tensor) -> torch.Tensor:
        return _stack(self, self.item_proj, item_feats, self.convs, edge_index)

    def forward_subgraph(self, item_feats: torch.Tensor, sub, edge_attr=None, sparse_grad=False) -> torch.Tensor:
        """``Z_s [N_s, hidden]`` on a ``neighbors.Subgraph`` (model.forward_subgraph); no ``edge_attr``."""
        if edge_attr is not None:
            raise NotImplementedError("PyGGATv2: edge features are not implemented")
        return forward_subgraph(self, item_feats, sub, sparse_grad=sparse_grad)

    def attention(self, item_feats: torch.Tensor, edge_index: torch.Tensor, edge_attr=None, order: str = "edge"):
        """One [E, H] attention tensor per layer (layer_attention); GATv2Conv takes no ``edge_attr``."""
        if edge_attr is not None:
            raise NotImplementedError("PyGGATv2: edge features are not implemented")
        return layer_attention(self, self.convs, item_feats, edge_index, None, order)


class CustomGAT(torch.nn.Module):
    def __init__(self, n_users: int, n_items: int, item_feat_dim: int, hidden: int, layers: int):
        super().__init__()
        self.n_users, self.n_items = n_users, n_items
        self.user_emb = torch.nn.Embedding(n_users, hidden)
        torch.nn.init.normal_(self.user_emb.weight, std=0.1)
        self.item_proj = torch.nn.Linear(item_feat_dim, hidden)
        self.layers = torch.nn.ModuleList([SimpleGATLayer(hidden, hidden) for _ in range(layers)])
        self._register_state_dict_hook(_unalias_state)

    def node_features(self, item_feats: torch.Tensor) -> torch.Tensor:
        u = self.user_emb.weight
        v = hip_ops.linear(item_feats, self.item_proj.weight, self.item_proj.bias)
        return torch.cat([u, v], dim=0)

    def forward(self, item_feats: torch.Tensor, edge_index: torch.Tensor) -> torch.Tensor:
        return _stack(self, self.item_proj, item_feats, self.layers, edge_index)

    def forward_subgraph(self, item_feats: torch.Tensor, sub, edge_attr=None, sparse_grad=False) -> torch.Tensor:
        """``Z_s [N_s, hidden]`` on a ``neighbors.Subgraph`` (model.forward_subgraph); no ``edge_attr``."""
        if edge_attr is not None:
            raise NotImplementedError("CustomGAT: edge features are not implemented")
        return forward_subgraph(self, item_feats, sub, sparse_grad=sparse_grad)

    def attention(self, item_feats: torch.Tensor, edge_index: torch.Tensor, edge_attr=None, order: str = "edge"):
        """One [E, 1] attention tensor per layer (layer_attention); the custom layer takes no ``edge_attr``."""
        if edge_attr is not None:
            raise NotImplementedError("CustomGAT: edge features are not implemented")
        return layer_attention(self, self.layers, item_feats, edge_index, None, order)


def bpr_loss(Z: torch.Tensor, n_users: int, u, i, j, loss: str = "bpr", prepared=None) -> torch.Tensor:
    """Loss of the train step, scripts/train_gat_pyg.py:313-322 (BPR or BCE), fused on the
    device (ppgat_bpr_fwd / ppgat_bpr_bwd; with ``prepared`` from ``hip_ops.bpr_prepare`` the
    backward's triple sort has already run beside the forward)."""
    return hip_ops.bpr_loss(Z, n_users, u, i, j, loss, prepared=prepared)


def softmax_loss(Z: torch.Tensor, n_users: int, u, cand, temperature: float = 1.0, correction=None) -> torch.Tensor:
    """Sampled-softmax loss of the positive ``cand[:, 0]`` against the negatives ``cand[:, 1:]``,
    fused on the device (ppgat_ssm_fwd / ppgat_ssm_bwd); ``correction``: the negatives' logQ table."""
    return hip_ops.softmax_loss(Z, n_users, u, cand, temperature, correction=correction)


def shared_softmax_loss(Z: torch.Tensor, n_users: int, u, pos, pool, temperature: float = 1.0,
                        history=None, correction=None) -> torch.Tensor:
    """Softmax loss of the positives ``pos`` against one ``pool`` of item ids shared by every sample,
    the sample's positive and its user's ``history`` masked out, fused on the device
    (ppgat_shs_fwd / ppgat_shs_bwd); ``correction``: the pool's logQ table."""
    if correction is None:
        return hip_ops.shared_softmax_loss(Z, n_users, u, pos, pool, temperature, history=history)
    return hip_ops.shared_softmax_loss_corrected(Z, n_users, u, pos, pool, temperature, history=history,
                                                 correction=correction)
