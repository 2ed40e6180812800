"""Gather skipping in the GAT edge kernels (include/ppgat.h ppgat_set_gather_skip): a neighbour
row whose weight is exactly zero (dropped edge) or whose grad_out row is marked all-zero in
nstate (D = -0.0f) is not loaded.  Switch on and off give equal results; NaN written into the rows
that must not be read shows they are not; the producers and the prologue mark exactly the zero rows.

One small graph: destination in-degrees and source out-degrees each cover
{0, 1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 600} (the short/long boundary at 16, the 64-edge
chunk, the hub cut at 256 with more than two pieces), plus 200 sources with one out-edge and 60
destinations with one in-edge, so that under dropout whole rows go unread."""
import ctypes
from importlib import import_module

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LADDER = (0, 1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 600)
N_NODES = 1500
NEG_ZERO_BITS = -(2 ** 31)  # 0x80000000 as int32


def _mods():
    return (import_module("plotpointe-gat-recommendation_amd.hip_ops"),
            import_module("plotpointe-gat-recommendation_amd._launch"),
            import_module("plotpointe-gat-recommendation_amd._lib"))


def _ladder_edges():
    """[2, E] int64 (row 0 src, row 1 dst).  Nodes 0..12: ladder destinations, 13..25: ladder
    sources, 26..225: sources with exactly one out-edge, 226..285: destinations with exactly one
    in-edge, 286..: the pool the other endpoints are drawn from."""
    rng = np.random.default_rng(7)
    pool = np.arange(286, N_NODES)
    src, dst = [], []
    for k, d in enumerate(LADDER):
        src.append(rng.choice(pool, d, replace=False)); dst.append(np.full(d, k))
        src.append(np.full(d, 13 + k)); dst.append(rng.choice(pool, d, replace=False))
    src.append(np.arange(26, 226)); dst.append(rng.choice(pool, 200))
    src.append(rng.choice(pool, 60)); dst.append(np.arange(226, 286))
    ei = np.stack([np.concatenate(src), np.concatenate(dst)]).astype(np.int64)
    return ei[:, rng.permutation(ei.shape[1])]


@pytest.fixture(scope="module")
def graph(pkg, cuda):
    ops, _, _ = _mods()
    ei = _ladder_edges()
    g = ops.csr_build(torch.from_numpy(ei).to(cuda), N_NODES)
    indeg, outdeg = g.in_degree().cpu().numpy(), g.out_degree().cpu().numpy()
    assert [int(indeg[k]) for k in range(13)] == list(LADDER)
    assert [int(outdeg[13 + k]) for k in range(13)] == list(LADDER)
    assert (outdeg[26:226] == 1).all() and (indeg[226:286] == 1).all()
    assert g.fwd_sched.n_hubs >= 2 and g.bwd_sched.n_hubs >= 2
    return g, ei


@pytest.fixture()
def switch():
    """Sets the switch; puts the process value back afterwards."""
    _, _, lib = _mods()
    first = lib.set_gather_skip(True)
    lib.set_gather_skip(first)
    yield lib.set_gather_skip
    lib.set_gather_skip(first)


def _inputs(cuda, heads, C, seed):
    gen = torch.Generator().manual_seed(seed)
    h = torch.randn(N_NODES, heads, C, generator=gen).to(cuda)
    s_src = torch.randn(N_NODES, heads, generator=gen).to(cuda)
    s_dst = torch.randn(N_NODES, heads, generator=gen).to(cuda)
    bias = (torch.randn(C, generator=gen) * 0.1).to(cuda)
    grad = torch.randn(N_NODES, C, generator=gen)
    zero_rows = torch.rand(N_NODES, generator=gen) < 0.3
    return h, s_src, s_dst, bias, grad.to(cuda), zero_rows.to(cuda)


def _forward(g, h, s_src, s_dst, bias, heads, C, mode, p, seed):
    ops, launch, _ = _mods()
    dev = h.device
    out, m, inv_l, agg = ops._fwd_outputs(g.n_nodes, heads, C, True, dev)
    seed_buf = ops.seed_buffer(p, dev)
    launch.fwd(g.fwd_sched, g.col, g.csr_eid, g.n_edges, 0, g.n_nodes, h, s_src, s_dst, bias, heads, C, mode, 0.2, p,
               seed, seed_buf, out, m, inv_l, agg)
    return out, m, inv_l, agg, seed_buf


def _prologue(g, grad, out, agg, bias, s_dst, m, inv_l, heads, C, mode):
    _, launch, _ = _mods()
    nstate = torch.empty(g.n_nodes, heads, 4, device=grad.device)
    launch.bwd_prologue(0, g.n_nodes, grad, out, agg, bias, s_dst, m, inv_l, heads, C, mode, nstate, None)
    return nstate


def _edges(g, h, s_src, nstate, grad, heads, C, mode, p, seed, seed_buf):
    _, launch, _ = _mods()
    dev = h.device
    D = torch.empty(g.n_nodes, heads * C, device=dev)
    S = torch.zeros(g.n_nodes, 2 * heads, device=dev)
    dz = torch.empty(max(g.n_edges, 1) * heads, device=dev)
    launch.bwd_edges(g.bwd_sched, g.row, g.csc_eid, None, g.n_edges, 0, h, s_src, nstate, grad, heads, C, mode, 0.2, p,
                     seed, seed_buf, D, S, dz)
    return D, S[:, :heads].clone(), dz


def _drop_mask(oracle, seed_buf, n_edges, p):
    """kept[e] for the original edge ids (head 0), from the seed the forward used."""
    seed_used = int(seed_buf.cpu().numpy().astype(np.uint64)[0])
    return oracle.dropout_scale(seed_used, np.arange(n_edges), 0, p) != 0


# heads 1: the short and long kernels; 2: the forward's heads loop (the backward takes the
# multi-head pass, which gathers every row); 3: the heads loop of the backward's per-head kernel
# (the custom mode is defined for heads = 1 without a bias)
@pytest.mark.parametrize("mode,heads", [(0, 1), (0, 2), (0, 3), (1, 1)],
                         ids=["pyg-h1", "pyg-h2", "pyg-h3", "custom-h1"])
@pytest.mark.parametrize("p", [0.0, 0.1, 0.5, 0.95])
@pytest.mark.parametrize("C", [64, 128])
def test_on_off_equal(pkg, cuda, oracle, graph, switch, C, p, mode, heads):
    g, ei = graph
    h, s_src, s_dst, bias, grad, zero_rows = _inputs(cuda, heads, C, 11 * C + heads)
    if mode == 1:
        bias = None
    grads = [grad, torch.where(zero_rows[:, None], torch.zeros_like(grad), grad)]
    res = []
    for on in (True, False):
        switch(on)
        out, m, inv_l, agg, seed_buf = _forward(g, h, s_src, s_dst, bias, heads, C, mode, p, 1234)
        got = [out, m, inv_l, agg]
        for go in grads:
            nstate = _prologue(g, go, out, agg, bias, s_dst, m, inv_l, heads, C, mode)
            got += list(_edges(g, h, s_src, nstate, go, heads, C, mode, p, 1234, seed_buf))
        res.append(got)
    names = ["out", "m", "inv_l", "agg"] + [f"{n}[{z}]" for z in ("dense", "zero rows") for n in ("dh", "ds_src", "dz")]
    for name, a, b in zip(names, *res):
        assert bool(torch.isfinite(a).all()), name
        assert torch.equal(a, b), name
    if p >= 0.5:  # a destination with in-edges, every one of them dropped, is among the rows compared
        kept = _drop_mask(oracle, seed_buf, g.n_edges, p)
        alive = np.bincount(ei[1], weights=kept, minlength=N_NODES)
        assert ((alive == 0) & (np.bincount(ei[1], minlength=N_NODES) > 0)).any()


@pytest.mark.parametrize("C", [64, 128])
def test_forward_skips_dropped_rows(pkg, cuda, oracle, graph, switch, C):
    """NaN in the h rows all of whose out-edges are dropped: unread with the switch on."""
    g, ei = graph
    p = 0.5
    h, s_src, s_dst, bias, _, _ = _inputs(cuda, 1, C, 5 + C)
    switch(True)
    clean = _forward(g, h, s_src, s_dst, bias, 1, C, 0, p, 77)
    kept = _drop_mask(oracle, clean[4], g.n_edges, p)
    alive = np.bincount(ei[0], weights=kept, minlength=N_NODES)
    rows = np.flatnonzero((alive == 0) & (np.bincount(ei[0], minlength=N_NODES) > 0))
    assert len(rows) >= 50
    hp = h.clone()
    hp[torch.from_numpy(rows).to(cuda)] = float("nan")
    got = _forward(g, hp, s_src, s_dst, bias, 1, C, 0, p, 77)
    for name, a, b in zip(("out", "m", "inv_l", "agg"), got, clean):
        assert bool(torch.isfinite(a).all()), name
        assert torch.equal(a, b), name
    switch(False)
    off = _forward(g, hp, s_src, s_dst, bias, 1, C, 0, p, 77)
    assert bool(torch.isnan(off[0]).any())


@pytest.mark.parametrize("which", ["dropped", "marked"])
@pytest.mark.parametrize("C", [64, 128])
def test_backward_skips_unneeded_rows(pkg, cuda, oracle, graph, switch, C, which):
    """NaN in the grad_out rows all of whose in-edges are dropped, or whose nstate carries the
    zero-row mark (nstate from the clean grad_out): unread with the switch on."""
    g, ei = graph
    p = 0.5
    h, s_src, s_dst, bias, grad, zero_rows = _inputs(cuda, 1, C, 9 + C)
    switch(True)
    out, m, inv_l, agg, seed_buf = _forward(g, h, s_src, s_dst, bias, 1, C, 0, p, 78)
    indeg = np.bincount(ei[1], minlength=N_NODES)
    if which == "dropped":
        kept = _drop_mask(oracle, seed_buf, g.n_edges, p)
        alive = np.bincount(ei[1], weights=kept, minlength=N_NODES)
        rows = np.flatnonzero((alive == 0) & (indeg > 0))
        # 62 destinations of in-degree 1 or 2 at p = 0.5: about 30 expected
        assert len(rows) >= 10
    else:
        grad = torch.where(zero_rows[:, None], torch.zeros_like(grad), grad)
        rows = np.flatnonzero(zero_rows.cpu().numpy())
        assert (indeg[rows] > 0).sum() >= 50
    nstate = _prologue(g, grad, out, None, bias, s_dst, m, inv_l, 1, C, 0)
    if which == "marked":
        marked = nstate[:, 0, 3].view(torch.int32) == NEG_ZERO_BITS
        assert torch.equal(marked, zero_rows)
    clean = _edges(g, h, s_src, nstate, grad, 1, C, 0, p, 78, seed_buf)
    gp = grad.clone()
    gp[torch.from_numpy(rows).to(cuda)] = float("nan")
    got = _edges(g, h, s_src, nstate, gp, 1, C, 0, p, 78, seed_buf)
    for name, a, b in zip(("dh", "ds_src", "dz"), got, clean):
        assert bool(torch.isfinite(a).all()), name
        assert torch.equal(a, b), name
    switch(False)
    off = _edges(g, h, s_src, nstate, gp, 1, C, 0, p, 78, seed_buf)
    assert bool(torch.isnan(off[0]).any())


@pytest.mark.parametrize("n_users,n_items,S", [(400, 100, 300), (50, 40, 0)])
def test_bpr_producer_marks_untouched_rows(pkg, cuda, n_users, n_items, S):
    """ppgat_bpr_bwd_producer: D carries the sign-bit-only pattern exactly on the rows no triple
    names, and dZ is zero there."""
    lib, C = pkg._lib.load(), 128
    rng = np.random.default_rng(S + 3)
    u, i, j = (torch.from_numpy(rng.integers(0, n, S)).to(cuda) for n in (n_users, n_items, n_items))
    N = n_users + n_items
    Z = torch.from_numpy(rng.standard_normal((N, C)).astype(np.float32) * 0.3).to(cuda)
    b = torch.from_numpy(rng.standard_normal(C).astype(np.float32) * 0.1).to(cuda)
    sd, m, il = (torch.from_numpy(rng.standard_normal(N).astype(np.float32)).to(cuda) for _ in range(3))
    nbytes = ctypes.c_size_t(0)
    pkg._lib.check(lib.ppgat_bpr_workspace_bytes(N, S, C, ctypes.byref(nbytes)), "ws")
    st = pkg._lib.stream_handle(cuda)
    gl = torch.tensor([1.7], device=cuda)
    ws = torch.full((int(nbytes.value),), 255, dtype=torch.uint8, device=cuda)
    loss = torch.empty(1, device=cuda)
    coef = torch.empty(max(S, 1), 2, device=cuda)
    pkg._lib.check(lib.ppgat_bpr_fwd(Z.data_ptr(), N, n_users, n_items, None, C, u.data_ptr(), i.data_ptr(),
                                     j.data_ptr(), S, 0, loss.data_ptr(), coef.data_ptr(), None, ws.data_ptr(),
                                     nbytes.value, st), "fwd")
    dZ = torch.full((N, C), float("nan"), device=cuda)
    ns = torch.full((N, 4), float("nan"), device=cuda)
    db = torch.full((C,), float("nan"), device=cuda)
    pkg._lib.check(lib.ppgat_bpr_bwd_producer(
        Z.data_ptr(), N, n_users, n_items, C, u.data_ptr(), i.data_ptr(), j.data_ptr(), S, coef.data_ptr(),
        gl.data_ptr(), dZ.data_ptr(), b.data_ptr(), sd.data_ptr(), m.data_ptr(), il.data_ptr(), 1.0, ns.data_ptr(),
        db.data_ptr(), ws.data_ptr(), nbytes.value, st), "bwd_producer")
    touched = torch.zeros(N, dtype=torch.bool, device=cuda)
    touched[u] = True
    touched[n_users + i] = True
    touched[n_users + j] = True
    assert bool((~touched).any())
    marked = ns[:, 3].contiguous().view(torch.int32) == NEG_ZERO_BITS
    assert torch.equal(marked, ~touched)
    assert bool((dZ[~touched] == 0).all())


@pytest.mark.parametrize("C", [64, 128])
def test_prologue_marks_zero_rows_only(pkg, cuda, C):
    """ppgat_bwd_prologue marks exactly the all-zero grad_out rows.  (out - bias) is 0 in column 0
    and negative elsewhere (column 1 included), so an unmarked D = <g, out - bias> is -0 by accident
    both on the zero rows and on the rows g = (-1, 0, ..., 0): the latter must come out +0."""
    ops, launch, _ = _mods()
    N = 700
    gen = torch.Generator().manual_seed(C)
    bias = torch.randn(C, generator=gen) * 0.1
    out = bias[None, :] - torch.rand(N, C, generator=gen) - 0.5
    out[:, 0] = bias[0]
    grad = torch.randn(N, C, generator=gen)
    zero_rows = torch.rand(N, generator=gen) < 0.3
    grad[zero_rows] = 0.0
    trap = torch.arange(N) % 7 == 3
    grad[trap] = 0.0
    grad[trap, 0] = -1.0
    zero_rows &= ~trap
    assert int(zero_rows.sum()) >= 50 and int(trap.sum()) >= 50
    s_dst, m, inv_l = (torch.randn(N, 1, generator=gen).to(cuda) for _ in range(3))
    nstate = torch.empty(N, 1, 4, device=cuda)
    launch.bwd_prologue(0, N, grad.to(cuda), out.to(cuda), None, bias.to(cuda), s_dst, m, inv_l, 1, C, 0, nstate, None)
    D = nstate[:, 0, 3].contiguous()
    marked = (D.view(torch.int32) == NEG_ZERO_BITS).cpu()
    assert torch.equal(marked, zero_rows)
    assert bool((D.cpu()[trap] == 0).all())  # the traps do test the canonical zero
    assert torch.equal(nstate[:, 0, :3], torch.cat([s_dst, m, inv_l], 1))


def _two_layer_step(pkg, cuda, capture):
    """One BPR step of the 2-layer heads = 1 model: the loss and every parameter gradient."""
    g = pkg.data.synthetic_ui_graph(n_users=3000, n_items=800, n_interactions=40_000, seed=5)
    ei = torch.from_numpy(g.edge_index_numpy()).to(cuda)
    feats = torch.from_numpy(pkg.data.synthetic_item_features(g.n_items, 64, seed=5)).to(cuda)
    torch.manual_seed(0)
    model = pkg.PyGGAT(g.n_users, g.n_items, item_feat_dim=64, hidden=128, layers=2, heads=1,
                       attn_dropout=0.1).to(cuda).train()
    u, i, j = (torch.from_numpy(a).to(cuda) for a in pkg.data.sample_bpr_numpy(g.user_ptr, g.user_items, g.n_items,
                                                                                 2_000, seed=1))

    def step():
        model.zero_grad(set_to_none=True)
        loss = pkg.bpr_loss(model(feats, ei), g.n_users, u, i, j)
        loss.backward()
        return loss.detach()

    if not capture:
        torch.manual_seed(100)
        loss = step()
    else:
        side = torch.cuda.Stream(cuda)
        side.wait_stream(torch.cuda.current_stream(cuda))
        with torch.cuda.stream(side):
            step()
        torch.cuda.current_stream(cuda).wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        torch.manual_seed(100)  # the host seeds the capture bakes in
        with torch.cuda.graph(graph):
            loss = step()
        graph.replay()
    torch.cuda.synchronize()
    res = {n: p.grad.detach().clone() for n, p in model.named_parameters()}
    res["loss"] = loss.clone()
    return res


@pytest.mark.parametrize("capture", [False, True], ids=["eager", "graph"])
def test_two_layer_step_on_off_equal(pkg, cuda, switch, capture):
    switch(True)
    on = _two_layer_step(pkg, cuda, capture)
    switch(False)
    off = _two_layer_step(pkg, cuda, capture)
    assert set(on) == set(off) and len(on) > 4
    for k in on:
        assert bool(torch.isfinite(on[k]).all()), k
        assert torch.equal(on[k], off[k]), k
