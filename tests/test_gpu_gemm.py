"""Projection GEMMs, weight-gradient assembly and the device Adam (GPU), against fp64 torch
restatements of the same ops (GATConv.lin + node scores, its input/weight gradients,
torch.optim.Adam).  Tolerance: max-abs error / max-abs reference <= 1e-5.  The default
GEMM family is the split-bf16 matrix-core one (csrc/ppgat_split.h); test_both_gemm_families
runs the config-2 and config-5 shapes once per family (PPGAT_GEMM is read once per process)."""
import ctypes
import json
import os
import subprocess
import sys
from importlib import import_module
from pathlib import Path

import pytest
import torch

pytestmark = pytest.mark.gpu


def rel(a, b):
    a = a.detach().double().cpu(); b = b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _ops():
    return import_module("plotpointe-gat-recommendation_amd.hip_ops")


@pytest.mark.parametrize("N,K,split", [(1, 128, 1), (31, 128, 31), (32, 128, 10), (1000, 96, 1000),
                                       (255_404, 128, 192_403), (4097, 64, 0), (777, 4, 300)])
def test_project_scores_vs_fp64(pkg, cuda, N, K, split):
    ops = _ops()
    g = torch.Generator().manual_seed(N + K)
    x = torch.randn(N, K, generator=g, dtype=torch.float64)
    W = torch.randn(128, K, generator=g, dtype=torch.float64) / K ** 0.5
    a_s = torch.randn(128, generator=g, dtype=torch.float64)
    a_d = torch.randn(128, generator=g, dtype=torch.float64)
    xd = x.float().to(cuda)
    x0, x1 = (xd[:split], xd[split:]) if 0 < split < N else (xd, None)
    if split == 0:
        x0, x1 = xd[:0], xd
    h, ss, sd = ops.project(x0, W.float().to(cuda), att_src=a_s.float().to(cuda), att_dst=a_d.float().to(cuda),
                            x_items=x1)
    ref = x @ W.t()
    assert rel(h, ref) <= 1e-5
    assert rel(ss, ref @ a_s) <= 1e-5
    assert rel(sd, ref @ a_d) <= 1e-5
    h2, _, _ = ops.project(x0, W.float().to(cuda), att_src=a_s.float().to(cuda), att_dst=a_d.float().to(cuda),
                           x_items=x1)
    assert torch.equal(h, h2)


def test_project_bias(pkg, cuda):
    ops = _ops()
    g = torch.Generator().manual_seed(3)
    x = torch.randn(5000, 128, generator=g, dtype=torch.float64)
    W = torch.randn(128, 128, generator=g, dtype=torch.float64)
    b = torch.randn(128, generator=g, dtype=torch.float64)
    y = ops.project(x.float().to(cuda), W.float().to(cuda), b.float().to(cuda))
    assert rel(y, x @ W.t() + b) <= 1e-5


@pytest.mark.parametrize("N", [1, 33, 20_000, 255_404])
def test_project_bwd_input_vs_fp64(pkg, cuda, N):
    lib = pkg._lib.load()
    g = torch.Generator().manual_seed(N)
    HC, K = 128, 128
    D = torch.randn(N, HC, generator=g, dtype=torch.float64)
    S = torch.randn(N, 2, generator=g, dtype=torch.float64)
    W = torch.randn(HC, K, generator=g, dtype=torch.float64) / 11
    a_s = torch.randn(HC, generator=g, dtype=torch.float64)
    a_d = torch.randn(HC, generator=g, dtype=torch.float64)
    Dd, Sd, Wd, asd, add = (t.float().to(cuda).contiguous() for t in (D, S, W, a_s, a_d))
    dx = torch.empty(N, K, device=cuda)
    pkg._lib.check(lib.ppgat_project_bwd_input(Dd.data_ptr(), HC, N, HC, Wd.data_ptr(), K, K, asd.data_ptr(),
                                               add.data_ptr(), Sd.data_ptr(), 2, dx.data_ptr(), K,
                                               pkg._lib.stream_handle(cuda)), "project_bwd_input")
    ref = D @ W + S[:, :1] * (a_s @ W)[None] + S[:, 1:2] * (a_d @ W)[None]
    assert rel(dx, ref) <= 1e-5


@pytest.mark.parametrize("N,split,with_dx", [(1, 1, True), (31, 31, True), (33, 10, True), (8193, 0, True),
                                             (20_000, 20_000, False), (255_404, 192_403, True)])
def test_project_bwd_fused_vs_fp64(pkg, cuda, N, split, with_dx):
    """ppgat_project_bwd_fused (one pass over D and x): dx, G = D^T x and GV = S^T x against fp64,
    x in two row segments or one, tail steps, a dx-less call; bitwise reproducible."""
    lib = pkg._lib.load()
    if not lib.ppgat_project_bwd_fused_supported(128):
        pytest.skip("fused dx/dW needs the split GEMM family")
    g = torch.Generator().manual_seed(N + 7)
    HC = K = 128
    D = torch.randn(N, HC, generator=g, dtype=torch.float64)
    S = torch.randn(N, 2, generator=g, dtype=torch.float64)
    x = torch.randn(N, K, generator=g, dtype=torch.float64)
    W = torch.randn(HC, K, generator=g, dtype=torch.float64) / 11
    a_s = torch.randn(HC, generator=g, dtype=torch.float64)
    a_d = torch.randn(HC, generator=g, dtype=torch.float64)
    Dd, Sd, xd, Wd, asd, add = (t.float().to(cuda).contiguous() for t in (D, S, x, W, a_s, a_d))
    x0, x1, sp = (xd[:split].contiguous(), xd[split:].contiguous(), split) if 0 < split < N else (xd, None, N)
    nbytes = ctypes.c_size_t(0)
    pkg._lib.check(lib.ppgat_project_bwd_fused_workspace_bytes(N, ctypes.byref(nbytes)), "ws")
    ws = torch.empty(int(nbytes.value), dtype=torch.uint8, device=cuda)

    def run():
        dx = torch.full((N, K), float("nan"), device=cuda) if with_dx else None
        G = torch.empty(HC, K, device=cuda)
        GV = torch.empty(2, K, device=cuda)
        pkg._lib.check(lib.ppgat_project_bwd_fused(Dd.data_ptr(), HC, Sd.data_ptr(), 2, x0.data_ptr(), K,
                                                   x1.data_ptr() if x1 is not None else None, K, sp, N, K,
                                                   Wd.data_ptr(), K, asd.data_ptr(), add.data_ptr(),
                                                   dx.data_ptr() if dx is not None else None, K, G.data_ptr(),
                                                   GV.data_ptr(), ws.data_ptr(), nbytes.value,
                                                   pkg._lib.stream_handle(cuda)), "project_bwd_fused")
        return dx, G, GV

    dx, G, GV = run()
    if with_dx:
        ref = D @ W + S[:, :1] * (a_s @ W)[None] + S[:, 1:2] * (a_d @ W)[None]
        assert rel(dx, ref) <= 1e-5
    assert rel(G, D.t() @ x) <= 1e-5
    assert rel(GV, S.t() @ x) <= 1e-5
    dx2, G2, GV2 = run()
    assert torch.equal(G, G2) and torch.equal(GV, GV2) and (dx is None or torch.equal(dx, dx2))


@pytest.mark.parametrize("N,with_bias", [(1, True), (33, True), (8193, False), (255_404, True)])
def test_project_bwd_fused_producer(pkg, cuda, N, with_bias):
    """ppgat_project_bwd_fused_producer: dx, G, GV bit for bit those of ppgat_project_bwd_fused,
    plus the producer layer's prologue from dx -- nstate = {s_dst, m, inv_l, <dx, x - b>} and
    dbias = sum_r dx_r -- against fp64 (and the fp32 ppgat_bwd_prologue within 1e-5)."""
    lib = pkg._lib.load()
    if not lib.ppgat_project_bwd_fused_supported(128):
        pytest.skip("fused dx/dW needs the split GEMM family")
    g = torch.Generator().manual_seed(N + 3)
    HC = K = 128
    D = torch.randn(N, HC, generator=g, dtype=torch.float64)
    S = torch.randn(N, 2, generator=g, dtype=torch.float64)
    x = torch.randn(N, K, generator=g, dtype=torch.float64)
    W = torch.randn(HC, K, generator=g, dtype=torch.float64) / 11
    a_s, a_d, b = (torch.randn(HC, generator=g, dtype=torch.float64) for _ in range(3))
    sd, m, il = (torch.randn(N, generator=g, dtype=torch.float64) for _ in range(3))
    Dd, Sd, xd, Wd, asd, add, bd, sdd, md, ild = (t.float().to(cuda).contiguous()
                                                  for t in (D, S, x, W, a_s, a_d, b, sd, m, il))
    nbytes = ctypes.c_size_t(0)
    pkg._lib.check(lib.ppgat_project_bwd_fused_workspace_bytes(N, ctypes.byref(nbytes)), "ws")
    ws = torch.empty(int(nbytes.value), dtype=torch.uint8, device=cuda)
    st = pkg._lib.stream_handle(cuda)
    outs = []
    for producer in (False, True):
        dx = torch.full((N, K), float("nan"), device=cuda)
        G, GV = torch.empty(HC, K, device=cuda), torch.empty(2, K, device=cuda)
        ns = torch.full((N, 4), float("nan"), device=cuda)
        db = torch.full((K,), float("nan"), device=cuda)
        common = (Dd.data_ptr(), HC, Sd.data_ptr(), 2, xd.data_ptr(), K, None, K, N, N, K, Wd.data_ptr(), K,
                  asd.data_ptr(), add.data_ptr(), dx.data_ptr(), K, G.data_ptr(), GV.data_ptr())
        if producer:
            pkg._lib.check(lib.ppgat_project_bwd_fused_producer(
                *common, bd.data_ptr() if with_bias else None, sdd.data_ptr(), md.data_ptr(), ild.data_ptr(), 1.0,
                ns.data_ptr(), db.data_ptr() if with_bias else None, ws.data_ptr(), nbytes.value, st), "producer")
        else:
            pkg._lib.check(lib.ppgat_project_bwd_fused(*common, ws.data_ptr(), nbytes.value, st), "fused")
        outs.append((dx, G, GV, ns, db))
    (dx0, G0, GV0, _, _), (dx1, G1, GV1, ns, db) = outs
    assert torch.equal(dx0, dx1) and torch.equal(G0, G1) and torch.equal(GV0, GV1)
    dx64 = dx1.double().cpu()
    xb = x - (b if with_bias else 0.0)
    Dref = (dx64 * xb).sum(1)
    scale = (dx64.abs() * xb.abs()).sum(1).clamp_min(1e-30)   # pre-cancellation size of each row's dot
    assert float(((ns[:, 3].double().cpu() - Dref).abs() / scale).max()) <= 1e-6
    assert torch.equal(ns[:, :3].cpu(), torch.stack([sdd, md, ild], 1).cpu())
    if with_bias:
        assert rel(db, dx64.sum(0)) <= 1e-5
    # the separate prologue on the same dx (ppgat_bwd_prologue) agrees to fp32 rounding
    ns2 = torch.empty(N, 4, device=cuda)
    db2 = torch.empty(K, device=cuda)
    part = torch.empty(max(int(lib.ppgat_bwd_partial_rows(N)), 1) * K, device=cuda)
    out = xd  # x IS the producer's output (bias included)
    pkg._lib.check(lib.ppgat_bwd_prologue(dx1.data_ptr(), out.data_ptr(), None, bd.data_ptr() if with_bias else None,
                                          sdd.data_ptr(), md.data_ptr(), ild.data_ptr(), N, 1, K, 0, ns2.data_ptr(),
                                          db2.data_ptr() if with_bias else None, part.data_ptr() if with_bias else None,
                                          st), "bwd_prologue")
    assert float(((ns2[:, 3].double().cpu() - ns[:, 3].double().cpu()).abs() / scale).max()) <= 1e-5
    if with_bias:
        assert rel(db, db2.double()) <= 1e-5


def test_producer_prologue_in_the_model(pkg, cuda, monkeypatch):
    """Two stacked heads = 1 layers: layer 1's backward prologue runs inside layer 2's dx kernel
    and layer 2's inside the loss backward (two hand-offs per backward, no ppgat_bwd_prologue
    call), and every gradient matches the unfused path within 1e-5."""
    from importlib import import_module
    ops = import_module("plotpointe-gat-recommendation_amd.hip_ops")
    gr = pkg.data.synthetic_ui_graph(n_users=3000, n_items=800, n_interactions=40_000, seed=5)
    ei = torch.from_numpy(gr.edge_index_numpy()).to(cuda)
    feats = torch.from_numpy(pkg.data.synthetic_item_features(gr.n_items, 64, seed=5)).to(cuda)
    u, i, j = (torch.from_numpy(a).to(cuda) for a in pkg.data.sample_bpr_numpy(gr.user_ptr, gr.user_items,
                                                                                 gr.n_items, 20_000, seed=1))
    calls = {"n": 0}
    real = ops._producer_of

    def counting(x, N, C=128):
        r = real(x, N, C)
        calls["n"] += r is not None
        return r
    # GATLayer.forward (ops_gat) and the loss forward (ops_loss) each look the name up in their own module
    for mod in ("ops_gat", "ops_loss"):
        monkeypatch.setattr(import_module("plotpointe-gat-recommendation_amd." + mod), "_producer_of", counting)
    lib = pkg._lib.load()
    real_pro = lib.ppgat_bwd_prologue
    pro_calls = {"n": 0}

    def counting_pro(*a):
        pro_calls["n"] += 1
        return real_pro(*a)
    monkeypatch.setattr(lib, "ppgat_bwd_prologue", counting_pro)
    grads, pros = [], []
    for flag in ("1", "0"):
        pro_calls["n"] = 0
        monkeypatch.setenv("PPGAT_PRODUCER_PROLOGUE", flag)
        torch.manual_seed(0)
        model = pkg.PyGGAT(gr.n_users, gr.n_items, item_feat_dim=64, hidden=128, layers=2, heads=1,
                           attn_dropout=0.1).to(cuda).train()
        torch.manual_seed(100)
        pkg.bpr_loss(model(feats, ei), gr.n_users, u, i, j).backward()
        grads.append({n: p.grad.detach().clone() for n, p in model.named_parameters()})
        pros.append(pro_calls["n"])
    assert calls["n"] == 2 and pros == [0, 2]
    for n in grads[0]:
        assert rel(grads[0][n], grads[1][n].double()) <= 1e-5, n


def test_producer_prologue_partial_grad_then_backward(pkg, cuda):
    """A partial autograd.grad over the consumer layer leaves a hand-off on the producer that its
    backward never took; a later backward into the producer from another root (a gradient the
    allocator may place at the dead dx's address, version 0) must not use that stale state."""
    gr = pkg.data.synthetic_ui_graph(n_users=2000, n_items=600, n_interactions=30_000, seed=9)
    ei = torch.from_numpy(gr.edge_index_numpy()).to(cuda)
    N = gr.n_nodes
    torch.manual_seed(3)
    c1 = pkg.GATConv(128, 128, heads=1, dropout=0.0, add_self_loops=False, concat=False).to(cuda)
    c2 = pkg.GATConv(128, 128, heads=1, dropout=0.0, add_self_loops=False, concat=False).to(cuda)
    x = torch.randn(N, 128, device=cuda)
    out1 = c1(x, ei)
    loss = c2(out1, ei).square().sum()
    torch.autograd.grad(loss, [c2.lin.weight], retain_graph=True)   # c1's backward does not run
    g1 = torch.randn_like(out1)                                      # likely the dead dx's block
    out1.backward(g1)
    got = {n: p.grad.detach().clone() for n, p in c1.named_parameters()}
    for p in c1.parameters():
        p.grad = None
    c1(x, ei).backward(g1)                                           # no consumer: no hand-off
    for n, p in c1.named_parameters():
        assert rel(got[n], p.grad.double()) <= 1e-6, n


def test_node_table_second_forward_is_caught(pkg, cuda):
    """The node table's item rows are rewritten by every forward (a raw-pointer write): a graph
    that saved the previous rows must fail autograd's version check, not silently use new rows."""
    gr = pkg.data.synthetic_ui_graph(n_users=1500, n_items=400, n_interactions=20_000, seed=4)
    ei = torch.from_numpy(gr.edge_index_numpy()).to(cuda)
    feats = torch.from_numpy(pkg.data.synthetic_item_features(gr.n_items, 64, seed=4)).to(cuda)
    torch.manual_seed(0)
    model = pkg.PyGGAT(gr.n_users, gr.n_items, item_feat_dim=64, hidden=128, layers=2, heads=1,
                       attn_dropout=0.0).to(cuda).train()
    first = model(feats, ei).square().sum()
    model(feats * 2, ei)                      # a second forward before the first backward
    with pytest.raises(RuntimeError, match="rewritten by a later forward"):
        first.backward()


def test_gemm_tn_segments(pkg, cuda):
    ops = _ops()
    g = torch.Generator().manual_seed(11)
    N, split = 130_001, 100_000  # >= 1e5 rows: both calls take the register-accumulator kernel
    A = torch.randn(N, 132, generator=g, dtype=torch.float64)
    B = torch.randn(N, 128, generator=g, dtype=torch.float64)
    Ad, Bd = A.float().to(cuda), B.float().to(cuda)
    out, cs, vo = ops.gemm_tn(Ad[:, :128], Bd[:split], want_colsum=True, V=Ad[:, 128:130], B_items=Bd[split:])
    assert rel(out, A[:, :128].t() @ B) <= 1e-5
    assert rel(cs, A[:, :128].sum(0)) <= 1e-5
    assert rel(vo, A[:, 128:130].t() @ B) <= 1e-5
    out1, _, vo1 = ops.gemm_tn(Ad[:, :128], Bd, V=Ad[:, 128:130])
    assert torch.equal(out, out1) and torch.equal(vo, vo1)


def test_gemm_tn_empty_operands(pkg, cuda):
    """Zero-width operands (an empty product) and zero rows (an empty reduction) give zeros of
    the right shape -- no recursion through the unaligned-row padding."""
    ops = _ops()
    A = torch.randn(1000, 8, device=cuda)
    for a, b, shape in ((A[:, :0], A, (0, 8)), (A, A[:, :0], (8, 0)), (A[:0], A[:0], (8, 8))):
        out, cs, vo = ops.gemm_tn(a, b, want_colsum=True, V=A[: a.size(0), :2])
        assert out.shape == shape and not out.any()
        assert cs.shape == (shape[0],) and not cs.any()
        assert vo.shape == (2, shape[1]) and not vo.any()


@pytest.mark.parametrize("heads,C,K", [(1, 128, 128), (2, 64, 96), (4, 32, 128)])
def test_weight_grads_vs_fp64(pkg, cuda, heads, C, K):
    ops = _ops()
    g = torch.Generator().manual_seed(heads)
    HC = heads * C
    G = torch.randn(HC, K, generator=g, dtype=torch.float64)
    GV = torch.randn(2 * heads, K, generator=g, dtype=torch.float64)
    W = torch.randn(HC, K, generator=g, dtype=torch.float64)
    a_s = torch.randn(heads, C, generator=g, dtype=torch.float64)
    a_d = torch.randn(heads, C, generator=g, dtype=torch.float64)
    dW, ds, dd = ops.weight_grads(*(t.float().to(cuda).contiguous() for t in (G, GV, W, a_s, a_d)), heads, C)
    Wv = W.view(heads, C, K)
    ref = (G.view(heads, C, K) + a_s[..., None] * GV[:heads, None, :] + a_d[..., None] * GV[heads:, None, :]).view(HC, K)
    assert rel(dW, ref) <= 1e-5
    assert rel(ds, torch.einsum("hck,hk->hc", Wv, GV[:heads])) <= 1e-5
    assert rel(dd, torch.einsum("hck,hk->hc", Wv, GV[heads:])) <= 1e-5


def test_adam_matches_torch(pkg, cuda):
    """ppgat_amd.optim.Adam == torch.optim.Adam (same hyper-parameters, L2 weight decay) over
    5 steps on 20 tensors (more than one launch), incl. sizes that are not multiples of 4."""
    g = torch.Generator().manual_seed(5)
    shapes = [(192_403, 128), (128, 128), (128,), (1, 1, 128), (7,), (1,), (1001, 3)] + [(33, 5)] * 13
    ref = [torch.randn(*s, generator=g).to(cuda).requires_grad_(True) for s in shapes]
    mine = [p.detach().clone().requires_grad_(True) for p in ref]
    o_ref = torch.optim.Adam(ref, lr=1e-3, weight_decay=1e-4)
    o_mine = pkg.optim.Adam(mine, lr=1e-3, weight_decay=1e-4)
    for step in range(5):
        grads = [torch.randn(*s, generator=g).to(cuda) for s in shapes]
        for p, q, gr in zip(ref, mine, grads):
            p.grad = gr.clone()
            q.grad = gr.clone()
        o_ref.step()
        o_mine.step()
    for p, q in zip(ref, mine):
        assert rel(q, p) <= 1e-6
        assert rel(o_mine.state[q]["exp_avg_sq"], o_ref.state[p]["exp_avg_sq"]) <= 1e-6
    assert float(o_mine.state[mine[0]]["step"]) == 5.0
    # state_dict round-trips into torch's Adam
    o2 = torch.optim.Adam(mine, lr=1e-3, weight_decay=1e-4)
    o2.load_state_dict(o_mine.state_dict())


def test_fused_layer_equals_unfused(pkg, cuda):
    """GATConv through the fused projection/dx kernels vs the same layer forced through the
    library GEMM path (x_items split vs one tensor as well): forward and all gradients."""
    ops = _ops()
    g = torch.Generator().manual_seed(0)
    N, E = 3000, 30_000
    ei = torch.stack([torch.randint(0, N, (E,), generator=g), torch.randint(0, N, (E,), generator=g)]).to(cuda)
    torch.manual_seed(1)
    conv = pkg.GATConv(128, 128, heads=1, dropout=0.0, add_self_loops=False, concat=False).to(cuda)
    with torch.no_grad():
        conv.bias.uniform_(-0.1, 0.1)
    x = torch.randn(N, 128, generator=g).to(cuda).requires_grad_(True)
    up = torch.randn(N, 128, generator=g).to(cuda)
    out_a = conv.forward_segments(x[:1000], x[1000:], ei)
    (out_a * up).sum().backward()
    ga = [x.grad.clone()] + [p.grad.clone() for p in conv.parameters()]
    x.grad = None
    conv.zero_grad()
    ops_gat = import_module("plotpointe-gat-recommendation_amd.ops_gat")  # where GATLayer looks it up
    orig = ops_gat.project_supported
    try:
        ops_gat.project_supported = lambda k, c: False
        out_b = conv(x, ei)
        (out_b * up).sum().backward()
    finally:
        ops_gat.project_supported = orig
    gb = [x.grad.clone()] + [p.grad.clone() for p in conv.parameters()]
    assert rel(out_a, out_b) <= 1e-5
    for a, b in zip(ga, gb):
        assert rel(a, b) <= 1e-4


def test_gemm_tn_large_shape_deterministic(pkg, cuda):
    """Beyond one 128 x 128 tile gemm_tn goes through the matrix-core TN kernel
    (ppgat_gemm_tn_big) with column-sliced operands: fp32-accurate and bitwise reproducible
    run to run (config 5's 1024 x 256 weight gradient, scaled down)."""
    ops = _ops()
    g = torch.Generator().manual_seed(21)
    N = 100_000
    A = torch.randn(N, 1032, generator=g, dtype=torch.float64)
    B = torch.randn(N, 256, generator=g, dtype=torch.float64)
    Ad, Bd = A.float().to(cuda), B.float().to(cuda)
    out, cs, vo = ops.gemm_tn(Ad[:, :1024], Bd, want_colsum=True, V=Ad[:, 1024:1032])
    assert rel(out, A[:, :1024].t() @ B) <= 1e-5
    assert rel(cs, A[:, :1024].sum(0)) <= 1e-5
    assert rel(vo, A[:, 1024:1032].t() @ B) <= 1e-5
    out2, cs2, vo2 = ops.gemm_tn(Ad[:, :1024], Bd, want_colsum=True, V=Ad[:, 1024:1032])
    assert torch.equal(out, out2) and torch.equal(cs, cs2) and torch.equal(vo, vo2)


@pytest.mark.parametrize("family,f16", [("split", "1"), ("split", "0"), ("fp32", "1")])
def test_both_gemm_families(cuda, family, f16):
    """Projection (x W^T + scores, + bias), dx and weight-gradient GEMMs at config-2 rows, and
    the config-5 NN shapes, in a fresh process per family (split: the large-M NN products on the
    fp16 two-term kernel, or with PPGAT_GEMM_F16=0 -- a lab-build switch -- on the bf16 x6 one; fp32 MFMA): all within
    2e-6 of fp64 (tighter than the suite's 1e-5), bitwise repeatable, the two B layouts of the
    NN GEMM identical."""
    root = Path(__file__).resolve().parents[1]
    env = dict(os.environ, PPGAT_GEMM=family, PPGAT_GEMM_F16=f16)
    if f16 == "0":  # the bf16 x6 pre-split NN kernel is a lab-build kernel now
        lab = root / "lab_build" / "libppgat.so"
        if not lab.exists():
            pytest.skip("lab build absent (make -C plotpointe-gat-recommendation_amd/csrc lab)")
        env["PPGAT_LIB"] = str(lab)
    res = {}
    for extra in ([], ["--cfg5"]):
        out = subprocess.run([sys.executable, str(root / "tools" / "gemm_split_check.py"), "--iters", "3"] + extra,
                             env=env, capture_output=True, text=True, timeout=300, cwd=str(root))
        assert out.returncode == 0, out.stderr[-2000:]
        res.update(json.loads(out.stdout.strip().splitlines()[-1]))
    assert res["mode"] == family
    for k, v in res.items():
        if k.endswith("_err"):
            assert v <= (5e-6 if k == "tn_big_err" else 2e-6), (k, v)
    assert res["fwd_bitwise_repeat"]
    assert res["out_1024x256_layouts_equal"] and res["gt_256x1024_layouts_equal"]
