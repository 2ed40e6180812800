"""The matrix-core GEMMs (ppgat_gemm_nn / ppgat_gemm_tn_big / ppgat_colsum) and the
multi-head aggregate-then-transform layer (ppgat_xgat_*) against the fp64 CPU oracle (GPU).

Tolerances: max-abs error / max-abs oracle value, 1e-5 for outputs and matrices (exact fp32
FMA chains on both sides of each reduction, different orders), 1e-4 for attention-vector and
bias gradients (sums over every edge / node with cancellation)."""
import importlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def rel(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _ops():
    return importlib.import_module("plotpointe-gat-recommendation_amd.hip_ops")


def _ops_gemm():  # the module that holds _CONST_BOUNDS
    return importlib.import_module("plotpointe-gat-recommendation_amd.ops_gemm")


def _ops_xgat():  # the module whose code looks up _xgat_weight_grads
    return importlib.import_module("plotpointe-gat-recommendation_amd.ops_xgat")


@pytest.mark.parametrize("M,K,N,layout", [(1000, 256, 256, 1), (3001, 1024, 256, 0), (777, 256, 1024, 0),
                                          (130, 32, 128, 1), (5000, 256, 384, 0)])
def test_gemm_nn_vs_fp64(cuda, M, K, N, layout):
    ops = _ops()
    g = torch.Generator().manual_seed(M + K + N)
    x = torch.randn(M, K, generator=g, dtype=torch.float64)
    B = torch.randn(K, N, generator=g, dtype=torch.float64) if layout == 0 else \
        torch.randn(N, K, generator=g, dtype=torch.float64)
    bias = torch.randn(N, generator=g, dtype=torch.float64)
    ref = 0.5 * (x @ (B if layout == 0 else B.t())) + bias
    y = ops.gemm_nn(x.float().to(cuda), B.float().to(cuda), layout, N, alpha=0.5, bias=bias.float().to(cuda))
    assert rel(y, ref) <= 1e-5
    y2 = ops.gemm_nn(x.float().to(cuda), B.float().to(cuda), layout, N, alpha=0.5, bias=bias.float().to(cuda))
    assert torch.equal(y, y2)


@pytest.mark.parametrize("M,K,N,layout", [(512, 896, 256, 1), (44, 896, 256, 1), (512, 128, 256, 0), (300, 512, 128, 1),
                                          (1, 384, 128, 1), (1000, 1024, 512, 0)])
def test_gemm_nn_split_k_vs_fp64(cuda, M, K, N, layout):
    """Small M with a long reduction (the FusionMLP batch: 512 x 896 -> 256): ppgat_gemm_nn_ws
    splits k over workgroups into the workspace and sums the splits in order; equals the
    unsplit kernel to 1e-5 relative, the fp64 product to 1e-5, and is bitwise repeatable."""
    import ctypes
    ops = _ops()
    lib = __import__("importlib").import_module("plotpointe-gat-recommendation_amd._lib").load()
    nbytes = ctypes.c_size_t(0)
    assert lib.ppgat_gemm_nn_workspace_bytes(M, K, N, ctypes.byref(nbytes)) == 0
    if M * N <= 512 * 256 and K >= 256:
        assert nbytes.value > 0  # the split path is taken
    g = torch.Generator().manual_seed(M * 7 + K)
    x = torch.randn(M, K, generator=g, dtype=torch.float64)
    B = torch.randn(K, N, generator=g, dtype=torch.float64) if layout == 0 else \
        torch.randn(N, K, generator=g, dtype=torch.float64)
    bias = torch.randn(N, generator=g, dtype=torch.float64)
    ref = 0.25 * (x @ (B if layout == 0 else B.t())) + bias
    xs, Bs, bs = x.float().to(cuda), B.float().to(cuda), bias.float().to(cuda)
    y = ops.gemm_nn(xs, Bs, layout, N, alpha=0.25, bias=bs)
    assert rel(y, ref) <= 1e-5
    assert torch.equal(y, ops.gemm_nn(xs, Bs, layout, N, alpha=0.25, bias=bs))
    y1 = torch.empty(M, N, device=cuda)  # the unsplit kernel (no workspace) on the same operands
    pkg_lib = __import__("importlib").import_module("plotpointe-gat-recommendation_amd._lib")
    pkg_lib.check(lib.ppgat_gemm_nn(xs.data_ptr(), K if M == 1 else xs.stride(0), M, K, Bs.data_ptr(), Bs.stride(0),
                                    layout, N, 0.25, bs.data_ptr(), y1.data_ptr(), N, pkg_lib.stream_handle(cuda)),
                  "gemm_nn")
    assert rel(y, y1.double()) <= 1e-5


@pytest.mark.parametrize("M,Ma,Nb", [(5000, 256, 1024), (100_003, 256, 256), (77, 128, 128), (0, 128, 256)])
def test_gemm_tn_big_and_colsum_vs_fp64(cuda, M, Ma, Nb):
    ops = _ops()
    g = torch.Generator().manual_seed(M + Ma)
    A = torch.randn(M, Ma, generator=g, dtype=torch.float64)
    B = torch.randn(M, Nb, generator=g, dtype=torch.float64)
    out = ops.gemm_tn_big(A.float().to(cuda), B.float().to(cuda))
    ref = A.t() @ B
    if M == 0:
        assert torch.equal(out.cpu(), torch.zeros(Ma, Nb))
        return
    assert rel(out, ref) <= 1e-5
    assert torch.equal(out, ops.gemm_tn_big(A.float().to(cuda), B.float().to(cuda)))
    if Ma in (128, 256):
        assert rel(ops.colsum(A.float().to(cuda)), A.sum(0)) <= 1e-5


def _graph(rng, n, e, hub_rows=0):
    src = rng.integers(0, n, e)
    dst = rng.integers(0, n, e)
    if hub_rows:  # a few destinations and sources with > 256 edges: hub pieces in both passes
        k = e // 5
        dst[:k] = rng.integers(0, hub_rows, k)
        src[k:2 * k] = rng.integers(0, hub_rows, k)
    return np.stack([src, dst]).astype(np.int64)


@pytest.mark.parametrize("gather", ["gd", "gd-free", "g", "gt"])
@pytest.mark.parametrize("n,e,C,heads,p,hubs", [(2000, 20_000, 256, 4, 0.0, 0), (1500, 30_000, 256, 4, 0.2, 3),
                                                (1200, 12_000, 128, 2, 0.1, 0), (900, 25_000, 256, 2, 0.0, 2),
                                                (1500, 60_000, 256, 4, 0.1, 1),  # 47-piece hubs: workgroup merges
                                                # hubs of 16 / 17 pieces: either side of the one-wave merges' limit
                                                (1500, 20_400, 256, 4, 0.1, 1), (1500, 20_600, 256, 4, 0.0, 1)])
def test_gatconv_aggregate_then_transform_vs_oracle(pkg, oracle, cuda, monkeypatch, n, e, C, heads, p, hubs, gather):
    """Both backward edge passes: gathering g_i (hs = x W^T / H per source, acc, dx = acc W / H;
    ppgat_xgat_bwd_edges_g, C == 256) and gathering gt_i (ppgat_xgat_bwd_edges).  "gd-free": the
    default pass without the forward's aggregates kept -- the weight gradient as acc^T x
    (hip_ops._xgat_keep_agg, the whole 200M-edge graph on one GPU)."""
    monkeypatch.setenv("PPGAT_XGAT_GATHER", gather.split("-")[0])
    monkeypatch.setenv("PPGAT_XGAT_AGG", "free" if gather.endswith("free") else "keep")
    ops = _ops()
    assert ops.xgat_supported(256, heads, C)
    rng = np.random.default_rng(n + heads)
    ei = _graph(rng, n, e, hubs)
    torch.manual_seed(3)
    conv = pkg.GATConv(256, C, heads=heads, dropout=p, add_self_loops=False, concat=False)
    with torch.no_grad():
        conv.bias.uniform_(-0.1, 0.1)
    conv = conv.to(cuda).train(p > 0)
    x64 = torch.from_numpy(rng.standard_normal((n, 256)))
    G64 = torch.from_numpy(rng.standard_normal((n, C)))
    cm = importlib.import_module("plotpointe-gat-recommendation_amd.conv")
    orig = cm._dropout_seed
    cm._dropout_seed = lambda: 55555
    try:
        x = x64.float().to(cuda).requires_grad_(True)
        out = conv(x, torch.from_numpy(ei).to(cuda))
        (out * G64.float().to(cuda)).sum().backward()
    finally:
        cm._dropout_seed = orig
    P = {k: v.detach().double().cpu().requires_grad_(True) for k, v in conv.named_parameters()}
    xr = x64.clone().requires_grad_(True)
    ref = oracle.pyg_gat_conv(xr, torch.from_numpy(ei), P["lin.weight"], P["att_src"], P["att_dst"], P["bias"],
                              heads, dropout_p=p, seed=55555)
    (ref * G64).sum().backward()
    assert rel(out, ref) <= 1e-5
    assert rel(x.grad, xr.grad) <= 1e-5
    assert rel(conv.lin.weight.grad, P["lin.weight"].grad) <= 1e-5
    assert rel(conv.bias.grad, P["bias"].grad) <= 1e-4
    assert rel(conv.att_src.grad, P["att_src"].grad) <= 1e-4
    assert rel(conv.att_dst.grad, P["att_dst"].grad) <= 1e-4


def test_linear_256_on_matrix_cores(pkg, cuda):
    """item_proj at config 5 (Linear 256 -> 256 + bias) through ppgat_gemm_nn / gemm_tn_big."""
    ops = _ops()
    g = torch.Generator().manual_seed(0)
    x = torch.randn(20_000, 256, generator=g, dtype=torch.float64)
    W = torch.randn(256, 256, generator=g, dtype=torch.float64) * 0.05
    b = torch.randn(256, generator=g, dtype=torch.float64)
    G = torch.randn(20_000, 256, generator=g, dtype=torch.float64)
    xd = x.float().to(cuda).requires_grad_(True)
    Wd = W.float().to(cuda).requires_grad_(True)
    bd = b.float().to(cuda).requires_grad_(True)
    y = ops.linear(xd, Wd, bd)
    (y * G.float().to(cuda)).sum().backward()
    xr, Wr, br = (t.clone().requires_grad_(True) for t in (x, W, b))
    yr = xr @ Wr.t() + br
    (yr * G).sum().backward()
    assert rel(y, yr) <= 1e-5
    assert rel(xd.grad, xr.grad) <= 1e-5
    assert rel(Wd.grad, Wr.grad) <= 1e-5
    assert rel(bd.grad, br.grad) <= 1e-5


def test_weight_grad_bound_ignores_rows_without_out_edges(pkg, oracle, cuda):
    """the fp16 weight-gradient G = g^T agg takes agg's column bound from the column
    maxima of x; the fp16 split's error is relative to that bound.  Ten rows of x 1e4 times
    larger than the rest that are nobody's source (no out-edge) never enter an aggregate: the
    bound comes from the source rows only (ppgat_colmax_abs_sources), so dW stays within 1e-5 of
    the fp64 oracle.  (The rows are isolated -- no in-edges either: as destinations their 1e4
    larger attention terms would swamp the per-edge logits' fp32 resolution, an fp32 property
    of any implementation.)  70,000 rows: the fp16 TN kernel's range (>= 64k rows).  Both bounds
    come from the edge passes (the rows they gather: every source / every destination with an
    edge) and equal those sets' exact maxima; the isolated rows' g is 1e6 larger as well -- outside
    the g bound, clamped in the split, adding the 0 their empty aggregates give."""
    rng = np.random.default_rng(11)
    n, e, heads, C = 70_000, 500_000, 4, 256
    out_rows = np.arange(n - 10, n)
    ei = np.stack([rng.integers(0, n - 10, e), rng.integers(0, n - 10, e)]).astype(np.int64)  # n-10.. isolated
    torch.manual_seed(5)
    conv = pkg.GATConv(256, C, heads=heads, dropout=0.0, add_self_loops=False, concat=False).to(cuda)
    x64 = torch.from_numpy(rng.standard_normal((n, 256)))
    x64[out_rows] *= 1e4
    G64 = torch.from_numpy(rng.standard_normal((n, C)))
    G64[out_rows] *= 1e6  # their g rows too: no in-edge, so outside the gathered bound of g (clamped, adding 0)
    x = x64.float().to(cuda).requires_grad_(True)
    ops = _ops()
    seen = {}
    real = ops._xgat_weight_grads

    def spy(*a, **k):
        seen.update(k)
        seen["xbits"] = a[1].get("xbits")
        return real(*a, **k)
    import pytest as _pt
    mp = _pt.MonkeyPatch()
    mp.setattr(_ops_xgat(), "_xgat_weight_grads", spy)
    try:
        out = conv(x, torch.from_numpy(ei).to(cuda))
        (out * G64.float().to(cuda)).sum().backward()
    finally:
        mp.undo()
    # the bounds the weight gradient used came from the edge passes, and equal the exact sets' maxima
    src_rows = np.unique(ei[0])
    dst_rows = np.unique(ei[1])
    xb = torch.from_numpy(np.abs(x64.float().numpy()[src_rows]).max(0)).view(torch.int32)
    gb = torch.from_numpy(np.abs(G64.float().numpy()[dst_rows]).max(0)).view(torch.int32)
    assert seen.get("gbits") is not None and torch.equal(seen["gbits"].cpu(), gb)
    assert seen.get("xbits") is not None and torch.equal(seen["xbits"].cpu(), xb)
    assert not torch.equal(ops.colmax_abs(x.detach()).cpu(), xb)  # (the isolated rows set the all-rows maxima)
    P = {k: v.detach().double().requires_grad_(True) for k, v in conv.named_parameters()}
    xr = x64.to(cuda).requires_grad_(True)
    ref = oracle.pyg_gat_conv(xr, torch.from_numpy(ei).to(cuda), P["lin.weight"], P["att_src"], P["att_dst"],
                              P["bias"], heads)
    (ref * G64.to(cuda)).sum().backward()
    assert rel(out, ref) <= 1e-5
    assert rel(conv.lin.weight.grad, P["lin.weight"].grad) <= 1e-5, rel(conv.lin.weight.grad, P["lin.weight"].grad)
    assert rel(x.grad, xr.grad) <= 1e-5


def test_linear_constant_input_bound_cached(pkg, cuda):
    """item_proj's weight gradient on the fp16 TN kernel (>= 64k rows) with the item features as a
    constant input: their column bound is computed once (hip_ops._const_colmax) and reused while
    the tensor is unchanged; dW within 1e-5 of fp64 both times, recomputed after an in-place change."""
    ops = _ops()
    g = torch.Generator().manual_seed(1)
    n = 70_000
    x = torch.randn(n, 256, generator=g, dtype=torch.float64)
    W = torch.randn(256, 256, generator=g, dtype=torch.float64) * 0.05
    b = torch.randn(256, generator=g, dtype=torch.float64)
    G = torch.randn(n, 256, generator=g, dtype=torch.float64)
    xd = x.float().to(cuda)                       # no grad: a constant input
    ref = G.t() @ x
    for it in range(3):
        Wd = W.float().to(cuda).requires_grad_(True)
        bd = b.float().to(cuda).requires_grad_(True)
        (ops.linear(xd, Wd, bd) * G.float().to(cuda)).sum().backward()
        assert rel(Wd.grad, ref) <= 1e-5
        e = _ops_gemm()._CONST_BOUNDS.get(id(xd))
        assert e is not None and e[0]() is xd and e[1][0] == xd._version and e[1][1] == xd.data_ptr()
        if it == 1:
            xd.mul_(2.0)                          # a new version: the bound is recomputed
            x = x * 2.0
            ref = G.t() @ x


def test_agg_free_weight_grad_fp16_path(pkg, oracle, cuda, monkeypatch):
    """The weight gradient without the forward's aggregates (PPGAT_XGAT_AGG=free, the form the
    whole 200M-edge graph takes on one GPU): G = (acc^T x) permuted on the fp16 TN kernel (>= 64k
    rows), acc's column maxima exact, x's over every row.  dW, dx, datt within the usual bounds
    of the fp64 oracle, and dW within 1e-5 of the default (agg kept) form."""
    rng = np.random.default_rng(12)
    n, e, heads, C = 70_000, 600_000, 4, 256
    ei = np.stack([rng.integers(0, n, e), rng.integers(0, n, e)]).astype(np.int64)
    torch.manual_seed(6)
    conv = pkg.GATConv(256, C, heads=heads, dropout=0.1, add_self_loops=False, concat=False)
    with torch.no_grad():
        conv.bias.uniform_(-0.1, 0.1)
    conv = conv.to(cuda).train()
    x64 = torch.from_numpy(rng.standard_normal((n, 256)))
    G64 = torch.from_numpy(rng.standard_normal((n, C)))
    cm = importlib.import_module("plotpointe-gat-recommendation_amd.conv")
    orig = cm._dropout_seed
    cm._dropout_seed = lambda: 777
    grads = {}
    try:
        for mode in ("keep", "free"):
            monkeypatch.setenv("PPGAT_XGAT_AGG", mode)
            conv.zero_grad(set_to_none=True)
            x = x64.float().to(cuda).requires_grad_(True)
            out = conv(x, torch.from_numpy(ei).to(cuda))
            (out * G64.float().to(cuda)).sum().backward()
            grads[mode] = {"dx": x.grad.clone(), **{k: v.grad.clone() for k, v in conv.named_parameters()}}
    finally:
        cm._dropout_seed = orig
    P = {k: v.detach().double().requires_grad_(True) for k, v in conv.named_parameters()}
    xr = x64.to(cuda).requires_grad_(True)
    ref = oracle.pyg_gat_conv(xr, torch.from_numpy(ei).to(cuda), P["lin.weight"], P["att_src"], P["att_dst"],
                              P["bias"], heads, dropout_p=0.1, seed=777)
    (ref * G64.to(cuda)).sum().backward()
    f = grads["free"]
    assert rel(f["lin.weight"], P["lin.weight"].grad) <= 1e-5
    assert rel(f["lin.weight"], grads["keep"]["lin.weight"].double()) <= 1e-5
    assert rel(f["dx"], xr.grad) <= 1e-5
    assert torch.equal(f["dx"], grads["keep"]["dx"])          # dx does not involve the weight-gradient form
    assert rel(f["att_src"], P["att_src"].grad) <= 1e-4 and rel(f["att_dst"], P["att_dst"].grad) <= 1e-4
    assert rel(f["bias"], P["bias"].grad) <= 1e-4


def test_node_table_joins_rows_without_a_copy(pkg, cuda, monkeypatch):
    """model.node_table: the user embedding's storage is the first rows of one table and the item
    projection writes the rest, so the aggregate-then-transform first layer gets cat(users, items)
    as a new header on that storage (hip_ops.join_rows) instead of a 1-KB-per-row copy.  Forward
    and every gradient bitwise those of the layers run on a materialised torch.cat; the alias
    survives an optimiser step; state_dict hands out an unaliased copy."""
    ops = _ops()
    mm = importlib.import_module("plotpointe-gat-recommendation_amd.model")
    om = importlib.import_module("plotpointe-gat-recommendation_amd.optim")
    nu, ni, e = 700, 400, 12_000
    rng = np.random.default_rng(9)
    u = rng.integers(0, nu, e)
    it = rng.integers(nu, nu + ni, e)
    ei = torch.from_numpy(np.stack([np.concatenate([u, it]), np.concatenate([it, u])]).astype(np.int64)).to(cuda)
    torch.manual_seed(5)
    model = mm.PyGGAT(nu, ni, 256, 256, 2, 4, 0.0).to(cuda)
    feats = torch.randn(ni, 256, device=cuda)
    G = torch.randn(nu + ni, 256, device=cuda)
    joins = []
    orig = ops._JoinRows.apply
    monkeypatch.setattr(ops._JoinRows, "apply", lambda a, b: joins.append(1) or orig(a, b))
    opt = om.Adam(model.parameters(), lr=1e-3)

    def ref_pass():
        x = torch.cat([model.user_emb.weight, ops.linear(feats, model.item_proj.weight, model.item_proj.bias)], 0)
        for conv in model.convs:
            x = conv(x, ei)
        (x * G).sum().backward()
        return x.detach().clone(), {k: p.grad.detach().clone() for k, p in model.named_parameters()}

    for step in range(2):
        model.zero_grad(set_to_none=True)
        out = model(feats, ei)
        (out * G).sum().backward()
        got = {k: p.grad.detach().clone() for k, p in model.named_parameters()}
        assert model.user_emb.weight.data_ptr() == model._node_rows.data_ptr()
        model.zero_grad(set_to_none=True)
        ref_out, ref = ref_pass()
        assert torch.equal(out, ref_out)
        for k in ref:
            assert torch.equal(got[k], ref[k]), k
        for k, p in model.named_parameters():
            p.grad = got[k]
        opt.step()
    assert len(joins) == 2
    w = model.state_dict()["user_emb.weight"]
    assert w.untyped_storage().nbytes() == w.numel() * 4 and torch.equal(w, model.user_emb.weight.detach())
