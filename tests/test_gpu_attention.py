"""Attention weights on the GPU: the three new kernels at kernel level on the degree ladder (both
hub layouts), the layers' ``return_attention_weights``, the models' ``attention()`` and
``evaluation.attention_topk``.

Tolerance.  Per edge the error is |alpha - alpha64| over the largest float64
weight of the edge's destination; the bound is four times the same figure of the plain float32
torch-CPU restatement (tests/_attn_ref.py) on the same inputs, floored at 2^-24: the kernels may
order their arithmetic differently from the restatement, but not worse than a few of its
roundings.  Every figure is printed before it is asserted and written by ``test_report``
(profiles/r18/attention_parity.json holds the committed copy).
"""
import numpy as np
import pytest
import torch

import _attn_ref as R
from _gatv2_ref import SHAPES as V2_SHAPES
from conftest import write_report

pytestmark = pytest.mark.gpu

SLOPE = 0.2
N = R.N_NODES
_FIGS = {}


def _note(name, kernel, restatement):
    b = R.bound(restatement)
    _FIGS[name] = {"kernel": kernel, "restatement": restatement, "bound": b}
    print(f"[attention] {name}: kernel {kernel:.3e} restatement {restatement:.3e} bound {b:.3e}")
    return b


@pytest.fixture(scope="module")
def ladder(pkg, cuda):
    """The ladder graph, built with the default max_edges (two hubs, 5 pieces) and with 64 (eight hubs)."""
    ei = R.ladder_graph()
    eit = torch.from_numpy(ei).to(cuda)
    graphs = {"default": pkg.hip_ops.csr_build(eit, N), "hubs64": pkg.hip_ops.csr_build(eit, N, max_edges=64)}
    # rows longer than max_edges are cut: 257 (2 pieces) and 600 (3) at 256; eight rows at 64
    d, h = graphs["default"].fwd_sched, graphs["hubs64"].fwd_sched
    assert (d.n_hubs, d.n_hub_items) == (2, 5) and (h.n_hubs, h.n_hub_items) == (8, 3 + 3 * 2 + 4 + 4 + 5 + 10)
    deg = np.bincount(ei[1], minlength=N)
    return ei, eit, graphs, deg


def _dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _guarded(E, H, cuda):
    """An [E, H] output in the middle of a sentinel-filled buffer: (buffer, view, check())."""
    pad = 64
    buf = torch.full(((E + 2 * pad) * H,), -7.25, dtype=torch.float32, device=cuda)
    view = buf[pad * H:(pad + E) * H].view(E, H)

    def check():
        assert bool((buf[:pad * H] == -7.25).all()) and bool((buf[(pad + E) * H:] == -7.25).all())
    return view, check


def _common_checks(a_slot, a_edge, again, g, ei, deg, inv_l, pyg):
    """Finite, order 1 = order 0 permuted by csr_eid, relaunch bitwise, and in PyG mode the
    largest weight of a destination = inv_l bitwise, a degree-1 destination's weight = 1.0."""
    E, H = a_edge.shape
    assert bool(torch.isfinite(a_edge).all()) and bool((a_edge >= 0).all())
    assert torch.equal(a_edge[g.csr_eid.long()], a_slot)
    assert torch.equal(again, a_edge)
    if pyg:
        dst = torch.from_numpy(ei[1]).to(a_edge.device)
        mx = torch.zeros(N, H, device=a_edge.device).scatter_reduce(0, dst[:, None].expand(-1, H), a_edge, "amax",
                                                                    include_self=True)
        has = torch.from_numpy(deg > 0).to(a_edge.device)
        assert torch.equal(mx[has], inv_l.view(N, H)[has])
        one = int(np.flatnonzero(deg == 1)[0])
        assert bool((a_edge[dst == one] == 1.0).all())


def _v1_case(pkg, cuda, ladder, gname, H, mode, edge, scale, name):
    ei, eit, graphs, deg = ladder
    g = graphs[gname]
    E = ei.shape[1]
    ops, launch = pkg.hip_ops, pkg._launch
    rng = np.random.default_rng(100 + H)
    s_src = (scale * rng.uniform(-1, 1, (N, H))).astype(np.float32)
    s_dst = (scale * rng.uniform(-1, 1, (N, H))).astype(np.float32) if scale < 100 else np.zeros((N, H), np.float32)
    et = rng.uniform(-3, 3, (E, H)).astype(np.float32) if edge else None
    ss, sd = _dev(s_src, cuda), _dev(s_dst, cuda)
    et_slot = _dev(et, cuda)[g.csr_eid.long()].contiguous() if edge else None
    pyg = mode == R.MODE_PYG
    if pyg or H == 1:  # the forward's own state
        h = _dev(rng.standard_normal((N, H * 4)).astype(np.float32), cuda)
        _, m, inv_l, _ = ops.gat_fwd(g, h, ss, sd, None, H, 4, mode, SLOPE, 0.0, 0, want_agg=False, edge_term=et_slot)
    else:  # the forward's custom mode is heads == 1: the state restated in float32
        ex = torch.exp(torch.nn.functional.leaky_relu(ss[eit[0]] + sd[eit[1]] + (_dev(et, cuda) if edge else 0.0),
                                                      SLOPE).clamp(-10.0, 10.0))
        inv_l = 1.0 / (torch.zeros(N, H, device=cuda).index_add_(0, eit[1], ex) + 1e-9)
        m = torch.zeros(N, H, device=cuda)
    a_slot = ops.attention_weights(g, ss, sd, m, inv_l, H, mode, SLOPE, edge_term=et_slot, order="slot")
    a_edge = ops.attention_weights(g, ss, sd, m, inv_l, H, mode, SLOPE, edge_term=et_slot, order="edge")
    view, check = _guarded(E, H, cuda)
    for order in (0, 1):
        launch.attention(g, ss, sd, m, inv_l, H, mode, SLOPE, order, view, et_slot)
        torch.cuda.synchronize()
        check()
        assert torch.equal(view, a_edge if order else a_slot)
    _common_checks(a_slot, a_edge, view.clone(), g, ei, deg, inv_l, pyg)
    a64 = R.v1_alpha(s_src, s_dst, ei, mode, SLOPE, et)
    a32 = R.v1_alpha(s_src, s_dst, ei, mode, SLOPE, et, dtype=torch.float32)
    fig = R.metric(a_edge, a64, ei, N)
    assert fig <= _note(name, fig, R.metric(a32, a64, ei, N)), name
    return a_edge, a64


@pytest.mark.parametrize("gname", ["default", "hubs64"])
@pytest.mark.parametrize("edge", [False, True])
@pytest.mark.parametrize("mode", [R.MODE_PYG, R.MODE_CUSTOM])
@pytest.mark.parametrize("H", [1, 2, 4, 8])
def test_v1_kernel(pkg, cuda, ladder, H, mode, edge, gname):
    """Logits spanning +-80 (scores uniform in +-40)."""
    _v1_case(pkg, cuda, ladder, gname, H, mode, edge, 40.0, f"v1_{'pyg' if mode == 0 else 'custom'}_h{H}"
             f"{'_edge' if edge else ''}_{gname}")


@pytest.mark.parametrize("gname", ["default", "hubs64"])
def test_v1_kernel_extreme_logits(pkg, cuda, ladder, gname):
    """PyG mode, logits spanning +-900 (leaky: -180 .. 900): nothing non-finite, and a weight whose
    logit lies more than 104 below its destination's maximum (exp underflows past the smallest
    denormal near 103.3) is 0 or denormal."""
    ei = ladder[0]
    a, a64 = _v1_case(pkg, cuda, ladder, gname, 2, R.MODE_PYG, False, 900.0, f"v1_pyg_h2_span900_{gname}")
    far = (a64 < np.exp(-104.0)) & (R.dest_max(a64, ei, N)[torch.from_numpy(ei[1])] > 0)
    assert int(far.sum()) > 500
    got = a.cpu()[far]
    assert bool(torch.isfinite(got).all()) and bool((got < 1.1754944e-38).all()) and bool((got >= 0).all())


@pytest.mark.parametrize("gname", ["default", "hubs64"])
@pytest.mark.parametrize("H,C", V2_SHAPES + [(1, 64)], ids=[f"h{h}c{c}" for h, c in V2_SHAPES] + ["h1c64_span900"])
def test_v2_kernel(pkg, cuda, ladder, H, C, gname, request):
    """Logits spanning about +-80 (standard deviation 25 over the 600-edge row); the last case +-900."""
    ei, eit, graphs, deg = ladder
    g = graphs[gname]
    E = ei.shape[1]
    extreme = "span900" in request.node.name
    rng = np.random.default_rng(200 + H * C)
    xl, xr = (2.0 * rng.standard_normal((N, H * C)).astype(np.float32) for _ in range(2))
    att = ((12.0 if extreme else 1.0) * 12.0 / np.sqrt(C) * rng.standard_normal((H, C))).astype(np.float32)
    dxl, dxr, datt = _dev(xl, cuda), _dev(xr, cuda), _dev(att, cuda)
    ops, launch = pkg.hip_ops, pkg._launch
    out = torch.empty(N, C, device=cuda)
    m, inv_l = torch.empty(N, H, device=cuda), torch.empty(N, H, device=cuda)
    launch.dynatt_fwd(g, dxl, dxr, datt, None, H, C, SLOPE, 0.0, 0, None, out, m, inv_l)
    a_slot = ops.gatv2_attention_weights(g, dxl, dxr, datt, m, inv_l, H, C, SLOPE, order="slot")
    a_edge = ops.gatv2_attention_weights(g, dxl, dxr, datt, m, inv_l, H, C, SLOPE)
    view, check = _guarded(E, H, cuda)
    for order in (0, 1):
        launch.dynatt_attention(g, dxl, dxr, datt, m, inv_l, H, C, SLOPE, order, view)
        torch.cuda.synchronize()
        check()
        assert torch.equal(view, a_edge if order else a_slot)
    _common_checks(a_slot, a_edge, view.clone(), g, ei, deg, inv_l, True)
    a64 = R.v2_alpha(xl, xr, att, ei, H, SLOPE)
    a32 = R.v2_alpha(xl, xr, att, ei, H, SLOPE, dtype=torch.float32)
    name = f"v2_h{H}_c{C}{'_span900' if extreme else ''}_{gname}"
    fig = R.metric(a_edge, a64, ei, N)
    assert fig <= _note(name, fig, R.metric(a32, a64, ei, N)), name
    if extreme:
        far = (a64 < np.exp(-104.0)) & (R.dest_max(a64, ei, N)[torch.from_numpy(ei[1])] > 0)
        assert int(far.sum()) > 500
        got = a_edge.cpu()[far]
        assert bool(torch.isfinite(got).all()) and bool((got < 1.1754944e-38).all()) and bool((got >= 0).all())


def test_v2_unsupported_shape_raises(pkg, cuda, ladder):
    g = ladder[2]["default"]
    z = torch.zeros(N, 3 * 64, device=cuda)
    with pytest.raises(NotImplementedError):
        pkg.hip_ops.gatv2_attention_weights(g, z, z, torch.zeros(3, 64, device=cuda), torch.zeros(N, 3, device=cuda),
                                            torch.zeros(N, 3, device=cuda), 3, 64, SLOPE)


@pytest.fixture(scope="module")
def topk_vals(ladder):
    """Per H: val [E, H] in edge order, multiples of 1/16 in {0 .. 3/16} (ties everywhere; the head
    mean is exact), destination 9's 127 edges all equal."""
    ei = ladder[0]
    out = {}
    for H in (1, 2, 4):
        v = (np.random.default_rng(300 + H).integers(0, 4, (ei.shape[1], H)) / 16.0).astype(np.float32)
        v[ei[1] == 9] = 0.125
        out[H] = v
    return out


@pytest.mark.parametrize("k", [1, 8, 16, 17, 32])
@pytest.mark.parametrize("H", [1, 2, 4])
def test_topk_kernel(pkg, cuda, ladder, topk_vals, H, k):
    ei, eit, graphs, deg = ladder
    g = graphs["default"]
    val = topk_vals[H]
    slot = _dev(val, cuda)[g.csr_eid.long()].contiguous()
    eid, v, cnt = pkg.hip_ops.attention_topk(g, slot, k)
    eid2, v2, cnt2 = pkg.hip_ops.attention_topk(g, slot, k)
    r_eid, r_v, r_cnt = R.topk_ref(val, ei, N, k)
    assert eid.dtype == torch.int32 and cnt.dtype == torch.int32 and v.dtype == torch.float32
    assert np.array_equal(cnt.cpu().numpy(), r_cnt) and np.array_equal(r_cnt, np.minimum(k, deg))
    assert np.array_equal(eid.cpu().numpy(), r_eid)          # degree 0, degree < k, the all-equal row, the 600-edge row
    assert np.array_equal(v.cpu().numpy(), r_v)
    assert torch.equal(eid, eid2) and torch.equal(v, v2) and torch.equal(cnt, cnt2)


# ---- module level --------------------------------------------------------------------------------
def _conv_cases(pkg):
    kw = dict(concat=False, add_self_loops=False, dropout=0.5)
    return {
        "gat_64_128_h1": (lambda: pkg.GATConv(64, 128, heads=1, **kw), 64, 1, None),
        "gat_32_64_h2": (lambda: pkg.GATConv(32, 64, heads=2, **kw), 32, 2, None),
        "gat_wide_256_128_h2": (lambda: pkg.GATConv(256, 128, heads=2, **kw), 256, 2, None),
        "gat_edge1": (lambda: pkg.GATConv(64, 128, heads=1, edge_dim=1, **kw), 64, 1, 1),
        "gat_edge16": (lambda: pkg.GATConv(32, 64, heads=2, edge_dim=16, **kw), 32, 2, 16),
        "simple_64_128": (lambda: pkg.SimpleGATLayer(64, 128, attn_dropout=0.5), 64, 1, None),
        "gatv2_h1_c128": (lambda: pkg.GATv2Conv(64, 128, heads=1, **kw), 64, 1, None),
        "gatv2_h2_c64": (lambda: pkg.GATv2Conv(64, 64, heads=2, **kw), 64, 2, None),
        "gatv2_h1_c128_shared": (lambda: pkg.GATv2Conv(64, 128, heads=1, share_weights=True, **kw), 64, 1, None),
        "gatv2_h2_c64_shared": (lambda: pkg.GATv2Conv(64, 64, heads=2, share_weights=True, **kw), 64, 2, None),
    }


CONV_NAMES = ["gat_64_128_h1", "gat_32_64_h2", "gat_wide_256_128_h2", "gat_edge1", "gat_edge16", "simple_64_128",
              "gatv2_h1_c128", "gatv2_h2_c64", "gatv2_h1_c128_shared", "gatv2_h2_c64_shared"]


@pytest.mark.parametrize("name", CONV_NAMES)
def test_layer_return_attention_weights(pkg, cuda, ladder, name):
    ei, eit, graphs, deg = ladder
    make, K, H, D = _conv_cases(pkg)[name]
    torch.manual_seed(7)
    conv = make().to(cuda)
    E = ei.shape[1]
    x = torch.randn(N, K, device=cuda)
    G = torch.randn(N, conv.out_channels if hasattr(conv, "out_channels") else conv.out_dim, device=cuda)
    ea = () if D is None else (torch.rand(E, D, device=cuda),)
    # eval mode: PyG's tuple; out bitwise equal to the unflagged call
    conv.eval()
    with torch.no_grad():
        plain = conv(x, eit, *ea)
        out, (ei_back, alpha_eval) = conv(x, eit, *ea, return_attention_weights=True)
    assert ei_back is eit and torch.equal(out, plain)
    assert alpha_eval.shape == (E, H) and alpha_eval.dtype == torch.float32 and not alpha_eval.requires_grad
    # train mode, dropout 0.5: the same weights (before the mask), each destination's summing to 1
    conv.train()
    xg = x.clone().requires_grad_(True)
    torch.manual_seed(11)
    out_t, (_, alpha_train) = conv(xg, eit, *ea, return_attention_weights=True)
    assert not alpha_train.requires_grad and alpha_train.grad_fn is None
    assert torch.equal(alpha_train, alpha_eval)
    sums = torch.zeros(N, H, device=cuda, dtype=torch.float64).index_add_(0, eit[1], alpha_train.double())
    has = torch.from_numpy(deg > 0).to(cuda)
    tol = 1e-9 / float(np.exp(-10.0)) + 1e-5 if name.startswith("simple") else 1e-5  # (l / (l + 1e-9) in custom mode)
    assert float((sums[has] - 1).abs().max()) <= tol and float(sums[~has].abs().max()) == 0
    assert not torch.equal(out_t.detach(), plain)             # the dropout mask did act on out
    # the gradients of the flagged call are those of the unflagged one, bit for bit
    out_t.backward(G)
    flagged = [xg.grad.clone()] + [p.grad.clone() for p in conv.parameters()]
    assert all(bool(torch.isfinite(t).all()) for t in flagged)
    conv.zero_grad(set_to_none=True)
    xg2 = x.clone().requires_grad_(True)
    torch.manual_seed(11)
    out_u = conv(xg2, eit, *ea)
    assert torch.equal(out_u, out_t)
    out_u.backward(G)
    for a, b in zip(flagged, [xg2.grad] + [p.grad for p in conv.parameters()]):
        assert torch.equal(a, b)
    # forward_segments takes the keyword too
    if D is None:
        conv.eval()
        with torch.no_grad():
            o2, (_, a2) = conv.forward_segments(x[:250], x[250:], eit, return_attention_weights=True)
        assert a2.shape == (E, H) and torch.equal(o2, conv.forward_segments(x[:250], x[250:], eit))
        assert float((a2 - alpha_eval).abs().max()) <= 1e-5   # (the segmented projection may round differently)


def test_layer_without_edges_returns_an_empty_tensor(pkg, cuda):
    conv = pkg.GATConv(32, 64, heads=2, concat=False, add_self_loops=False).to(cuda).eval()
    ei0 = torch.zeros(2, 0, dtype=torch.int64, device=cuda)
    with torch.no_grad():
        out, (_, alpha) = conv(torch.randn(20, 32, device=cuda), ei0, return_attention_weights=True)
    assert alpha.shape == (0, 2) and out.shape == (20, 64)


# ---- models --------------------------------------------------------------------------------------
N_USERS, N_ITEMS, FEAT, HIDDEN, LAYERS = 250, 150, 32, 64, 2


def _model(pkg, family, cuda):
    model = __import__("importlib").import_module(f"{pkg.__name__}.model")
    torch.manual_seed(5)
    if family == "gat_pyg":
        return model.PyGGAT(N_USERS, N_ITEMS, FEAT, HIDDEN, LAYERS, 2, 0.3).to(cuda), 2
    if family == "gatv2_pyg":
        return model.PyGGATv2(N_USERS, N_ITEMS, FEAT, HIDDEN, LAYERS, 2, 0.3).to(cuda), 2
    return model.CustomGAT(N_USERS, N_ITEMS, FEAT, HIDDEN, LAYERS).to(cuda), 1


@pytest.mark.parametrize("family", ["gat_pyg", "gatv2_pyg", "gat_custom"])
def test_model_attention_and_topk(pkg, cuda, ladder, family):
    ei, eit, graphs, deg = ladder
    ev = __import__("importlib").import_module(f"{pkg.__name__}.evaluation")
    m, H = _model(pkg, family, cuda)
    feats = torch.randn(N_ITEMS, FEAT, device=cuda)
    layers = m.convs if hasattr(m, "convs") else m.layers
    m.train()
    layers[0].eval()                                          # a mixed state, to be found again afterwards
    flags = [mod.training for mod in m.modules()]
    alphas = m.attention(feats, eit)
    assert [mod.training for mod in m.modules()] == flags
    assert len(alphas) == LAYERS
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    if family == "gatv2_pyg":
        assert "convs.0.lin_r.weight" in sd
    r64 = R.model_alphas(sd, feats.cpu(), ei, LAYERS, H, family, SLOPE)
    r32 = R.model_alphas(sd, feats.cpu(), ei, LAYERS, H, family, SLOPE, dtype=torch.float32)
    for l, a in enumerate(alphas):
        assert a.shape == (ei.shape[1], H) and a.dtype == torch.float32 and not a.requires_grad
        fig = R.metric(a, r64[l], ei, N)
        name = f"model_{family}_layer{l}"
        assert fig <= _note(name, fig, R.metric(r32[l], r64[l], ei, N)), name
    # the most-attended neighbours: the selection over the last layer's weights
    for k, layer in ((10, -1), (3, 0)):
        src, w, cnt = ev.attention_topk(m, feats, eit, k, layer=layer)
        assert [mod.training for mod in m.modules()] == flags
        r_eid, r_w, r_cnt = R.topk_ref(alphas[layer].cpu().numpy(), ei, N, k)
        r_src = np.where(r_eid >= 0, ei[0][np.maximum(r_eid, 0)], -1)
        assert src.dtype == torch.int64 and np.array_equal(src.cpu().numpy(), r_src)
        assert np.array_equal(w.cpu().numpy(), r_w) and np.array_equal(cnt.cpu().numpy(), r_cnt)


def test_report():
    """The figures of this run, written by conftest.write_report as attention_parity.json."""
    assert _FIGS, "run after the parity tests of this file"
    worst = max(_FIGS.items(), key=lambda kv: kv[1]["kernel"] / kv[1]["bound"])
    write_report("attention_parity", {"metric": "max |alpha - alpha64| / max_dest alpha64", "cases": _FIGS,
                                      "worst_case": worst[0], "worst_kernel_over_bound": worst[1]["kernel"] / worst[1]["bound"]})
