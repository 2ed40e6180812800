"""GATConv edge features on the GPU: the staged attribute tables, the fused operator against the
float64 restatement (tests/_egat_ref.py) evaluated on the same fp32 inputs -- the host test
checks that no logit of the recipe sits within 1e-5 of the LeakyReLU kink, so both take the same
side on every edge -- then the zero term, edge_attr=None, 1-D attributes, the empty graph, bitwise
repeatability (debug library included), graph capture, the 2-layer model and the trainer.

The asserted bounds are the project's: 1e-5 for rows and gradients, 1e-4 for attention vectors.
The figures measured on an MI355X (write_report; profiles/r12/parity/egat_*.json) are in DESIGN.md
section 15: out rows 6.7e-7, dx 8.5e-7 on its term scale, edge-parameter gradients 1.8e-6 at worst."""
import functools
import importlib
import json
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import _egat_ref as ref
from conftest import ROOT, row_rel, write_report

pytestmark = pytest.mark.gpu

TOL, TOL_ATT = 1e-5, 1e-4  # the project's bounds: rows and gradients; attention vectors
SEED = 20250114
N = ref.N_NODES
LEAVES = ("x", "W", "att_src", "att_dst", "lin_edge", "att_edge", "bias")


@pytest.fixture(scope="module")
def hip_ops(pkg):
    return importlib.import_module(pkg.__name__ + ".hip_ops")


@pytest.fixture(scope="module", autouse=True)
def _epoch_zero(pkg, cuda):
    pkg._lib.dropout_set_epoch(0, cuda)
    yield
    pkg._lib.dropout_set_epoch(0, cuda)


@pytest.fixture(scope="module")
def graphs(pkg, hip_ops, cuda):
    """{max_edges: CSRGraph} over the 900-node test graph (hub pieces at 256, many more at 32)."""
    ei = ref.make_graph()
    eid = torch.from_numpy(ei).to(cuda)
    out = {256: hip_ops.csr_build(eid, N), 32: hip_ops.csr_build(eid, N, max_edges=32)}
    assert out[256].fwd_sched.n_hubs >= 1 and out[256].bwd_sched.n_hubs >= 1
    assert out[32].fwd_sched.n_hub_items >= 22 + 9 and out[32].bwd_sched.n_hub_items >= 22
    triple = np.flatnonzero((ei[0] == 11) & (ei[1] == 7))
    assert triple.size == 3
    return types.SimpleNamespace(ei=ei, by_max=out, E=ei.shape[1], triple=triple)


@functools.lru_cache(maxsize=None)
def _mask(E: int, H: int, p: float, seed: int):
    from oracle import gat_oracle
    if p <= 0:
        return None
    return torch.from_numpy(np.stack([gat_oracle.dropout_scale(seed, np.arange(E), h, p) for h in range(H)], 1))


@functools.lru_cache(maxsize=None)
def _inputs(H: int, C: int, D: int, zero_att_edge: bool = False):
    ei = ref.make_graph()
    P = ref.inputs(N, ei.shape[1], H, C, D)
    if zero_att_edge:
        P["att_edge"] = np.zeros_like(P["att_edge"])
    return P  # shared: callers copy before they change anything


@functools.lru_cache(maxsize=None)
def _reference(H: int, C: int, D: int, p: float, zero_att_edge: bool = False):
    """The float64 layer and gradients on the recipe's fp32 inputs (computed once per case)."""
    ei = ref.make_graph()
    return ref.formulas(_inputs(H, C, D, zero_att_edge), ei, H, 0.2, _mask(ei.shape[1], H, p, SEED))


def _v(lin_edge, att_edge, H):
    """GATConv._edge_args' v: an elementwise product and a sum."""
    C = att_edge.numel() // H
    return (lin_edge.view(H, C, -1) * att_edge.view(H, C, 1)).sum(1)


def _run(hip_ops, g, P, H, C, p, cuda, edge=True, seed=SEED, attr=None):
    """out and the gradients of LEAVES (None where a leaf takes no part) through hip_ops.gat_layer."""
    T = {k: torch.from_numpy(np.array(P[k])).to(cuda) for k in LEAVES}
    for t in T.values():
        t.requires_grad_(True)
    if attr is None:
        attr = torch.from_numpy(np.array(P["edge_attr"])).to(cuda)
    kw = dict(edge_v=_v(T["lin_edge"], T["att_edge"], H), edge_attr=attr) if edge else {}
    out = hip_ops.gat_layer(T["x"], T["W"], T["att_src"], T["att_dst"], T["bias"], g, H, C, 0, 0.2, p, seed, **kw)
    G = torch.from_numpy(np.array(P["G"])).to(cuda)
    grads = torch.autograd.grad(out, [T[k] for k in LEAVES], G, allow_unused=True)
    return (out.detach(),) + tuple(grads)


def _figures(got, want):
    """The issue's bounds for one operator run; returns the measured figures."""
    out, dx, dW, das, dad, dle, dae, db = got
    fig = {"z_absmax": want["z_absmax"], "kink_ratio": want["kink_ratio"]}
    fig["out_row_rel"] = row_rel(out, want["out"])[0]
    fig["dx_whole"] = ref.rel(dx, want["dx"])
    fig["dx_scaled_rows"], fig["dx_zero_scale_rows_absmax"] = ref.scaled_rows(dx, want["dx"], want["scale_x"])
    fig["dx_plain_rows"] = row_rel(dx, want["dx"])[0]  # reported, not asserted (rows whose terms cancel)
    fig["dW"], fig["dbias"] = ref.rel(dW, want["dW"]), ref.rel(db, want["dbias"])
    fig["datt_src"], fig["datt_dst"] = ref.rel(das, want["datt_src"]), ref.rel(dad, want["datt_dst"])
    fig["dlin_edge"], fig["datt_edge"] = ref.rel(dle, want["dlin_edge"]), ref.rel(dae, want["datt_edge"])
    return fig


def _check(fig, edge_grads=("dlin_edge", "datt_edge")):
    print(json.dumps(fig))
    assert fig["out_row_rel"] <= TOL, fig
    assert fig["dx_whole"] <= TOL and fig["dx_scaled_rows"] <= TOL and fig["dx_zero_scale_rows_absmax"] == 0.0, fig
    assert fig["dW"] <= TOL and fig["dbias"] <= TOL, fig
    for k in ("datt_src", "datt_dst") + tuple(edge_grads):
        assert fig[k] <= TOL_ATT, (k, fig)
    return fig


# ---------------------------------------------------------------------------------------------
# staging
# ---------------------------------------------------------------------------------------------
def test_staging_tables_and_cache(pkg, hip_ops, graphs, cuda):
    """attr[csr_eid] and attr[csc_eid] bit for bit; the same tensor again does no work; an in-place
    edit restages; a 1-D tensor stages as [E, 1]."""
    ops_graph = importlib.import_module(pkg.__name__ + ".ops_graph")  # the counter lives where it is counted
    g, E = graphs.by_max[256], graphs.E
    rng = np.random.default_rng(3)
    for D in (1, 3, 16):
        attr = torch.from_numpy(rng.random((E, D)).astype(np.float32)).to(cuda)
        n0 = ops_graph.EDGE_STAGE_COUNT
        a_csr, a_csc = hip_ops.stage_edge_attr(g, attr)
        assert ops_graph.EDGE_STAGE_COUNT == n0 + 1
        assert torch.equal(a_csr, attr[g.csr_eid.long()]) and torch.equal(a_csc, attr[g.csc_eid.long()])
        b_csr, b_csc = hip_ops.stage_edge_attr(g, attr)
        assert ops_graph.EDGE_STAGE_COUNT == n0 + 1 and b_csr is a_csr and b_csc is a_csc
        attr[5:9].mul_(2.0)
        c_csr, c_csc = hip_ops.stage_edge_attr(g, attr)
        assert ops_graph.EDGE_STAGE_COUNT == n0 + 2 and c_csr is not a_csr
        assert torch.equal(c_csr, attr[g.csr_eid.long()]) and torch.equal(c_csc, attr[g.csc_eid.long()])
        # an equal tensor that is another object is another entry (no keying on contents or addresses)
        hip_ops.stage_edge_attr(g, attr.clone())
        assert ops_graph.EDGE_STAGE_COUNT == n0 + 3
    flat = torch.from_numpy(rng.random(E).astype(np.float32)).to(cuda)
    f_csr, f_csc = hip_ops.stage_edge_attr(g, flat)
    assert tuple(f_csr.shape) == (E, 1) and torch.equal(f_csr[:, 0], flat[g.csr_eid.long()])
    assert torch.equal(f_csc[:, 0], flat[g.csc_eid.long()])
    with pytest.raises(ValueError, match="edge_attr"):
        hip_ops.stage_edge_attr(g, flat[:-1])
    with pytest.raises(ValueError, match="edge_attr"):
        hip_ops.stage_edge_attr(g, flat.double())
    with pytest.raises(ValueError, match="edge_attr"):
        hip_ops.stage_edge_attr(g, flat.cpu())


def test_term_tables(hip_ops, graphs, cuda):
    """t_csr[k, h] = <attr[csr_eid[k]], v[h]> and t_csc likewise, the same bits for the same edge;
    without a backward only t_csr is made."""
    g, E = graphs.by_max[32], graphs.E
    rng = np.random.default_rng(4)
    for H, D in ((1, 1), (2, 3), (8, 16)):
        attr = torch.from_numpy(rng.random((E, D)).astype(np.float32)).to(cuda)
        v = torch.from_numpy(rng.standard_normal((H, D)).astype(np.float32)).to(cuda)
        staged = hip_ops.stage_edge_attr(g, attr)
        t_csr, t_csc = hip_ops.edge_terms(g, staged, v, H, want_csc=True)
        t_csr, t_csc = t_csr.view(E, H), t_csc.view(E, H)
        want = attr.double() @ v.double().t()
        assert float((t_csr.double() - want[g.csr_eid.long()]).abs().max()) <= 1e-6 * float(want.abs().max())
        by_edge = torch.empty_like(t_csr)
        by_edge[g.csr_eid.long()] = t_csr
        assert torch.equal(by_edge[g.csc_eid.long()], t_csc)
        only, none = hip_ops.edge_terms(g, staged, v, H, want_csc=False)
        assert none is None and torch.equal(only.view(E, H), t_csr)


# ---------------------------------------------------------------------------------------------
# operator
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,C,D", ref.CASES)
def test_operator_parity(hip_ops, graphs, cuda, H, C, D):
    """out and every gradient against float64 at p = 0 and p = 0.3, on max_edges 256 and 32."""
    P = _inputs(H, C, D)
    ind = np.bincount(graphs.ei[1], minlength=N)
    iso = torch.from_numpy(np.flatnonzero(ind == 0)).to(cuda)
    bias = torch.from_numpy(np.array(P["bias"])).to(cuda)
    a3 = P["edge_attr"][graphs.triple]
    assert len({tuple(r) for r in a3.tolist()}) == 3  # the three 11 -> 7 columns carry distinct attributes
    record = {}
    for p in (0.0, 0.3):
        want = _reference(H, C, D, p)
        for T, g in graphs.by_max.items():
            got = _run(hip_ops, g, P, H, C, p, cuda)
            assert iso.numel() >= 20 and torch.equal(got[0][iso], bias.expand(iso.numel(), C))
            record[f"p{p}_max_edges{T}"] = _check(_figures(got, want))
    write_report(f"egat_op_h{H}_c{C}_d{D}", record)


def test_a_wrong_permutation_would_fail(hip_ops, graphs, cuda):
    """The parity bound is sensitive to the edge order: the same layer fed the attributes shifted
    by one column is off by far more than the bound.  (Among the three 11 -> 7 columns alone a
    permutation shows only under dropout: the three share both end points, and the masks go by
    edge id -- the p = 0.3 cases above cover that.)"""
    H, C, D = 1, 64, 1
    P = dict(_inputs(H, C, D))
    P["edge_attr"] = np.roll(np.array(P["edge_attr"]), 1, axis=0)
    got = _run(hip_ops, graphs.by_max[256], P, H, C, 0.0, cuda)
    err = row_rel(got[0], _reference(H, C, D, 0.0)["out"])[0]
    print("out rows with shifted attributes:", err)
    assert err > 100 * TOL


@pytest.mark.parametrize("H,C,D", [(1, 128, 1), (2, 64, 3)])
def test_zero_term(hip_ops, graphs, cuda, H, C, D):
    """att_edge = 0: out and the existing parameters' gradients agree with the layer run without edge
    features; datt_edge is non-zero and matches the reference; dlin_edge is zero."""
    P = _inputs(H, C, D, True)
    want = _reference(H, C, D, 0.3, True)
    for g in graphs.by_max.values():
        got = _run(hip_ops, g, P, H, C, 0.3, cuda)
        plain = _run(hip_ops, g, P, H, C, 0.3, cuda, edge=False)
        assert plain[5] is None and plain[6] is None
        same = all(torch.equal(got[k], plain[k]) for k in (0, 1, 2, 3, 4, 7))
        print(f"zero term h{H} c{C} d{D} max_edges {g.fwd_sched.max_edges}: bitwise equal to the plain layer: {same}")
        assert row_rel(got[0], plain[0])[0] <= TOL
        for k in (1, 2, 3, 4, 7):
            assert ref.rel(got[k], plain[k]) <= TOL, k
        fig = _figures(got, want)
        assert float(want["datt_edge"].abs().max()) > 0 and float(got[5].abs().max()) == 0.0
        _check(fig, edge_grads=("datt_edge",))


def test_module_without_edge_attr_is_the_plain_layer(pkg, graphs, cuda):
    """A layer built with edge_dim called with edge_attr=None runs today's path (PyG skips the term
    in the same way): bitwise the plain layer, and lin_edge / att_edge get no gradient."""
    kw = dict(heads=2, concat=False, add_self_loops=False, dropout=0.3)
    torch.manual_seed(3)
    conv = pkg.GATConv(128, 64, edge_dim=3, **kw).to(cuda).train()
    torch.manual_seed(3)
    plain = pkg.GATConv(128, 64, **kw).to(cuda).train()
    ei = torch.from_numpy(graphs.ei).to(cuda)
    x = torch.from_numpy(np.array(_inputs(2, 64, 3)["x"])).to(cuda)
    G = torch.from_numpy(np.array(_inputs(2, 64, 3)["G"])).to(cuda)
    outs = []
    for m in (conv, plain):
        torch.manual_seed(11)  # the dropout seed
        out = m(x, ei)
        out.backward(G)
        outs.append(out.detach())
    assert torch.equal(outs[0], outs[1])
    for k, p in plain.named_parameters():
        assert torch.equal(dict(conv.named_parameters())[k].grad, p.grad), k
    assert conv.lin_edge.weight.grad is None and conv.att_edge.grad is None
    with pytest.raises(ValueError, match="edge_dim"):
        plain(x, ei, torch.zeros(graphs.E, 3, device=cuda))
    with pytest.raises(ValueError, match="edge_attr"):
        conv(x, ei, torch.zeros(graphs.E, 2, device=cuda))
    with pytest.raises(NotImplementedError, match="requires_grad"):
        conv(x, ei, torch.zeros(graphs.E, 3, device=cuda, requires_grad=True))


def test_module_against_the_operator_and_flat_attributes(pkg, hip_ops, graphs, cuda):
    """GATConv(edge_dim=1): a 1-D edge_attr [E] equals the [E, 1] form bit for bit; the module is
    the operator spelled out; its parameter gradients against the float64 reference."""
    H, C, D = 2, 64, 1
    P = dict(_inputs(H, C, D))
    conv = pkg.GATConv(ref.K_IN, C, heads=H, edge_dim=D, concat=False, add_self_loops=False).to(cuda)
    with torch.no_grad():
        for k, name in (("lin.weight", "W"), ("att_src", "att_src"), ("att_dst", "att_dst"), ("bias", "bias"),
                        ("lin_edge.weight", "lin_edge"), ("att_edge", "att_edge")):
            t = dict(conv.named_parameters())[k]
            t.copy_(torch.from_numpy(np.array(P[name])).view(t.shape))
    ei = torch.from_numpy(graphs.ei).to(cuda)
    x = torch.from_numpy(np.array(P["x"])).to(cuda)
    G = torch.from_numpy(np.array(P["G"])).to(cuda)
    col = torch.from_numpy(np.array(P["edge_attr"])).to(cuda)
    flat = col[:, 0].clone()
    res = []
    for attr in (col, flat):
        conv.zero_grad(set_to_none=True)
        out = conv(x, ei, attr)
        out.backward(G)
        res.append([out.detach()] + [p.grad.clone() for p in conv.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(*res))
    want = _reference(H, C, D, 0.0)
    fig = {"out_row_rel": row_rel(res[0][0], want["out"])[0],
           "dlin_edge": ref.rel(conv.lin_edge.weight.grad, want["dlin_edge"]),
           "datt_edge": ref.rel(conv.att_edge.grad.view(H, C), want["datt_edge"]),
           "dW": ref.rel(conv.lin.weight.grad, want["dW"]), "datt_src": ref.rel(conv.att_src.grad.view(H, C),
                                                                               want["datt_src"])}
    print(json.dumps(fig))
    assert fig["out_row_rel"] <= TOL and fig["dW"] <= TOL, fig
    assert fig["dlin_edge"] <= TOL_ATT and fig["datt_edge"] <= TOL_ATT and fig["datt_src"] <= TOL_ATT, fig
    # forward_segments: the same rows as two tensors
    conv.eval()
    with torch.no_grad():
        assert torch.equal(conv.forward_segments(x[:300].clone(), x[300:].clone(), ei, col), conv(x, ei, col))
    write_report("egat_module", fig)


def test_no_grad_forward_makes_no_backward_table(pkg, hip_ops, graphs, cuda, monkeypatch):
    """Eval / export: the forward asks for the CSR term table only."""
    asked = []
    real = hip_ops.edge_terms
    ops_gat = importlib.import_module(pkg.__name__ + ".ops_gat")  # where GATLayer.forward looks edge_terms up
    monkeypatch.setattr(ops_gat, "edge_terms", lambda g, s, v, h, want_csc: asked.append(want_csc) or
                        real(g, s, v, h, want_csc))
    conv = pkg.GATConv(128, 64, heads=1, edge_dim=1, concat=False, add_self_loops=False).to(cuda).eval()
    x = torch.from_numpy(np.array(_inputs(1, 64, 1)["x"])).to(cuda)
    attr = torch.from_numpy(np.array(_inputs(1, 64, 1)["edge_attr"])).to(cuda)
    ei = torch.from_numpy(graphs.ei).to(cuda)
    with torch.no_grad():
        a = conv(x, ei, attr)
    b = conv(x, ei, attr)
    assert asked == [False, True] and torch.equal(a, b.detach())


def test_no_edges(hip_ops, cuda):
    n, H, C, D = 50, 2, 64, 3
    g = hip_ops.csr_build(torch.zeros(2, 0, dtype=torch.int64, device=cuda), n)
    P = ref.inputs(n, 0, H, C, D)
    got = _run(hip_ops, g, P, H, C, 0.3, cuda)
    bias = torch.from_numpy(P["bias"]).to(cuda)
    assert torch.equal(got[0], bias.expand(n, C))
    assert all(t is not None and bool(torch.isfinite(t).all()) for t in got)
    for k in (1, 2, 3, 4, 5, 6):
        assert float(got[k].abs().max()) == 0.0, k
    assert ref.rel(got[7], P["G"].sum(0)) <= TOL


def test_repeat_gives_the_same_bits(hip_ops, graphs, cuda):
    for (H, C, D), T in (((4, 128, 3), 256), ((1, 64, 1), 32), ((1, 32, 3), 32)):
        P = _inputs(H, C, D)
        a = _run(hip_ops, graphs.by_max[T], P, H, C, 0.3, cuda)
        b = _run(hip_ops, graphs.by_max[T], P, H, C, 0.3, cuda)
        assert all(torch.equal(x, y) for x, y in zip(a, b))


DEBUG_SNIPPET = r"""
import sys, importlib
import numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import _egat_ref as ref
pkg = importlib.import_module("plotpointe-gat-recommendation_amd")
hip_ops = importlib.import_module(pkg.__name__ + ".hip_ops")
assert pkg._lib.debug_build()
H, C, D, n = 2, 64, 3, ref.N_NODES
ei = ref.make_graph()
g = hip_ops.csr_build(torch.from_numpy(ei).cuda(), n)
P = ref.inputs(n, ei.shape[1], H, C, D)
names = ("x", "W", "att_src", "att_dst", "lin_edge", "att_edge", "bias")
T = {k: torch.from_numpy(P[k]).cuda().requires_grad_(True) for k in names}
v = (T["lin_edge"].view(H, C, -1) * T["att_edge"].view(H, C, 1)).sum(1)
out = hip_ops.gat_layer(T["x"], T["W"], T["att_src"], T["att_dst"], T["bias"], g, H, C, 0, 0.2, 0.3, int(sys.argv[3]),
                        edge_v=v, edge_attr=torch.from_numpy(P["edge_attr"]).cuda())
grads = torch.autograd.grad(out, [T[k] for k in names], torch.from_numpy(P["G"]).cuda())
np.savez(sys.argv[2], *[t.detach().cpu().numpy() for t in (out,) + tuple(grads)])
print("DEBUG-OK")
"""


def test_debug_library_gives_the_same_bits(hip_ops, graphs, cuda, tmp_path):
    dbg = ROOT / "plotpointe-gat-recommendation_amd" / "libppgat_debug.so"
    if not dbg.exists():
        pytest.fail("libppgat_debug.so missing: build() makes it")
    env = dict(os.environ, PPGAT_LIB=str(dbg), HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, "-c", DEBUG_SNIPPET, str(ROOT), str(tmp_path / "d.npz"), str(SEED)], env=env,
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "DEBUG-OK" in p.stdout, p.stdout[-2000:] + p.stderr[-3000:]
    got = _run(hip_ops, graphs.by_max[256], _inputs(2, 64, 3), 2, 64, 0.3, cuda)
    with np.load(tmp_path / "d.npz") as z:
        for k, t in enumerate(got):
            assert np.array_equal(z[f"arr_{k}"], t.cpu().numpy()), k


# ---------------------------------------------------------------------------------------------
# model, capture, trainer
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cfg1(pkg_name: str):
    """The cfg1 synthetic graph with its rating edge features."""
    pkg = importlib.import_module(pkg_name)
    data = pkg.data
    inter = data.synthetic_interactions_small(seed=0)
    maps = data.node_maps_from_interactions(inter)
    u2i, i2i = data.index_maps(maps)
    tr, _, _ = data.map_splits_to_index(*data.build_splits(inter), u2i, i2i)
    n_users, n_items = int(maps["n_users"]), int(maps["n_items"])
    ei = data.build_edge_index(n_users, n_items, tr)
    ea = data.edge_attr_rating(tr, inter, u2i, i2i)
    feats = np.random.RandomState(0).standard_normal((n_items, 64)).astype(np.float32)
    return n_users, n_items, ei, ea, feats


@pytest.mark.parametrize("heads", [1, 2])
def test_model_two_layers(pkg, cuda, heads):
    """PyGGAT(hidden=128, edge_dim=1), two layers, on the cfg1 synthetic graph against the float64
    stack: Z rows and both layers' edge-parameter gradients (the stacked layers' producer hand-off
    is on for heads = 1)."""
    n_users, n_items, ei, ea, feats = _cfg1(pkg.__name__)
    torch.manual_seed(7)
    model = pkg.PyGGAT(n_users, n_items, item_feat_dim=64, hidden=128, layers=2, heads=heads, attn_dropout=0.1,
                       edge_dim=1).to(cuda).eval()
    with torch.no_grad():
        for c in model.convs:
            c.att_edge.mul_(3.0)
            c.bias.copy_(0.05 * torch.randn_like(c.bias))
    f_d, ei_d, ea_d = torch.from_numpy(feats).to(cuda), ei.to(cuda), torch.from_numpy(ea).to(cuda)
    Gn = np.random.default_rng(2).standard_normal((n_users + n_items, 128)).astype(np.float32)
    Z = model(f_d, ei_d, ea_d)
    Z.backward(torch.from_numpy(Gn).to(cuda))
    sd = {k: v.detach().double().cpu().requires_grad_(True) for k, v in model.state_dict().items()}
    Z64 = ref.model_forward(sd, torch.from_numpy(feats).double(), ei, torch.from_numpy(ea).double(), 2, heads)
    (Z64 * torch.from_numpy(Gn).double()).sum().backward()
    fig = {"Z_row_rel": row_rel(Z, Z64)[0]}
    params = dict(model.named_parameters())
    for l in (0, 1):
        for k in (f"convs.{l}.lin_edge.weight", f"convs.{l}.att_edge", f"convs.{l}.att_src", f"convs.{l}.lin.weight"):
            fig["d_" + k] = ref.rel(params[k].grad, sd[k].grad)
    print(json.dumps(fig))
    write_report(f"egat_model_h{heads}", fig)
    assert fig["Z_row_rel"] <= TOL, fig
    for l in (0, 1):
        assert fig[f"d_convs.{l}.lin_edge.weight"] <= TOL_ATT and fig[f"d_convs.{l}.att_edge"] <= TOL_ATT, fig


def test_graph_replay_equals_eager_steps(pkg, cuda):
    """One forward + backward + Adam step of a 2-layer PyGGAT(edge_dim=1) captured after an eager
    warm-up (which stages the attributes) and replayed 3 times == the same 3 steps run eagerly;
    the masks advance per replay."""
    _lib = pkg._lib
    g = pkg.data.synthetic_ui_graph(n_users=3000, n_items=800, n_interactions=40_000, seed=5)
    ei = torch.from_numpy(g.edge_index_numpy()).to(cuda)
    ea = torch.from_numpy(np.random.default_rng(8).integers(0, 5, ei.size(1)).astype(np.float32) / 4).to(cuda)
    feats = torch.from_numpy(pkg.data.synthetic_item_features(g.n_items, 64, seed=5)).to(cuda)
    torch.manual_seed(0)
    model = pkg.PyGGAT(g.n_users, g.n_items, item_feat_dim=64, hidden=128, layers=2, heads=1, attn_dropout=0.2,
                       edge_dim=1).to(cuda).train()
    u, i, j = (torch.from_numpy(a).to(cuda) for a in pkg.data.sample_bpr_numpy(g.user_ptr, g.user_items, g.n_items,
                                                                                 20_000, seed=1))
    opt = pkg.optim.Adam(model.parameters(), lr=1e-2, weight_decay=1e-4, capturable=True)

    def step():
        _lib.dropout_advance(cuda)
        loss = pkg.bpr_loss(model(feats, ei, ea), g.n_users, u, i, j)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        return loss.detach()

    try:
        side = torch.cuda.Stream(cuda)
        side.wait_stream(torch.cuda.current_stream(cuda))
        with torch.cuda.stream(side):
            for _ in range(2):
                step()
        torch.cuda.current_stream(cuda).wait_stream(side)
        torch.cuda.synchronize()
        snap_p = [p.detach().clone() for p in model.parameters()]
        snap_s = {k: (v["exp_avg"].clone(), v["exp_avg_sq"].clone(), v["step"].clone()) for k, v in opt.state.items()}
        graph = torch.cuda.CUDAGraph()
        torch.manual_seed(99)
        with torch.cuda.graph(graph):
            loss_static = step()
        _lib.dropout_set_epoch(1000, cuda)
        losses_g = []
        for _ in range(3):
            graph.replay()
            losses_g.append(float(loss_static))
        got = [p.detach().clone() for p in model.parameters()]
        with torch.no_grad():
            for p, s in zip(model.parameters(), snap_p):
                p.copy_(s)
            for k, (m, v, t) in snap_s.items():
                opt.state[k]["exp_avg"].copy_(m)
                opt.state[k]["exp_avg_sq"].copy_(v)
                opt.state[k]["step"].copy_(t)
        _lib.dropout_set_epoch(1000, cuda)
        losses_e = []
        for _ in range(3):
            torch.manual_seed(99)  # the host seeds the capture baked in
            losses_e.append(float(step()))
        torch.cuda.synchronize()
    finally:
        _lib.dropout_set_epoch(0, cuda)
    print("losses", losses_g, losses_e)
    assert len(set(losses_g)) == 3  # parameters and masks move between replays
    np.testing.assert_allclose(losses_g, losses_e, rtol=1e-6)
    moved = [float((a - s).abs().max()) for a, s in zip(got, snap_p)]
    names = [k for k, _ in model.named_parameters()]
    assert all(moved[names.index(k)] > 0 for k in ("convs.0.lin_edge.weight", "convs.1.att_edge"))
    for a, b in zip(got, model.parameters()):
        assert ref.rel(a, b) <= 1e-6


def _train_child(tmp, *flags, epochs=2, samples=20000):
    """train.py in a fresh process under a time limit -> (stdout, metrics record, checkpoint path)."""
    out = tmp / ("run_" + "_".join(f.strip("-") for f in flags[:2]) if flags else "run_default")
    cmd = [sys.executable, str(ROOT / "plotpointe-gat-recommendation_amd" / "train.py"), "--synthetic", "cfg1",
           "--epochs", str(epochs), "--eval-neg-k", "100", "--samples-per-epoch", str(samples), "--device-eval",
           "--models-prefix", str(out)] + list(flags)
    p = subprocess.run(cmd, cwd=str(ROOT), capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"))
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    files, ckpts = list(out.glob("metrics_gat_pyg_d128_*.json")), list((out / "checkpoints").glob("gat_pyg_d128_*.pt"))
    assert len(files) == 1 and len(ckpts) == 1
    return p.stdout, json.loads(files[0].read_text()), ckpts[0]


def test_trainer_with_rating_features(pkg, cuda, tmp_path):
    """train.py --edge-features rating in a child; its checkpoint reloaded into a fresh model here
    reproduces what the child computed from its final model: the --recommend-out lists and scores
    (made from the child's final Z after it reloaded the best checkpoint) bit for bit, and the test
    metrics of the metrics JSON under the child's own sampler and seed."""
    train = importlib.import_module(pkg.__name__ + ".train")
    recs = tmp_path / "recs.npz"
    log, rec, ckpt_path = _train_child(tmp_path, "--edge-features", "rating", "--recommend-out", str(recs),
                                       "--recommend-k", "10")
    losses = [float(v) for v in re.findall(r"\] loss=(\S+) \(bpr\)", log)]
    print("losses", losses)
    assert len(losses) == 2 and all(np.isfinite(losses)), losses
    assert rec["config"]["edge_features"] == "rating"
    ck = torch.load(ckpt_path, map_location=cuda, weights_only=True)
    assert ck["config"]["edge_features"] == "rating" and "convs.1.lin_edge.weight" in ck["state_dict"]
    cfg = train.Config(**ck["config"])
    tr, va, te, n_users, n_items, feats_np = train.load_inputs(cfg, "cfg1")
    feats = torch.tensor(feats_np, dtype=torch.float32, device=cuda)
    ei = pkg.data.build_edge_index(n_users, n_items, tr).to(cuda)
    ea = torch.from_numpy(train.load_edge_attr(cfg, "cfg1", tr)).to(cuda)
    assert tuple(ea.shape) == (ei.size(1), 1)
    m = train.build_model(cfg, n_users, n_items, feats_np.shape[1]).to(cuda).eval()
    m.load_state_dict(ck["state_dict"])
    with torch.no_grad():
        Z = m(feats, ei, ea)
        assert bool(torch.isfinite(Z).all()) and not torch.equal(m(feats, ei), Z)  # the edge term is live
    # the child's final embeddings, through its lists: same items, same scores, bit for bit
    ptr, flat = train.user_csr(tr, n_users)
    sampler = importlib.import_module(pkg.__name__ + ".sampler").BPRSampler(ptr, flat, n_items, device=cuda)
    idx, sc = pkg.recommend_topk(Z[:n_users], Z[n_users:n_users + n_items], None, k=10, sampler=sampler)
    with np.load(recs) as z:
        assert z["items"].shape == (n_users, 10)
        assert np.array_equal(z["items"], idx.cpu().numpy()) and np.array_equal(z["scores"], sc.cpu().numpy())
    # and the child's test metrics: the same protocol (--device-eval), sampler and seed
    samp = pkg.evaluation.eval_sampled(m, cfg, feats, ei, tr, te, fast=False, sampler=sampler, seed=cfg.seed,
                                       edge_attr=ea)
    assert samp == rec["test"], (samp, rec["test"])
    full = pkg.eval_full(m, cfg, feats, ei, tr, te, edge_attr=ea)
    assert set(full) == {"recall@10", "recall@20", "ndcg@10", "ndcg@20"} and all(0 <= v <= 1 for v in full.values())
    I = pkg.evaluation.export_item_embeddings(m, feats, ei, edge_attr=ea)
    assert np.array_equal(I, Z[n_users:].cpu().numpy())


def test_trainer_flag_none_is_the_default_run(pkg, cuda, tmp_path):
    _, a, _ = _train_child(tmp_path, epochs=1, samples=5000)  # one after the other
    _, b, _ = _train_child(tmp_path, "--edge-features", "none", epochs=1, samples=5000)
    assert a["config"]["edge_features"] == b["config"]["edge_features"] == "none"
    strip = lambda r: {k: v for k, v in r.items() if k != "config"} | {
        "config": {k: v for k, v in r["config"].items() if k != "models_prefix"}}
    assert strip(a) == strip(b)
