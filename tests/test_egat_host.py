"""GATConv edge features without a GPU: the float64 reference (tests/_egat_ref.py) anchored to the
pinned restatement (oracle.gat_oracle.pyg_gat_conv) and to autograd, the collapse of lin_edge and
att_edge to v, the LeakyReLU-kink condition the GPU parity cases rely on, the constructor and
state_dict, the rating edge features, the trainer's options and the new ABI entries' argument
checks -- CPU."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import _egat_ref as ref

N = ref.N_NODES


def _rel(a, b):
    return ref.rel(a, b)


@pytest.fixture(scope="module")
def graph():
    ei = ref.make_graph()
    assert N == 900 and 6500 <= ei.shape[1] <= 7100
    return ei


def _mask(E, H, p=0.3, seed=5):
    from oracle import gat_oracle
    return torch.from_numpy(np.stack([gat_oracle.dropout_scale(seed, np.arange(E), h, p) for h in range(H)], 1))


@pytest.mark.parametrize("H,C,D", [(1, 32, 3), (2, 64, 1)])
def test_zero_att_edge_is_the_pinned_layer(oracle, graph, H, C, D):
    """att_edge = 0: out and every gradient of the new reference equal oracle.pyg_gat_conv's, with
    and without dropout; the edge parameters' own gradients: lin_edge's is zero, att_edge's is not."""
    P = ref.inputs(N, graph.shape[1], H, C, D)
    P["att_edge"] = np.zeros_like(P["att_edge"])
    ei = torch.from_numpy(graph)
    for p, seed in ((0.0, 0), (0.3, 5)):
        mask = _mask(graph.shape[1], H, p, seed) if p > 0 else None
        got = ref.autograd_grads(P, graph, H, 0.2, mask)
        L = {k: torch.from_numpy(P[k]).double().requires_grad_(True) for k in ("x", "W", "att_src", "att_dst", "bias")}
        out = oracle.pyg_gat_conv(L["x"], ei, L["W"], L["att_src"], L["att_dst"], L["bias"], H, dropout_p=p, seed=seed)
        (out * torch.from_numpy(P["G"]).double()).sum().backward()
        assert _rel(got["out"], out) <= 1e-12
        for k, g in (("x", "dx"), ("W", "dW"), ("att_src", "datt_src"), ("att_dst", "datt_dst"), ("bias", "dbias")):
            assert _rel(got[g], L[k].grad) <= 1e-12, (g, p)
        assert float(got["dlin_edge"].abs().max()) == 0.0 and float(got["datt_edge"].abs().max()) > 0.0


@pytest.mark.parametrize("H,C,D", [(1, 32, 1), (2, 64, 3), (4, 128, 3)])
def test_formulas_equal_autograd_and_collapse(graph, H, C, D):
    """The explicit formulas (dv, dlin_edge, datt_edge included) against float64 autograd through the
    un-collapsed layer, <= 1e-10; edge_attr @ v.T against the un-collapsed logit term, <= 1e-12."""
    P = ref.inputs(N, graph.shape[1], H, C, D)
    for mask in (None, _mask(graph.shape[1], H)):
        a, f = ref.autograd_grads(P, graph, H, 0.2, mask), ref.formulas(P, graph, H, 0.2, mask)
        for k in ("out",) + ref.GRADS:
            assert _rel(f[k].reshape(a[k].shape), a[k]) <= 1e-10, (k, _rel(f[k].reshape(a[k].shape), a[k]))
        assert _rel(f["a_e_collapsed"], f["a_e"]) <= 1e-12
        assert float(f["dv"].abs().max()) > 0


@pytest.mark.parametrize("H,C,D", ref.CASES)
def test_no_logit_near_the_kink(graph, H, C, D):
    """The condition of the GPU parity cases, from the float64 reference alone: every
    |z| >= 1e-5 (|s_src| + |s_dst| + |a_e|), so the fp32 sum of the three terms (relative error of
    a few 2^-24 of that magnitude) cannot land on the other side of the LeakyReLU kink."""
    f = ref.formulas(ref.inputs(N, graph.shape[1], H, C, D), graph, H)
    print(f"kink_ratio h{H} c{C} d{D}: {f['kink_ratio']:.3e}")
    assert f["kink_ratio"] >= 1e-5, f["kink_ratio"]


def test_recipe_draw_order():
    """x first, edge_attr last and uniform in [0, 1)."""
    P = ref.inputs(50, 70, 2, 64, 3)
    rng = np.random.default_rng(1)
    assert np.array_equal(P["x"], (0.5 * rng.standard_normal((50, 128))).astype(np.float32))
    assert list(P) == list(ref.NAMES) and P["edge_attr"].shape == (70, 3) and P["edge_attr"].dtype == np.float32
    assert 0.0 <= P["edge_attr"].min() and P["edge_attr"].max() < 1.0 and P["lin_edge"].shape == (128, 3)


def test_constructor_and_state_dict(pkg):
    kw = dict(heads=2, concat=False, add_self_loops=False)
    torch.manual_seed(3)
    conv = pkg.GATConv(128, 64, edge_dim=3, **kw)
    torch.manual_seed(3)
    plain = pkg.GATConv(128, 64, **kw)
    sd = conv.state_dict()
    assert set(sd) == {"att_src", "att_dst", "bias", "att_edge", "lin.weight", "lin_edge.weight"}
    assert tuple(sd["lin_edge.weight"].shape) == (128, 3) and tuple(sd["att_edge"].shape) == (1, 2, 64)
    assert conv.edge_dim == 3 and plain.edge_dim is None
    # the other keys and their seeded values are those of the layer without edge_dim
    psd = plain.state_dict()
    assert set(psd) == set(sd) - {"lin_edge.weight", "att_edge"}
    for k, v in psd.items():
        assert torch.equal(v, sd[k]), k
    # glorot: U(+-sqrt(6 / (fan_in + fan_out))) on the last two dimensions
    assert float(sd["lin_edge.weight"].abs().max()) <= (6.0 / (128 + 3)) ** 0.5
    assert float(sd["att_edge"].abs().max()) <= (6.0 / (2 + 64)) ** 0.5 and float(sd["att_edge"].abs().max()) > 0
    other = pkg.GATConv(128, 64, edge_dim=3, **kw)
    other.load_state_dict(sd)
    assert all(torch.equal(v, other.state_dict()[k]) for k, v in sd.items())
    with pytest.raises(RuntimeError):  # strict: the edge keys are required
        other.load_state_dict(psd)
    assert pkg.GATConv(8, 8, edge_dim=16, heads=1, concat=False, add_self_loops=False).lin_edge.weight.shape == (8, 16)
    with pytest.raises(NotImplementedError):
        pkg.GATConv(128, 64, edge_dim=17, **kw)
    with pytest.raises(NotImplementedError):  # out of scope: stays as it was
        pkg.GATv2Conv(128, 64, edge_dim=4, **kw)


def test_edge_attr_argument_checks(pkg):
    """edge_attr is checked before any device work: wrong dtype / device / rows raise ValueError
    naming the argument, requires_grad and D > 16 NotImplementedError."""
    hip_ops = importlib.import_module(pkg.__name__ + ".hip_ops")
    cpu = torch.device("cpu")
    ok = torch.zeros(10, 2)
    assert hip_ops.check_edge_attr(ok, 10, cpu) is ok and hip_ops.check_edge_attr(torch.zeros(10), 10, cpu).dim() == 1
    for bad in (torch.zeros(10, 2, dtype=torch.float64), torch.zeros(9, 2), torch.zeros(10, 2, 1), [0.0] * 10):
        with pytest.raises(ValueError, match="edge_attr"):
            hip_ops.check_edge_attr(bad, 10, cpu)
    with pytest.raises(ValueError, match="edge_attr"):
        hip_ops.check_edge_attr(ok, 10, torch.device("cuda:0"))
    with pytest.raises(NotImplementedError, match="requires_grad"):
        hip_ops.check_edge_attr(torch.zeros(10, 2, requires_grad=True), 10, cpu)
    with pytest.raises(NotImplementedError):
        hip_ops.check_edge_attr(torch.zeros(10, 17), 10, cpu)
    with pytest.raises(NotImplementedError, match="aggregate-then-transform"):
        hip_ops.gat_layer_x(None, None, None, None, None, None, 2, 128, 0.2, edge_v=ok, edge_attr=ok)


def test_model_takes_edge_dim(pkg):
    m = pkg.PyGGAT(7, 5, item_feat_dim=12, hidden=64, layers=2, heads=2, attn_dropout=0.1, edge_dim=1)
    keys = set(m.state_dict())
    assert {"convs.0.lin_edge.weight", "convs.0.att_edge", "convs.1.lin_edge.weight", "convs.1.att_edge"} <= keys
    assert tuple(m.convs[1].lin_edge.weight.shape) == (128, 1)
    plain = pkg.PyGGAT(7, 5, item_feat_dim=12, hidden=64, layers=2, heads=2, attn_dropout=0.1)
    assert not any("edge" in k for k in plain.state_dict())


def test_edge_attr_rating_follows_build_edge_index(pkg):
    """Columns 2t and 2t + 1 carry (r - 1) / 4 of train interaction t, found here from the
    interactions frame on its own."""
    data = pkg.data
    inter = data.synthetic_interactions_small(seed=0)
    maps = data.node_maps_from_interactions(inter)
    u2i, i2i = data.index_maps(maps)
    tr, _, _ = data.map_splits_to_index(*data.build_splits(inter), u2i, i2i)
    n_users, n_items = int(maps["n_users"]), int(maps["n_items"])
    ei = data.build_edge_index(n_users, n_items, tr).numpy()
    ea = data.edge_attr_rating(tr, inter, u2i, i2i)
    assert ea.dtype == np.float32 and ea.shape == (ei.shape[1], 1)
    assert set(np.unique(ea).tolist()) <= {0.0, 0.25, 0.5, 0.75, 1.0} and len(np.unique(ea)) == 5
    assert np.array_equal(ea[0::2], ea[1::2])
    # independent lookup: the (user, item) pairs that occur once in the frame
    raw_u = {v: k for k, v in u2i.items()}
    raw_i = {v: k for k, v in i2i.items()}
    s_u, s_i = inter["user_id"].astype(str), inter["asin"].astype(str)
    checked = 0
    for t in np.random.default_rng(0).permutation(ei.shape[1] // 2)[:200].tolist():
        u, it = int(ei[0, 2 * t]), int(ei[1, 2 * t]) - n_users
        assert (int(ei[1, 2 * t + 1]), int(ei[0, 2 * t + 1]) - n_users) == (u, it)
        row = inter[(s_u == raw_u[u]) & (s_i == raw_i[it])]
        if len(row) != 1:
            continue
        want = np.float32((float(row["rating"].iloc[0]) - 1.0) / 4.0)
        assert ea[2 * t, 0] == want and ea[2 * t + 1, 0] == want
        checked += 1
    assert checked >= 20
    # no rating column: 1.0 per edge, as build_ui_edges
    ones = data.edge_attr_rating(tr, inter.drop(columns=["rating"]), u2i, i2i)
    assert ones.shape == ea.shape and bool((ones == 1.0).all())
    assert data.edge_attr_rating(tr).shape == ea.shape


def test_edge_attr_rating_repeated_pairs_and_unmapped_rows(pkg):
    """A (user, item) pair that occurs more than once is matched in (ts, row) order, whatever the
    frame's row order; rows whose ids are not in the node maps are passed over."""
    import pandas as pd
    data = pkg.data
    inter = pd.DataFrame({
        "user_id": ["b", "a", "a", "a", "a", "a", "zz", "b", "b"],
        "asin":    ["y", "x", "w", "x", "z", "y", "x", "x", "q"],
        "ts":      [1,   3,   5,   1,   4,   2,   0,   2,   3],
        "rating":  [2.0, 3.0, 4.0, 5.0, 2.0, 1.0, 4.0, 4.0, 1.0]})
    u2i, i2i = {"a": 0, "b": 1}, {"x": 0, "y": 1, "z": 2, "w": 3, "q": 4}
    # user a in ts order: x(5) y(1) x(3) z(2) w(4): train is the first three; user b: y(2) x(4) q(1): train y
    tr, va, te = data.map_splits_to_index(*data.build_splits(inter[inter["user_id"] != "zz"]), u2i, i2i)
    assert tr[0].tolist() == [0, 1, 0] and tr[1].tolist() == [1]
    ea = data.edge_attr_rating(tr, inter, u2i, i2i)
    want = {0: [5.0, 1.0, 3.0], 1: [2.0]}
    flat = np.array([r for u in tr for r in want[u]], np.float32)
    assert np.array_equal(ea[:, 0], np.repeat((flat - 1) / 4, 2))
    with pytest.raises(KeyError):
        data.edge_attr_rating({0: np.array([4])}, inter, u2i, i2i)
    assert data.edge_attr_rating({}, inter, u2i, i2i).shape == (0, 1)


def test_trainer_options(pkg):
    train = importlib.import_module(pkg.__name__ + ".train")
    assert train.build_parser().parse_args([]).edge_features == "none"
    assert train.build_parser().parse_args(["--edge-features", "rating"]).edge_features == "rating"
    for extra, word in ((["--world-size", "2"], "world-size"), (["--model-family", "gatv2_pyg"], "gatv2_pyg"),
                        (["--model-family", "lightgcn"], "lightgcn"), (["--model-family", "gat_custom"], "gat_custom")):
        with pytest.raises(NotImplementedError, match=word):
            train.main(["--edge-features", "rating", "--synthetic", "cfg1"] + extra)
    cfg = train.Config("p", "r", "s", "g", "e", "m", hidden_dim=64, layers=1, edge_features="rating")
    assert cfg.__dict__["edge_features"] == "rating" and train.Config("p", "r", "s", "g", "e", "m").edge_features == "none"
    assert train.build_model(cfg, 7, 5, 12).convs[0].edge_dim == 1
    assert train.load_edge_attr(train.Config("p", "r", "s", "g", "e", "m"), "cfg1", {}) is None


def test_abi_return_codes(pkg):
    """The new entries validate their arguments before any device work."""
    lib = pkg._lib.load()
    assert lib.ppgat_edge_dv_partial_rows(0) == 1 and lib.ppgat_edge_dv_partial_rows(-1) == -1
    assert lib.ppgat_edge_dv_partial_rows(2_608_620) == lib.ppgat_edge_dv_partial_rows(2_608_620) <= 1024
    p = ctypes.c_void_p(16)
    assert lib.ppgat_edge_attr_permute(p, p, 10, 17, p, None) == 2 and b"edge_dim" in lib.ppgat_last_error()
    assert lib.ppgat_edge_attr_permute(None, p, 10, 3, p, None) == 1
    assert lib.ppgat_edge_terms(p, p, p, 10, 17, 1, p, p, None) == 2
    assert lib.ppgat_edge_terms(p, p, p, 10, 3, 9, p, p, None) == 1
    assert lib.ppgat_edge_terms(p, None, p, 10, 3, 1, p, p, None) == 1  # t_csc needs attr_csc
    assert lib.ppgat_edge_dv(p, p, 10, 1, 17, p, p, None) == 2
    assert lib.ppgat_edge_dv(None, p, 10, 1, 3, p, p, None) == 1
    rc = lib.ppgat_edge_fwd(None, None, None, None, 10, 5, 1, 128, None, None, None, None, 0, 0.2, 0.0, 0, None, None,
                            None, None, None, None, 0, None)
    assert rc == 1 and b"edge_term" in lib.ppgat_last_error()
    rc = lib.ppgat_edge_bwd_edges(None, None, None, None, None, 5, 1, 128, None, None, None, None, 0, 0.2, 0.0, 0, None,
                                  None, 128, None, 1, None, None, 0, None)
    assert rc == 1 and b"edge_term" in lib.ppgat_last_error()
