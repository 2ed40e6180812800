"""Seed-subgraph sampling on the GPU (csrc/ppgat_subgraph.hip, neighbors.py, model.forward_subgraph):
every output equals the numpy reference bit for bit, the derived graph equals csr_build of its own
edge_index, the edge cases, the equivalence with the existing whole-graph forward at the seeds, the
trainer.  The extraction is integers throughout: no tolerance there."""
import importlib
import json
import re

import numpy as np
import pytest
import torch

import _subgraph_ref as ref
from conftest import row_rel

pytestmark = pytest.mark.gpu

N = ref.N
OUT_TOL, ATT_TOL = 2e-5, 2e-4  # two fp32 paths, each pinned to the fp64 oracle at 1e-5 (1e-4: attention vectors)
GRAPH_ARRAYS = ["rowptr", "col", "csr_eid", "colptr", "row", "csc_eid", "csc2csr", "csr2csc"]


def _sched_equal(a, b):
    assert (a.n_items, a.n_hub_items, a.n_hubs, a.max_edges, a.n_long_items) == \
        (b.n_items, b.n_hub_items, b.n_hubs, b.max_edges, b.n_long_items)
    for name in ("item_row", "item_beg", "item_end"):
        assert torch.equal(getattr(a, name)[:a.n_items], getattr(b, name)[:a.n_items]), name
    assert torch.equal(a.hub_row[:a.n_hubs], b.hub_row[:a.n_hubs])
    assert torch.equal(a.hub_ptr[:a.n_hubs + 1], b.hub_ptr[:a.n_hubs + 1])


def _graph_equal(gs, gb):
    assert (gs.n_nodes, gs.n_edges) == (gb.n_nodes, gb.n_edges)
    for name in GRAPH_ARRAYS:
        a, b = getattr(gs, name), getattr(gb, name)
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), name
    _sched_equal(gs.fwd_sched, gb.fwd_sched)
    _sched_equal(gs.bwd_sched, gb.bwd_sched)


@pytest.fixture(scope="module")
def graphs(pkg, cuda):
    """F -> (edge_index numpy, edge_index tensor, parent graph), built once."""
    out = {}
    for F in sorted({c[0] for c in ref.CASES}):
        ei_np = ref.graph(F)
        ei = torch.from_numpy(ei_np).to(cuda)
        out[F] = (ei_np, ei, pkg.hip_ops.csr_build(ei, N))
    return out


def _dev(a, cuda, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a if dtype is None else np.asarray(a, dtype))).to(cuda)


def _equal_ref(pkg, sub, want):
    assert sub.n_id.dtype == torch.int64 and sub.depth.dtype == torch.int32 and sub.eid.dtype == torch.int64
    assert sub.edge_index_s.dtype == torch.int64 and sub.seed_local.dtype == torch.int64
    assert np.array_equal(sub.n_id.cpu().numpy(), want["n_id"])
    assert np.array_equal(sub.depth.cpu().numpy(), want["depth"])
    assert sub.n_users_s == want["n_users_s"]
    assert sub.edge_index_s.shape == want["edge_index_s"].shape
    assert np.array_equal(sub.edge_index_s.cpu().numpy(), want["edge_index_s"])
    assert np.array_equal(sub.eid.cpu().numpy(), want["eid"])
    assert np.array_equal(sub.seed_local.cpu().numpy(), want["seed_local"])
    assert (sub.n_nodes, sub.n_edges) == (len(want["n_id"]), len(want["eid"]))
    _graph_equal(sub.graph_s, pkg.hip_ops.csr_build(sub.edge_index_s.clone(), sub.n_nodes))


def _subs_equal(a, b):
    for name in ("n_id", "depth", "edge_index_s", "eid", "seed_local"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert a.n_users_s == b.n_users_s
    _graph_equal(a.graph_s, b.graph_s)


# ---- exactness ------------------------------------------------------------------------
@pytest.mark.parametrize("seed", ref.SEEDS, ids=["seed42", "seed2^64-3"])
@pytest.mark.parametrize("F,L", [c[:2] for c in ref.CASES])
def test_cases_equal_reference_and_csr_build(pkg, graphs, cuda, F, L, seed):
    ei_np, ei, g = graphs[F]
    sub = pkg.sample_subgraph(ei, N, _dev(ref.seeds16(), cuda), L, F, seed, n_users=ref.N_USERS, graph=g)
    _equal_ref(pkg, sub, ref.case(F, L, seed))
    # a restriction of the whole sampled graph: the kept edges are among sample_neighbors'
    _, eid_all, _ = pkg.sample_neighbors(ei, N, F, seed, graph=g)
    assert torch.isin(sub.eid, eid_all).all()


def test_per_node_caps(pkg, graphs, cuda):
    ei_np, ei, g = graphs[7]
    rng = np.random.default_rng(11)
    seeds = ref.seeds16()
    for fo in (np.zeros(N), np.full(N, -1), rng.integers(-1, 65, N)):
        fo = fo.astype(np.int32)
        if fo.min() < fo.max():  # the mixed one: a sampled row at the maximum, the hub kept whole, a seed at 0
            fo[14], fo[ref.HUB], fo[5] = 64, -1, 0
        sub = pkg.sample_subgraph(ei, N, _dev(seeds, cuda), 2, 7, 42, fanout_of=_dev(fo, cuda), n_users=ref.N_USERS,
                                  graph=g)
        _equal_ref(pkg, sub, ref.subgraph(ei_np, N, seeds, 2, 7, 42, fanout_of=fo, n_users=ref.N_USERS))
        if fo[ref.HUB] < 0:  # the hub kept whole: its row is cut into hub pieces in the sub-schedule
            hub_local = int(np.searchsorted(sub.n_id.cpu().numpy(), ref.HUB))
            assert sub.graph_s.in_degree()[hub_local] >= ref.HUB_DEGREE and sub.graph_s.fwd_sched.n_hubs >= 1
        if not fo.any():
            assert sub.n_edges == 0 and sub.n_nodes == 15
    fo = np.full(N, 5, np.int32)
    fo[17] = 65  # not a node of the subgraph: refused all the same
    with pytest.raises(ValueError, match="fanout_of"):
        pkg.sample_subgraph(ei, N, _dev(seeds, cuda), 2, 7, 42, fanout_of=_dev(fo, cuda), graph=g)


def test_seed_order_and_duplicates_do_not_change_the_subgraph(pkg, graphs, cuda):
    ei_np, ei, g = graphs[7]
    seeds = ref.seeds16()
    a = pkg.sample_subgraph(ei, N, _dev(seeds, cuda), 2, 7, 42, n_users=ref.N_USERS, graph=g)
    other = np.concatenate([seeds[::-1], seeds[3:9], seeds[:1]])
    b = pkg.sample_subgraph(ei, N, _dev(other, cuda), 2, 7, 42, n_users=ref.N_USERS, graph=g)
    for name in ("n_id", "depth", "edge_index_s", "eid"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    _graph_equal(a.graph_s, b.graph_s)
    assert np.array_equal(b.n_id[b.seed_local].cpu().numpy(), other)
    assert torch.equal(a.localize(_dev(other, cuda)), b.seed_local)
    with pytest.raises(ValueError, match="not nodes"):
        a.localize(_dev(np.array([4, 2999]), cuda))  # 2999 is isolated and no seed


def test_refusals(pkg, graphs, cuda):
    ei_np, ei, g = graphs[7]
    for bad in (N, -1, 1 << 40):
        seeds = ref.seeds16().copy()
        seeds[7] = bad
        with pytest.raises(ValueError, match="seeds"):
            pkg.sample_subgraph(ei, N, _dev(seeds, cuda), 2, 7, 42, graph=g)
    s = _dev(ref.seeds16(), cuda)
    for hops in (-1, 9):
        with pytest.raises(ValueError, match="hops"):
            pkg.sample_subgraph(ei, N, s, hops, 7, 42, graph=g)
    for fanout in (0, 65):
        with pytest.raises(NotImplementedError):
            pkg.sample_subgraph(ei, N, s, 2, fanout, 42, graph=g)
    with pytest.raises(RuntimeError):
        pkg.sample_subgraph(ei, N, s.int(), 2, 7, 42, graph=g)


def test_two_calls_give_the_same_bits(pkg, graphs, cuda):
    ei_np, ei, g = graphs[7]
    s = _dev(ref.seeds16(), cuda)
    a = pkg.sample_subgraph(ei, N, s, 2, 7, 5, n_users=ref.N_USERS, graph=g)
    b = pkg.sample_subgraph(ei, N, s, 2, 7, 5, n_users=ref.N_USERS, graph=g)
    _subs_equal(a, b)
    c = pkg.sample_subgraph(ei, N, s, 2, 7, 6, n_users=ref.N_USERS, graph=g)
    assert not (c.eid.shape == a.eid.shape and torch.equal(a.eid, c.eid))


def test_zero_hops_empty_and_isolated_seeds(pkg, graphs, cuda):
    ei_np, ei, g = graphs[7]
    z = pkg.sample_subgraph(ei, N, _dev(ref.seeds16(), cuda), 0, 7, 42, n_users=ref.N_USERS, graph=g)
    _equal_ref(pkg, z, ref.subgraph(ei_np, N, ref.seeds16(), 0, 7, 42, n_users=ref.N_USERS))
    assert z.n_nodes == 15 and z.n_edges == 0
    e = pkg.sample_subgraph(ei, N, torch.zeros(0, dtype=torch.int64, device=cuda), 2, 7, 42, n_users=ref.N_USERS,
                            graph=g)
    assert e.n_nodes == 0 and e.n_edges == 0 and e.n_users_s == 0 and e.seed_local.numel() == 0
    assert e.edge_index_s.shape == (2, 0) and e.graph_s.rowptr.tolist() == [0] and e.graph_s.colptr.tolist() == [0]
    iso = np.array([2999, 2900, N - 1, 2999], np.int64)
    s = pkg.sample_subgraph(ei, N, _dev(iso, cuda), 2, 7, 42, n_users=ref.N_USERS, graph=g)
    _equal_ref(pkg, s, ref.subgraph(ei_np, N, iso, 2, 7, 42, n_users=ref.N_USERS))
    assert s.n_nodes == 3 and s.n_edges == 0


def test_guard_elements_are_untouched(pkg, graphs, cuda):
    """The launches into oversized buffers: everything past an output's stated length keeps its
    fill, and what lies before equals sample_subgraph's."""
    launch = importlib.import_module(pkg.__name__ + "._launch")
    ei_np, ei, g = graphs[7]
    PAD, FILL, F, L = 64, -7, 7, 2
    seeds = _dev(ref.seeds16(), cuda)
    want = pkg.sample_subgraph(ei, N, seeds, L, F, 42, n_users=ref.N_USERS, graph=g)
    Ns, Es, T = want.n_nodes, want.n_edges, seeds.numel()

    def buf(n, dtype=torch.int32):
        return torch.full((n + PAD,), FILL, dtype=dtype, device=cuda)

    (sws, sbytes), (nws, nbytes) = pkg.neighbors.subgraph_workspace(N, g.n_edges, cuda)
    info, cap, rowptr_p, colptr_p = buf(6), buf(N), buf(N + 1), buf(N + 1)
    launch.subgraph_seed(seeds, N, info[2:], sws, sbytes)
    for hop in range(L):
        launch.subgraph_expand(g, hop, F, None, 42, sws, sbytes)
    launch.subgraph_plan(N, ref.N_USERS, L, F, None, cap, info[2:], sws, sbytes)
    launch.neighbor_count(g, F, cap[:N], rowptr_p, info, nws, nbytes)
    assert info[:6].tolist() == [Es, 0, Ns, want.n_users_s, 0, 0] and (info[6:] == FILL).all()
    assert (cap[N:] == FILL).all() and int((cap[:N] == F).sum()) == int((want.depth < L).sum())
    col, csr_eid, row, csc_eid, csc2csr, csr2csc = (buf(Es) for _ in range(6))
    ei_s, eid = buf(2 * Es, torch.int64), buf(Es, torch.int64)
    launch.neighbor_sample(g, ei, 42, rowptr_p, Es, col, csr_eid, ei_s, eid, nws, nbytes)
    launch.neighbor_derive(g, Es, colptr_p, row, csc_eid, csc2csr, csr2csc, nws, nbytes)
    n_id, depth, seed_local = buf(Ns, torch.int64), buf(Ns), buf(T, torch.int64)
    rowptr_s, colptr_s = buf(Ns + 1), buf(Ns + 1)
    launch.subgraph_relabel(N, Ns, Es, seeds, rowptr_p, colptr_p, n_id, depth, rowptr_s, colptr_s, col, row, ei_s,
                            seed_local, sws, sbytes)
    torch.cuda.synchronize()
    gs = want.graph_s
    got = {"rowptr": (rowptr_s, gs.rowptr), "colptr": (colptr_s, gs.colptr), "col": (col, gs.col), "row": (row, gs.row),
           "csr_eid": (csr_eid, gs.csr_eid), "csc_eid": (csc_eid, gs.csc_eid), "csc2csr": (csc2csr, gs.csc2csr),
           "csr2csc": (csr2csc, gs.csr2csc), "n_id": (n_id, want.n_id), "depth": (depth, want.depth),
           "seed_local": (seed_local, want.seed_local), "eid": (eid, want.eid),
           "edge_index_s": (ei_s, want.edge_index_s.reshape(-1))}
    for name, (t, w) in got.items():
        assert torch.equal(t[:w.numel()], w), name
        assert (t[w.numel():] == FILL).all() and t.numel() == w.numel() + PAD, name
    assert (rowptr_p[N + 1:] == FILL).all() and (colptr_p[N + 1:] == FILL).all()


# ---- the sampler object, the graph cache, edge attributes ---------------------------------------
def test_sampler_batches_follow_their_seeds_and_leave_one_cache_entry(pkg, graphs, cuda):
    ei_np, ei, _ = graphs[7]
    cache = pkg.hip_ops.graph_cache
    cache.clear()
    smp = pkg.SubgraphSampler(ei, N, 2, 7, seed=42, n_users=ref.N_USERS)
    seeds = ref.seeds16()
    subs = []
    nb = pkg.neighbors
    for epoch, b in ((0, 0), (0, 1), (1, 0)):
        sub = smp.batch(epoch, b, _dev(seeds, cuda))
        s = nb.epoch_seed(nb.epoch_seed(42, epoch), b)
        _equal_ref(pkg, sub, ref.subgraph(ei_np, N, seeds, 2, 7, s, n_users=ref.N_USERS))
        assert cache.get(sub.edge_index_s, sub.n_nodes) is sub.graph_s  # found, not rebuilt
        subs.append(sub)
    assert not torch.equal(subs[0].eid, subs[1].eid) and not torch.equal(subs[1].eid, subs[2].eid)
    held = [t for _, t, _ in cache.entries]
    assert any(h is ei for h in held) and any(h is subs[2].edge_index_s for h in held)
    assert sum(any(h is s.edge_index_s for s in subs) for h in held) == 1  # one subgraph entry after three batches
    cache.clear()


def test_edge_attributes_follow_eid(pkg, graphs, cuda):
    ei_np, ei, g = graphs[7]
    ea_np = np.random.default_rng(8).random((ei_np.shape[1], 1)).astype(np.float32)
    sub = pkg.sample_subgraph(ei, N, _dev(ref.seeds16(), cuda), 2, 7, 42, n_users=ref.N_USERS, graph=g)
    want = ref.case(7, 2, 42)
    assert np.array_equal(_dev(ea_np, cuda).index_select(0, sub.eid).cpu().numpy(), ea_np[want["eid"]])


# ---- equivalence with the whole-graph forward at the seeds ----------------------------------------
FEAT, HIDDEN = 32, 32
KINDS = ["gat", "gatv2", "custom"]


def _model(pkg, kind, n_users, n_items, cuda, edge_dim=None):
    torch.manual_seed(5)
    if kind == "gat":
        m = pkg.PyGGAT(n_users, n_items, FEAT, HIDDEN, 2, 2, 0.3, edge_dim=edge_dim)
    elif kind == "gatv2":
        m = pkg.PyGGATv2(n_users, n_items, FEAT, HIDDEN, 2, 1, 0.3)
    else:
        m = pkg.CustomGAT(n_users, n_items, FEAT, HIDDEN, 2)
    with torch.no_grad():  # PyG's zero biases would leave an isolated seed's row at zero
        for name, p in m.named_parameters():
            if name.endswith("bias"):
                p.normal_(std=0.1)
    return m.to(cuda).eval()


def _grads(model, Z, rows, G):
    model.zero_grad()
    (Z.index_select(0, rows) * G).sum().backward()
    return {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}


def _compare(tag, Zs, gs, Zf, gf, figures):
    rel, row, zmax = row_rel(Zs, Zf)
    print(f"[{tag}] seed rows: max row-relative difference {rel:.3e} (row {row}), zero rows {zmax:.1e}")
    figures[tag + ".out"] = rel
    assert row >= 0 and rel <= OUT_TOL and zmax == 0.0  # (row < 0: no nonzero reference row to compare)
    assert set(gs) == set(gf) and len(gf) >= 6
    for k in sorted(gf):
        a, b = gs[k].double(), gf[k].double()
        scale = float(b.abs().max())
        err = float((a - b).abs().max()) / max(scale, 1e-300)
        tol = ATT_TOL if "att" in k else OUT_TOL
        print(f"[{tag}] d{k}: {err:.3e} of {scale:.3e} (bound {tol:.0e})")
        figures[f"{tag}.d{k}"] = err
        assert scale > 0 and err <= tol, (k, err)


@pytest.mark.parametrize("kind", KINDS)
def test_seed_rows_equal_the_sampled_whole_graph_forward(pkg, graphs, cuda, kind):
    ei_np, ei, g = graphs[7]
    F, L, seed = 7, 2, 42
    cache = pkg.hip_ops.graph_cache
    cache.clear()
    model = _model(pkg, kind, ref.N_USERS, ref.N_ITEMS, cuda)
    feats = torch.randn(ref.N_ITEMS, FEAT, device=cuda)
    seeds = _dev(np.unique(ref.seeds16()), cuda)
    G = torch.randn(seeds.numel(), HIDDEN, device=cuda)
    sub = pkg.sample_subgraph(ei, N, seeds, L, F, seed, n_users=ref.N_USERS, graph=g)
    ei_sampled, _, _ = pkg.sample_neighbors(ei, N, F, seed, graph=g)
    Zf = model(feats, ei_sampled)
    gf = _grads(model, Zf, seeds, G)
    Zs = model.forward_subgraph(feats, sub)
    assert Zs.shape == (sub.n_nodes, HIDDEN)
    gs = _grads(model, Zs, sub.seed_local, G)
    figures = {}
    _compare(f"{kind}.sampled", Zs.index_select(0, sub.seed_local), gs, Zf.index_select(0, seeds), gf, figures)
    cache.clear()


@pytest.mark.parametrize("kind", KINDS)
def test_fanout_at_least_the_largest_degree_equals_the_full_graph(pkg, cuda, kind):
    rng = np.random.default_rng(3)
    nu, ni = 300, 200
    du, di = rng.integers(0, 40, nu), rng.integers(0, 65, ni)
    du[:2], di[:3] = [0, 39], [64, 0, 63]
    ei_np = np.concatenate([np.stack([nu + rng.integers(0, ni, du.sum()), np.repeat(np.arange(nu), du)]),
                            np.stack([rng.integers(0, nu, di.sum()), nu + np.repeat(np.arange(ni), di)])], axis=1)
    ei_np = np.ascontiguousarray(ei_np[:, rng.permutation(ei_np.shape[1])])
    assert np.bincount(ei_np[1], minlength=nu + ni).max() == 64
    ei = _dev(ei_np, cuda)
    cache = pkg.hip_ops.graph_cache
    cache.clear()
    model = _model(pkg, kind, nu, ni, cuda)
    feats = torch.randn(ni, FEAT, device=cuda)
    seeds = _dev(np.array([0, 1, 7, 150, 299, nu, nu + 1, nu + 2, nu + 100, nu + 199]), cuda)
    G = torch.randn(seeds.numel(), HIDDEN, device=cuda)
    sub = pkg.sample_subgraph(ei, nu + ni, seeds, 2, 64, 42, n_users=nu)
    want = ref.subgraph(ei_np, nu + ni, seeds.cpu().numpy(), 2, 64, 42, n_users=nu)
    assert want["keep"].all()
    _equal_ref(pkg, sub, want)
    Zf = model(feats, ei)
    gf = _grads(model, Zf, seeds, G)
    Zs = model.forward_subgraph(feats, sub)
    gs = _grads(model, Zs, sub.seed_local, G)
    _compare(f"{kind}.full", Zs.index_select(0, sub.seed_local), gs, Zf.index_select(0, seeds), gf, {})
    cache.clear()


def test_edge_features_reach_the_subgraph_through_eid(pkg, graphs, cuda):
    ei_np, ei, g = graphs[7]
    cache = pkg.hip_ops.graph_cache
    cache.clear()
    model = _model(pkg, "gat", ref.N_USERS, ref.N_ITEMS, cuda, edge_dim=1)
    feats = torch.randn(ref.N_ITEMS, FEAT, device=cuda)
    edge_attr = torch.rand(ei.size(1), 1, device=cuda)
    seeds = _dev(np.unique(ref.seeds16()), cuda)
    G = torch.randn(seeds.numel(), HIDDEN, device=cuda)
    sub = pkg.sample_subgraph(ei, N, seeds, 2, 7, 42, n_users=ref.N_USERS, graph=g)
    ei_sampled, eid, _ = pkg.sample_neighbors(ei, N, 7, 42, graph=g)
    Zf = model(feats, ei_sampled, edge_attr.index_select(0, eid))
    gf = _grads(model, Zf, seeds, G)
    Zs = model.forward_subgraph(feats, sub, edge_attr)
    gs = _grads(model, Zs, sub.seed_local, G)
    _compare("gat.edge", Zs.index_select(0, sub.seed_local), gs, Zf.index_select(0, seeds), gf, {})
    cache.clear()


# ---- trainer ---------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [[], ["--edge-features", "rating"], ["--model-family", "gatv2_pyg"],
                                   ["--loss", "softmax"]], ids=["gat", "edge", "gatv2", "softmax"])
def test_trainer(pkg, cuda, tmp_path, capsys, monkeypatch, extra):
    train = importlib.import_module(pkg.__name__ + ".train")
    seen = []
    evaluate = train.evaluate
    monkeypatch.setattr(train, "evaluate", lambda args, model, cfg, feats, edge_index, *a, **k:
                        seen.append(int(edge_index.size(1))) or evaluate(args, model, cfg, feats, edge_index, *a, **k))
    capsys.readouterr()
    out = train.main(["--synthetic", "cfg1", "--epochs", "2", "--fanout", "5", "--subgraph-batch", "4096",
                      "--eval-neg-k", "100", "--device-eval", "--fast-sampler", "--structured-logs", "--models-prefix",
                      str(tmp_path)] + extra)
    log = capsys.readouterr().out
    ev = [json.loads(ln) for ln in log.splitlines() if ln.startswith("{")]
    ends = [e for e in ev if e["event"] == "epoch_end"]
    n_users, n_items = (int(v) for v in re.search(r"n_users=(\d+), n_items=(\d+)", log).groups())
    assert len(ends) == 2
    full = seen[0]
    assert len(seen) == 3 and seen == [full] * 3  # two validations and the test, all on the whole graph
    for e in ends:
        assert e["batches"] > 1 and 0 < e["mean_sub_nodes"] <= n_users + n_items
        assert 0 < e["mean_sub_edges"] <= 5 * (n_users + n_items) and "sampled_edges" not in e
    assert list((tmp_path / "checkpoints").glob("*.pt"))
    vals = list(out["test"].values()) + list(out["val"].values()) + [e["loss"] for e in ends]
    assert vals and all(np.isfinite(v) for v in vals), out
    assert "--subgraph-batch 4096" in out["notes"]
