"""Fan-out neighbour sampling on the GPU (csrc/ppgat_nsample.hip, neighbors.py): the sampled
edges equal the numpy reference bit for bit, every array of the derived graph equals csr_build of
the sampled edge_index, the edge cases, the wiring into the layers and the trainer.  Integers
throughout: no tolerance anywhere."""
import importlib
import json
import re

import numpy as np
import pytest
import torch

import _nsample_ref as ref

pytestmark = pytest.mark.gpu

FANOUTS = [1, 2, 7, 32, 63, 64]
SEEDS = [42, (1 << 64) - 3]
GRAPH_ARRAYS = ["rowptr", "col", "csr_eid", "colptr", "row", "csc_eid", "csc2csr", "csr2csc"]
N_LADDER = 320


def ladder(F: int):
    """In-degrees 0, 1, 2, F - 1, F, F + 1, 2F - 1, 2F, 63, 64, 65, 127, 128, 129, 1000, twenty times
    over (rows 0 .. 299: they straddle the 256-row block of the pick), one hub of 70,000 (row 300)
    and isolated nodes after it; random sources (repeated pairs included), columns shuffled so that
    edge ids interleave across rows."""
    rng = np.random.default_rng(100 + F)
    deg = np.zeros(N_LADDER, np.int64)
    deg[:300] = [0, 1, 2, F - 1, F, F + 1, 2 * F - 1, 2 * F, 63, 64, 65, 127, 128, 129, 1000] * 20
    deg[300] = 70000
    dst = np.repeat(np.arange(N_LADDER), deg)
    src = rng.integers(0, N_LADDER, len(dst))
    ei = np.stack([src, dst])[:, rng.permutation(len(dst))]
    assert len(np.unique(ei[0] * N_LADDER + ei[1])) < ei.shape[1]  # repeated (src, dst) pairs
    return np.ascontiguousarray(ei)


@pytest.fixture(scope="module")
def hip_ops(pkg):
    return pkg.hip_ops


@pytest.fixture(scope="module")
def ladders(pkg, cuda):
    """F -> (edge_index numpy, edge_index tensor, parent graph), built once."""
    out = {}
    for F in FANOUTS:
        ei_np = ladder(F)
        ei = torch.from_numpy(ei_np).to(cuda)
        out[F] = (ei_np, ei, pkg.hip_ops.csr_build(ei, N_LADDER))
    return out


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


def _check(pkg, ei_np, ei, n, fanout, seed, fanout_of=None, graph=None):
    """One sample against the reference and against csr_build of its own output."""
    fo = torch.from_numpy(np.asarray(fanout_of, np.int32)).to(ei.device) if fanout_of is not None else None
    ei_s, eid, gs = pkg.sample_neighbors(ei, n, fanout, seed, fanout_of=fo, graph=graph)
    _, want_ei, want_eid = ref.sample(ei_np, n, fanout, seed, fanout_of)
    assert ei_s.dtype == torch.int64 and eid.dtype == torch.int64 and ei_s.shape == (2, len(want_eid))
    assert np.array_equal(eid.cpu().numpy(), want_eid)
    assert np.array_equal(ei_s.cpu().numpy(), want_ei)
    _graph_equal(gs, pkg.hip_ops.csr_build(ei_s.clone(), n))
    return ei_s, eid, gs


# ---- exactness ------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS, ids=["seed42", "seed2^64-3"])
@pytest.mark.parametrize("F", FANOUTS)
def test_ladder_equals_reference_and_csr_build(pkg, ladders, F, seed):
    ei_np, ei, g = ladders[F]
    ei_s, eid, gs = _check(pkg, ei_np, ei, N_LADDER, F, seed, graph=g)
    deg = np.bincount(ei_np[1], minlength=N_LADDER)
    assert gs.n_edges == int(np.minimum(deg, F).sum()) < ei_np.shape[1]
    assert torch.equal(gs.in_degree().cpu(), torch.from_numpy(np.minimum(deg, F)).int())


def test_two_calls_give_the_same_bits(pkg, ladders):
    ei_np, ei, g = ladders[7]
    a = pkg.sample_neighbors(ei, N_LADDER, 7, 5, graph=g)
    b = pkg.sample_neighbors(ei, N_LADDER, 7, 5, graph=g)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    _graph_equal(a[2], b[2])
    c = pkg.sample_neighbors(ei, N_LADDER, 7, 6, graph=g)
    assert c[1].shape == a[1].shape and not torch.equal(a[1], c[1])


# ---- edge cases -----------------------------------------------------------------------
def test_fanout_at_least_the_largest_degree_keeps_the_graph(pkg, cuda):
    rng = np.random.default_rng(3)
    n = 300
    deg = rng.integers(0, 65, n)
    deg[:3] = [64, 0, 63]
    dst = np.repeat(np.arange(n), deg)
    ei_np = np.stack([rng.integers(0, n, len(dst)), dst])[:, rng.permutation(len(dst))]
    ei = torch.from_numpy(np.ascontiguousarray(ei_np)).to(cuda)
    ei_s, eid, gs = _check(pkg, ei_np, ei, n, 64, 42)
    assert torch.equal(ei_s, ei) and torch.equal(eid, torch.arange(ei.size(1), device=cuda))
    _graph_equal(gs, pkg.hip_ops.graph_cache.get(ei, n))


def test_no_edges(pkg, cuda):
    ei = torch.zeros(2, 0, dtype=torch.int64, device=cuda)
    ei_s, eid, gs = _check(pkg, np.zeros((2, 0), np.int64), ei, 5, 3, 42)
    assert ei_s.shape == (2, 0) and eid.shape == (0,) and gs.n_edges == 0
    assert not gs.rowptr.any() and not gs.colptr.any()


@pytest.mark.parametrize("F,kept", [(2, 2), (3, 3), (64, 3)])
def test_one_node_with_self_loops(pkg, cuda, F, kept):
    ei_np = np.zeros((2, 3), np.int64)
    ei_s, eid, gs = _check(pkg, ei_np, torch.from_numpy(ei_np).to(cuda), 1, F, 42)
    assert gs.n_edges == kept and gs.rowptr.tolist() == [0, kept]


def test_per_node_caps(pkg, ladders, cuda):
    ei_np, ei, g = ladders[7]
    rng = np.random.default_rng(9)
    deg = np.bincount(ei_np[1], minlength=N_LADDER)
    for fo in (np.zeros(N_LADDER), np.full(N_LADDER, -1), rng.integers(-1, 65, N_LADDER)):
        fo = fo.astype(np.int32)
        if fo.min() < fo.max():  # the mixed one: a sampled row at the maximum, the hub kept whole, a row at 0
            fo[14], fo[300], fo[29] = 64, -1, 0
        ei_s, eid, gs = _check(pkg, ei_np, ei, N_LADDER, 7, 42, fanout_of=fo, graph=g)
        want = np.where(fo >= 0, np.minimum(deg, fo), deg)
        assert torch.equal(gs.in_degree().cpu(), torch.from_numpy(want).int())
    assert gs.in_degree()[300] == 70000 and gs.in_degree()[14] == 64 and gs.fwd_sched.n_hubs >= 1
    fo = np.full(N_LADDER, 5, np.int32)
    fo[17] = 65
    with pytest.raises(ValueError, match="fanout_of"):
        pkg.sample_neighbors(ei, N_LADDER, 7, 42, fanout_of=torch.from_numpy(fo).to(cuda), graph=g)
    with pytest.raises(NotImplementedError):
        pkg.sample_neighbors(ei, N_LADDER, 65, 42, graph=g)
    with pytest.raises(NotImplementedError):
        pkg.sample_neighbors(ei, N_LADDER, 0, 42, graph=g)


def test_guard_elements_are_untouched(pkg, ladders, cuda):
    """The three launches into oversized buffers: everything past an output's stated length keeps
    its fill, and what lies before equals sample_neighbors'."""
    launch = importlib.import_module(pkg.__name__ + "._launch")
    ei_np, ei, g = ladders[7]
    N, PAD, FILL = N_LADDER, 64, -7
    want_ei, want_eid, want_g = pkg.sample_neighbors(ei, N, 7, 42, graph=g)
    Es = want_g.n_edges

    def buf(n, dtype=torch.int32):
        return torch.full((n + PAD,), FILL, dtype=dtype, device=cuda)

    ws, nbytes = launch.neighbor_workspace(N, g.n_edges, cuda)
    rowptr_s, info = buf(N + 1), buf(2)
    launch.neighbor_count(g, 7, None, rowptr_s, info, ws, nbytes)
    assert info[:2].tolist() == [Es, 0]
    col, csr_eid, row, csc_eid, csc2csr, csr2csc = (buf(Es) for _ in range(6))
    colptr, ei_s, eid = buf(N + 1), buf(2 * Es, torch.int64), buf(Es, torch.int64)
    launch.neighbor_sample(g, ei, 42, rowptr_s, Es, col, csr_eid, ei_s, eid, ws, nbytes)
    launch.neighbor_derive(g, Es, colptr, row, csc_eid, csc2csr, csr2csc, ws, nbytes)
    torch.cuda.synchronize()
    got = {"rowptr": rowptr_s, "col": col, "csr_eid": csr_eid, "colptr": colptr, "row": row, "csc_eid": csc_eid,
           "csc2csr": csc2csr, "csr2csc": csr2csc}
    for name, t in got.items():
        want = getattr(want_g, name)
        assert torch.equal(t[:want.numel()], want), name
        assert (t[want.numel():] == FILL).all() and t.numel() == want.numel() + PAD, name
    assert torch.equal(ei_s[:2 * Es].view(2, Es), want_ei) and (ei_s[2 * Es:] == FILL).all()
    assert torch.equal(eid[:Es], want_eid) and (eid[Es:] == FILL).all()
    assert (info[2:] == FILL).all()


# ---- the sampler object and the graph cache -------------------------------------------------
def test_epochs_differ_and_follow_their_seeds(pkg, hip_ops, ladders, cuda):
    ei_np, ei, _ = ladders[7]
    hip_ops.graph_cache.clear()
    smp = pkg.NeighborSampler(ei, N_LADDER, 7, seed=42)
    kept, tensors = [], []
    for e in range(3):
        ei_s, eid, gs = smp.epoch(e)
        _, want_ei, want_eid = ref.sample(ei_np, N_LADDER, 7, ref.epoch_seed(42, e))
        assert np.array_equal(eid.cpu().numpy(), want_eid) and np.array_equal(ei_s.cpu().numpy(), want_ei)
        assert hip_ops.graph_cache.get(ei_s, N_LADDER) is gs  # found, not rebuilt
        kept.append(eid)
        tensors.append(ei_s)
    assert not torch.equal(kept[0], kept[1]) and not torch.equal(kept[1], kept[2])
    held = [ref_t for _, ref_t, _ in hip_ops.graph_cache.entries]
    assert sum(any(t is h for t in tensors) for h in held) == 1 and any(h is tensors[2] for h in held)
    assert any(h is ei for h in held) and len(held) == 2  # the parent and the last epoch's graph
    hip_ops.graph_cache.drop(tensors[2])
    assert len(hip_ops.graph_cache.entries) == 1
    hip_ops.graph_cache.clear()


# ---- wiring into the layers ---------------------------------------------------------------
def _run_layer(pkg, conv, x, edge_index, cuda, edge_attr=None):
    """Forward and backward of ``conv`` in train mode from a fixed dropout seed."""
    pkg._lib.dropout_set_epoch(0, cuda)
    torch.manual_seed(77)
    conv.zero_grad()
    xx = x.clone().requires_grad_(True)
    out = conv(xx, edge_index) if edge_attr is None else conv(xx, edge_index, edge_attr)
    out.square().sum().backward()
    return [out.detach().clone(), xx.grad.clone()] + [p.grad.clone() for p in conv.parameters()]


def _layers(pkg, cuda):
    kw = dict(concat=False, add_self_loops=False)
    torch.manual_seed(3)
    return {"gat": pkg.GATConv(16, 32, heads=2, dropout=0.5, **kw).to(cuda).train(),
            "gatv2": pkg.GATv2Conv(16, 32, dropout=0.5, **kw).to(cuda).train()}


@pytest.mark.parametrize("kind", ["gat", "gatv2"])
def test_layers_on_the_derived_graph_equal_a_fresh_build(pkg, hip_ops, ladders, cuda, kind):
    ei_np, ei, _ = ladders[7]
    hip_ops.graph_cache.clear()
    conv = _layers(pkg, cuda)[kind]
    x = torch.randn(N_LADDER, 16, device=cuda)
    smp = pkg.NeighborSampler(ei, N_LADDER, 7, seed=1)
    ei_s, eid, gs = smp.epoch(0)
    builds = []
    ops_graph = importlib.import_module(pkg.__name__ + ".ops_graph")  # where graph_cache.get looks csr_build up
    orig = ops_graph.csr_build
    ops_graph.csr_build = lambda *a, **k: builds.append(1) or orig(*a, **k)
    try:
        got = _run_layer(pkg, conv, x, ei_s, cuda)
        assert not builds  # the registered graph was found
        fresh = ei_s.clone()
        want = _run_layer(pkg, conv, x, fresh, cuda)
        assert builds == [1] and hip_ops.graph_cache.get(fresh, N_LADDER) is not gs
    finally:
        ops_graph.csr_build = orig
        hip_ops.graph_cache.clear()
    assert len(got) == len(want) >= 5
    assert got[0].abs().max() > 0 and got[1].abs().max() > 0
    for a, b in zip(got, want):
        assert torch.isfinite(a).all() and torch.equal(a, b)


def test_edge_attributes_follow_eid(pkg, hip_ops, ladders, cuda):
    ei_np, ei, g = ladders[7]
    hip_ops.graph_cache.clear()
    torch.manual_seed(4)
    conv = pkg.GATConv(16, 32, heads=2, edge_dim=1, dropout=0.5, concat=False, add_self_loops=False).to(cuda).train()
    x = torch.randn(N_LADDER, 16, device=cuda)
    ea_np = np.random.default_rng(8).random((ei_np.shape[1], 1)).astype(np.float32)
    edge_attr = torch.from_numpy(ea_np).to(cuda)
    smp = pkg.NeighborSampler(ei, N_LADDER, 7, seed=2)
    ei_s, eid, gs = smp.epoch(1)
    got = _run_layer(pkg, conv, x, ei_s, cuda, edge_attr.index_select(0, eid))
    _, want_ei, want_eid = ref.sample(ei_np, N_LADDER, 7, ref.epoch_seed(2, 1))
    want = _run_layer(pkg, conv, x, torch.from_numpy(want_ei).to(cuda), cuda, torch.from_numpy(ea_np[want_eid]).to(cuda))
    hip_ops.graph_cache.clear()
    assert len(got) == len(want) >= 7
    assert got[0].abs().max() > 0 and got[1].abs().max() > 0
    for a, b in zip(got, want):
        assert torch.isfinite(a).all() and torch.equal(a, b)


# ---- trainer ---------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [[], ["--edge-features", "rating"],
                                   ["--model-family", "gatv2_pyg", "--fanout-items", "2", "--resample-every", "2"]],
                         ids=["gat", "edge", "gatv2_items"])
def test_trainer(pkg, cuda, tmp_path, capsys, monkeypatch, extra):
    train = importlib.import_module(pkg.__name__ + ".train")
    seen = []
    evaluate = train.evaluate
    monkeypatch.setattr(train, "evaluate", lambda args, model, cfg, feats, edge_index, *a, **k:
                        seen.append(int(edge_index.size(1))) or evaluate(args, model, cfg, feats, edge_index, *a, **k))
    capsys.readouterr()
    out = train.main(["--synthetic", "cfg1", "--fanout", "5", "--epochs", "2", "--eval-neg-k", "100", "--device-eval",
                      "--fast-sampler", "--structured-logs", "--models-prefix", str(tmp_path)] + extra)
    log = capsys.readouterr().out
    ev = [json.loads(ln) for ln in log.splitlines() if ln.startswith("{")]
    ends = [e for e in ev if e["event"] == "epoch_end"]
    n_users, n_items = (int(v) for v in re.search(r"n_users=(\d+), n_items=(\d+)", log).groups())
    assert len(ends) == 2 and all("sampled_edges" in e for e in ends)
    full = seen[0]
    assert len(seen) == 3 and seen == [full] * 3  # two validations and the test, all on the whole graph
    for e in ends:
        assert 0 < e["sampled_edges"] <= 5 * (n_users + n_items) and e["sampled_edges"] < full
    if "--resample-every" in extra:
        assert ends[0]["sampled_edges"] == ends[1]["sampled_edges"]
    vals = list(out["test"].values()) + list(out["val"].values()) + [e["loss"] for e in ends]
    assert vals and all(np.isfinite(v) for v in vals), out
