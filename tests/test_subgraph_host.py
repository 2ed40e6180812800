"""Seed-subgraph sampling, the parts that need no GPU: the numpy reference against an independent
BFS over the sampler's keep mask, what the test cases cover (asserted from the reference alone), the
edge cases of the rule, the ABI's refusals (nothing launched), the trainer's refusals -- CPU."""
import collections
import ctypes
import importlib

import numpy as np
import pytest

import _nsample_ref as nref
import _subgraph_ref as ref


def _bfs(ei, n_nodes, seeds, hops, keep):
    """The rule written again: per-destination lists of kept in-edges, a queue, Python sets."""
    into = collections.defaultdict(list)
    for e in np.flatnonzero(keep).tolist():
        into[int(ei[1, e])].append(e)
    depth = {int(s): 0 for s in seeds}
    queue = collections.deque(sorted(depth))
    kept = set()
    while queue:
        v = queue.popleft()
        if depth[v] >= hops:
            continue
        for e in into[v]:
            kept.add(e)
            s = int(ei[0, e])
            if s not in depth:
                depth[s] = depth[v] + 1
                queue.append(s)
    return depth, sorted(kept)


@pytest.mark.parametrize("seed", ref.SEEDS, ids=["seed42", "seed2^64-3"])
@pytest.mark.parametrize("F,L,two_depth", ref.CASES)
def test_reference_agrees_with_an_independent_bfs(F, L, two_depth, seed):
    ei = ref.graph(F)
    got = ref.case(F, L, seed)
    keep, want_ei, want_eid = nref.sample(ei, ref.N, F, seed)
    assert np.array_equal(got["keep"], keep)
    depth, kept = _bfs(ei, ref.N, ref.seeds16(), L, keep)
    nodes = sorted(depth)
    assert got["n_id"].tolist() == nodes and got["depth"].tolist() == [depth[v] for v in nodes]
    assert got["eid"].tolist() == kept
    assert np.array_equal(got["n_id"][got["edge_index_s"]], ei[:, got["eid"]])  # local ids name the same nodes
    assert np.array_equal(got["n_id"][got["seed_local"]], ref.seeds16())
    assert got["n_users_s"] == sum(v < ref.N_USERS for v in nodes)
    assert (np.diff(got["n_id"]) > 0).all() and (np.diff(got["eid"]) > 0).all()
    print(f"(F={F}, L={L}, seed={seed}): N_s={len(nodes)} E_s={len(kept)} E={ei.shape[1]}")


@pytest.mark.parametrize("seed", ref.SEEDS, ids=["seed42", "seed2^64-3"])
@pytest.mark.parametrize("F,L,two_depth", ref.CASES)
def test_cases_cover_what_they_claim(F, L, two_depth, seed):
    ei = ref.graph(F)
    got = ref.case(F, L, seed)
    assert 113000 <= ei.shape[1] <= 124000 and len(set(ref.seeds16().tolist())) == 15 and len(ref.seeds16()) == 16
    if (F, L) != (64, 2):
        assert len(got["n_id"]) < ref.N / 2
    deg = np.bincount(ei[1], minlength=ref.N)
    X = np.flatnonzero((got["depth_all"] >= 0) & (got["depth_all"] < L))
    dx = deg[X]
    assert (dx < F).any() and (dx == F).any() and (dx == F + 1).any() and (dx >= 1000).any() and ref.HUB in X
    # a source that feeds destinations of two different depths through kept edges
    src, dst = ei[0, got["eid"]], ei[1, got["eid"]]
    dd = got["depth_all"][dst]
    lo, hi = np.full(ref.N, 99), np.full(ref.N, -1)
    np.minimum.at(lo, src, dd)
    np.maximum.at(hi, src, dd)
    if two_depth:
        assert (hi > lo).any()
    # the isolated seed is a node without edges; the last 100 users and items hold no other node
    iso = got["n_id"][(got["n_id"] >= 2900) & (got["n_id"] < ref.N_USERS) | (got["n_id"] >= ref.N_USERS + 1400)]
    assert iso.tolist() == [2950]


def test_zero_hops_empty_and_isolated_seeds():
    ei = ref.graph(7)
    z = ref.subgraph(ei, ref.N, ref.seeds16(), 0, 7, 42, n_users=ref.N_USERS)
    assert z["n_id"].tolist() == sorted(set(ref.seeds16().tolist())) and z["eid"].size == 0
    assert z["edge_index_s"].shape == (2, 0) and not z["depth"].any()
    e = ref.subgraph(ei, ref.N, np.zeros(0, np.int64), 3, 7, 42, n_users=ref.N_USERS)
    assert e["n_id"].size == 0 and e["eid"].size == 0 and e["seed_local"].size == 0 and e["n_users_s"] == 0
    iso = np.array([2999, 2900, ref.N - 1, 2999], np.int64)
    s = ref.subgraph(ei, ref.N, iso, 2, 7, 42, n_users=ref.N_USERS)
    assert s["n_id"].tolist() == [2900, 2999, ref.N - 1] and s["eid"].size == 0 and s["n_users_s"] == 2
    assert s["seed_local"].tolist() == [1, 0, 2, 1]


# ---- library and trainer ---------------------------------------------------------------
def test_abi_refusals_launch_nothing(pkg):
    lib = pkg._lib.load()
    assert lib.ppgat_subgraph_max_hops() == 8
    p = ctypes.c_void_p(256)  # never dereferenced: every call below is refused on the host
    big = 1 << 20
    # seed
    ok = [p, 16, 100, p, p, big, None]
    assert lib.ppgat_subgraph_seed(*[None if k == 0 else v for k, v in enumerate(ok)]) == 1
    for pos, val, rc in ((1, -1, 1), (2, -1, 1), (3, None, 1), (4, None, 1), (5, 0, 1), (2, 1 << 31, 2), (1, 1 << 31, 2)):
        a = list(ok)
        a[pos] = val
        assert lib.ppgat_subgraph_seed(*a) == rc, (pos, val)
    # expand: fanout, hop, sizes, pointers, workspace
    ok = [p, p, 100, 500, 0, 5, None, 42, p, big, None]
    for fanout in (0, -1, 65):
        a = list(ok)
        a[5] = fanout
        assert lib.ppgat_subgraph_expand(*a) == 2 and b"fanout" in lib.ppgat_last_error()
    for pos, val, rc in ((4, -1, 1), (4, 8, 1), (2, -1, 1), (3, -1, 1), (0, None, 1), (1, None, 1), (8, None, 1),
                         (9, 0, 1), (2, 1 << 31, 2)):
        a = list(ok)
        a[pos] = val
        assert lib.ppgat_subgraph_expand(*a) == rc, (pos, val)
    # plan
    ok = [100, 60, 2, 5, None, p, p, p, big, None]
    for fanout in (0, 65):
        a = list(ok)
        a[3] = fanout
        assert lib.ppgat_subgraph_plan(*a) == 2
    for pos, val in ((0, -1), (1, -1), (1, 101), (2, -1), (2, 9), (5, None), (6, None), (7, None), (8, 0)):
        a = list(ok)
        a[pos] = val
        assert lib.ppgat_subgraph_plan(*a) == 1, (pos, val)
    assert b"workspace" in lib.ppgat_last_error()
    # relabel
    ok = [100, 40, 70, p, 16, p, p, p, p, p, p, p, p, p, p, p, big, None]
    for pos, val in ((0, -1), (1, -1), (1, 101), (2, -1), (4, -1), (16, 0)):
        a = list(ok)
        a[pos] = val
        assert lib.ppgat_subgraph_relabel(*a) == 1, (pos, val)
    for pos in (3, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15):
        a = list(ok)
        a[pos] = None
        assert lib.ppgat_subgraph_relabel(*a) == 1, pos
    with pytest.raises(NotImplementedError):
        a = [p, p, 100, 500, 0, 65, None, 42, p, big, None]
        pkg._lib.check(lib.ppgat_subgraph_expand(*a), "subgraph_expand")


def test_workspace_query_is_host_only(pkg):
    lib = pkg._lib.load()
    n = ctypes.c_size_t(0)
    assert lib.ppgat_subgraph_workspace_bytes(1000, ctypes.byref(n)) == 0
    assert n.value >= 2 * 1001 * 4  # the depths and the relabel map
    small = n.value
    assert lib.ppgat_subgraph_workspace_bytes(100000, ctypes.byref(n)) == 0 and n.value > small
    assert lib.ppgat_subgraph_workspace_bytes(0, ctypes.byref(n)) == 0
    assert lib.ppgat_subgraph_workspace_bytes(-1, ctypes.byref(n)) == 1
    assert lib.ppgat_subgraph_workspace_bytes(10, None) == 1
    assert lib.ppgat_version() == 3


def test_python_layer_refuses_cpu_tensors(pkg):
    import torch
    ei = torch.tensor([[0, 1], [1, 2]])
    with pytest.raises(RuntimeError, match="ROCm"):
        pkg.sample_subgraph(ei, 3, torch.tensor([0]), 2, 5, 42)
    with pytest.raises(RuntimeError, match="ROCm"):
        pkg.SubgraphSampler(ei, 3, 2, 5)
    assert pkg.neighbors.MAX_HOPS == 8
    for cls in (pkg.PyGGAT, pkg.PyGGATv2, pkg.CustomGAT):
        assert callable(cls.forward_subgraph)
    assert callable(pkg.forward_subgraph) and callable(pkg.Subgraph.localize)


def test_trainer_refusals_and_defaults(pkg):
    train = importlib.import_module(pkg.__name__ + ".train")
    base = ["--synthetic", "cfg1", "--fanout", "5", "--subgraph-batch", "4096"]
    with pytest.raises(NotImplementedError, match="subgraph-batch"):
        train.main(base + ["--model-family", "lightgcn"])
    with pytest.raises(NotImplementedError, match="subgraph-batch"):
        train.main(base + ["--world-size", "2"])
    with pytest.raises(NotImplementedError, match="subgraph-batch"):
        train.main(base + ["--loss", "softmax", "--shared-negatives", "64"])
    with pytest.raises(ValueError, match="fanout"):
        train.main(["--synthetic", "cfg1", "--subgraph-batch", "4096"])
    with pytest.raises(ValueError, match="resample-every"):
        train.main(base + ["--resample-every", "2"])
    with pytest.raises(ValueError):
        train.main(["--synthetic", "cfg1", "--fanout", "5", "--subgraph-batch", "-1"])
    args = train.build_parser().parse_args([])
    assert args.subgraph_batch == 0 and args.fanout == 0 and args.resample_every == 1
