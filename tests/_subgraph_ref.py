"""Numpy reference of seed-subgraph sampling (include/ppgat.h "seed-subgraph sampling";
csrc/ppgat_subgraph.hip) and the graph its tests run on -- test infrastructure only.

The rule.  S = the edges ``_nsample_ref.sample`` keeps under (fanout, fanout_of, seed).
depth(v) = 0 at the seeds, else 1 + the least depth of a destination v feeds through an edge of S.
V = {depth <= L}, X = {depth < L}, K = {e in S : dst(e) in X}.  n_id = V ascending; a node's local id
is its position in n_id; the kept edges stay in ascending original edge id.
"""
from __future__ import annotations

import functools

import numpy as np

import _nsample_ref as nref

N_USERS, N_ITEMS = 3000, 1500
N = N_USERS + N_ITEMS
HUB_ITEM, HUB_DEGREE = 200, 70000
HUB = N_USERS + HUB_ITEM
# (F, L) and whether a source feeding destinations of two different depths must exist
CASES = [(1, 2, False), (2, 2, False), (2, 3, True), (7, 2, True), (32, 1, False), (64, 1, False), (64, 2, True)]
SEEDS = [42, (1 << 64) - 3]


def ladder(F: int):
    return [0, 1, 2, F - 1, F, F + 1, 2 * F - 1, 2 * F, 63, 64, 65, 127, 128, 129, 1000] * 10


@functools.lru_cache(maxsize=None)
def graph(F: int) -> np.ndarray:
    """edge_index [2, E] over 3,000 users (nodes 0 ..) and 1,500 items (nodes 3,000 ..): user rows
    0 .. 149 and item rows 0 .. 149 carry the in-degree ladder (sources from the other side: items
    < 1,400, users < 2,900, repeated pairs included), item 200 is a hub of 70,000 in-edges, 6,000
    random user-item pairs in both directions among users 150 .. 2,899 and items 150 .. 1,399, the
    last 100 users and items isolated; columns shuffled so that edge ids interleave across rows."""
    rng = np.random.default_rng(200 + F)
    deg = np.asarray(ladder(F), np.int64)
    rows = np.arange(len(deg))
    parts = [np.stack([N_USERS + rng.integers(0, 1400, deg.sum()), np.repeat(rows, deg)]),  # items -> user rows
             np.stack([rng.integers(0, 2900, deg.sum()), N_USERS + np.repeat(rows, deg)]),  # users -> item rows
             np.stack([rng.integers(0, 2900, HUB_DEGREE), np.full(HUB_DEGREE, HUB)])]
    u, i = rng.integers(150, 2900, 6000), N_USERS + rng.integers(150, 1400, 6000)
    parts += [np.stack([u, i]), np.stack([i, u])]
    ei = np.concatenate(parts, axis=1)
    ei = np.ascontiguousarray(ei[:, rng.permutation(ei.shape[1])])
    out_deg, in_deg = np.bincount(ei[0], minlength=N), np.bincount(ei[1], minlength=N)
    for lo, hi in ((2900, 3000), (N_USERS + 1400, N)):
        assert not out_deg[lo:hi].any() and not in_deg[lo:hi].any()
    assert np.array_equal(in_deg[:150], deg) and np.array_equal(in_deg[N_USERS:N_USERS + 150], deg)
    return ei


def seeds16() -> np.ndarray:
    """Sixteen seeds, fifteen unique, in no order: a degree-0 row, the rows of degree F, F + 1 and
    1000 on both sides, the hub, an isolated node, one duplicate, background nodes."""
    I = N_USERS
    return np.array([I + 14, 4, 2950, HUB, 0, I + 5, 500, 14, I + 600, 5, 4, I + 4, 2000, I + 1300, 1200, I + 900],
                    np.int64)


def subgraph(edge_index, n_nodes: int, seeds, hops: int, fanout: int, seed: int, fanout_of=None, n_users=None):
    """-> dict(n_id, depth, n_users_s, edge_index_s, eid, seed_local) plus ``keep`` [E] (the whole
    sampled graph's flags) and ``depth_all`` [n_nodes] (-1: no depth)."""
    ei = np.asarray(edge_index, np.int64)
    seeds = np.asarray(seeds, np.int64)
    assert ((seeds >= 0) & (seeds < n_nodes)).all()
    keep, _, _ = nref.sample(ei, n_nodes, fanout, seed, fanout_of)
    src, dst = ei[0], ei[1]
    depth = np.full(n_nodes, -1, np.int64)
    depth[seeds] = 0
    for h in range(hops):
        new = src[keep & (depth[dst] == h)]
        depth[new[depth[new] < 0]] = h + 1
    expanded = (depth >= 0) & (depth < hops)
    eid = np.flatnonzero(keep & expanded[dst])
    n_id = np.flatnonzero(depth >= 0)
    local = np.full(n_nodes, -1, np.int64)
    local[n_id] = np.arange(len(n_id))
    ei_s = local[ei[:, eid]]
    assert (ei_s >= 0).all()
    nu = n_nodes if n_users is None else int(n_users)
    return {"n_id": n_id, "depth": depth[n_id].astype(np.int32), "n_users_s": int((n_id < nu).sum()),
            "edge_index_s": ei_s, "eid": eid, "seed_local": local[seeds], "keep": keep, "depth_all": depth}


@functools.lru_cache(maxsize=None)
def case(F: int, L: int, seed: int):
    """The reference of one (F, L, seed) on ``graph(F)`` with ``seeds16()``: computed once, shared,
    never written to."""
    out = subgraph(graph(F), N, seeds16(), L, F, seed, n_users=N_USERS)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out
