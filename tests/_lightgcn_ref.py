"""fp64 oracle for the LightGCN tests (test infrastructure only): a dense A in float64 and
torch autograd, feasible at N ~ 1,200.  Restates scripts/train_lightgcn.py:64-76 and :326-331.
Also builds the toy graphs the GPU tests share."""
from __future__ import annotations

import numpy as np
import torch

from oracle import sampler_oracle as so


def dense_adj(indices: np.ndarray, values: np.ndarray, n: int) -> torch.Tensor:
    """Un-coalesced COO -> dense float64 (repeated entries add, as torch.sparse.mm does)."""
    A = torch.zeros(n, n, dtype=torch.float64)
    A.index_put_((torch.as_tensor(indices[0]), torch.as_tensor(indices[1])),
                 torch.as_tensor(np.asarray(values, np.float64)), accumulate=True)
    return A


def propagate(A: torch.Tensor, x0: torch.Tensor, K: int) -> torch.Tensor:
    out = acc = x0
    for _ in range(K):
        out = A @ out
        acc = acc + out
    return acc / (K + 1)


def bpr_loss(Z: torch.Tensor, n_users: int, u, i, j) -> torch.Tensor:
    U, I = Z[:n_users], Z[n_users:]
    pos = (U[u] * I[i]).sum(-1)
    neg = (U[u] * I[j]).sum(-1)
    return -torch.log(torch.sigmoid(pos - neg) + 1e-8).mean()


def toy_train_pos(rng, n_users=901, n_items=300, iso_users=20, iso_items=10):
    """The issue's toy graph T -> train_pos_idx (dict in user order).  Item 0 held by 700 users
    (three hub pieces), item 1 by exactly 256, item 2 by exactly 257 (the piece boundary), user 1
    with exactly 16 and user 2 with exactly 17 interactions (the short / long boundary), every
    10th user 17-59, the rest 1-8, every 50th user repeats an interaction; the last ``iso_users``
    users and ``iso_items`` items have none."""
    live_u, live_i = n_users - iso_users, n_items - iso_items
    pool = np.arange(3, live_i)  # items 0, 1, 2 are placed by hand
    tr = {}
    for u in range(live_u):
        if u == 1:
            d = 16
        elif u == 2:
            d = 17
        elif u % 10 == 0:
            d = int(rng.integers(17, 60))
        else:
            d = int(rng.integers(1, 9))
        tr[u] = list(rng.choice(pool, size=d, replace=False))
    # hand-placed holders replace a user's LAST pool item, keeping the degrees above
    def hold(item, users):
        for u in users:
            tr[u][-1] = item
    order = rng.permutation(np.setdiff1d(np.arange(live_u), [1, 2]))
    hold(0, order[:700])
    for u in order[:256]:
        tr[u].append(1)                       # 256 holders of item 1 (degree + 1, off the boundaries)
    for u in order[300:557]:
        tr[u].append(2)                       # 257 holders of item 2
    for u in range(0, live_u, 50):
        if u not in (1, 2):
            tr[u].append(tr[u][0])            # a repeated interaction
    # keep users 1 and 2 at exactly 16 / 17
    assert len(tr[1]) == 16 and len(tr[2]) == 17
    return {u: np.asarray(v, dtype=np.int64) for u, v in tr.items()}


def directed_adj(rng, n, n_iso=30):
    """A directed, randomly weighted matrix with no symmetry on n nodes, degrees as in T: row
    (destination) hubs and column (source) hubs are different nodes.  -> (indices [2, nnz], values)."""
    live = n - n_iso
    rows, cols = [], []
    for r in range(live):
        if r == 0:
            d = 700
        elif r == 1:
            d = 16
        elif r == 2:
            d = 17
        elif r == 3:
            d = 256
        elif r == 4:
            d = 257
        elif r % 10 == 0:
            d = int(rng.integers(17, 60))
        else:
            d = int(rng.integers(1, 9))
        c = rng.choice(live, size=d, replace=False)
        rows.append(np.full(d, r)); cols.append(c)
    # column hubs: nodes live-1 (600 rows) and live-2 (exactly 257 rows) as sources
    for c, d in ((live - 1, 600), (live - 2, 257)):
        r = rng.choice(live - 10, size=d, replace=False)
        rows.append(r); cols.append(np.full(d, c))
    rows = np.concatenate(rows).astype(np.int64)
    cols = np.concatenate(cols).astype(np.int64)
    perm = rng.permutation(len(rows))
    rows, cols = rows[perm], cols[perm]
    vals = rng.uniform(0.01, 1.0, len(rows)).astype(np.float32)
    return np.vstack([rows, cols]), vals


def sample_positives_numpy(user_ptr, user_items, n_items, neg_per_pos, batch_size, batch, seed):
    """ppgat_bpr_sample_positives restated: triple t -> position p = t // neg_per_pos of user_items
    in the order given, its owner u, i = user_items[p], j = the first draw d of (seed, t, d) that
    is not one of u's items.  -> (u, i, j, bad)."""
    user_ptr = np.asarray(user_ptr, np.int64)
    user_items = np.asarray(user_items, np.int64)
    total = len(user_items) * neg_per_pos
    t0 = batch * batch_size
    S = min(batch_size, total - t0)
    t = np.arange(t0, t0 + S, dtype=np.int64)
    p = t // neg_per_pos
    u = np.searchsorted(user_ptr, p, side="right") - 1
    i = user_items[p]
    items_sorted, _ = so.prepare(user_ptr, user_items)
    owner = np.repeat(np.arange(len(user_ptr) - 1, dtype=np.int64), np.diff(user_ptr))
    keys = owner * np.int64(n_items) + items_sorted
    j = np.full(S, -1, np.int64)
    open_ = np.arange(S)
    for d in range(so.MAX_NEG_DRAWS):
        if open_.size == 0:
            break
        c = so.below(so.draw64(seed, t[open_].astype(np.uint64), d), n_items)
        q = u[open_] * np.int64(n_items) + c
        ix = np.minimum(np.searchsorted(keys, q), len(keys) - 1)
        hit = keys[ix] == q
        j[open_[~hit]] = c[~hit]
        open_ = open_[hit]
    bad = 0
    if open_.size:
        j[open_] = 0
        bad = 2
    return u, i, j, bad
