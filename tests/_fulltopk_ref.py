"""numpy reference of the full-catalogue top-K (ppgat_full_topk), shared by the host and GPU tests.

fp64 scores (``_fullrank_ref.scores64``); the user's history set to -inf by INDEX; the total order
(score descending, item index ascending) by ``np.lexsort``; the first k, padded with -1 / -inf
where fewer than k items are eligible.
"""
from __future__ import annotations

import numpy as np

import _fullrank_ref as rr


def history_mask(users, n_items, ptr=None, items=None):
    """[n_query, n_items] bool: True where item i is in history(users[b])."""
    users = np.asarray(users, np.int64)
    ex = np.zeros((len(users), n_items), bool)
    if ptr is not None:
        for b, u in enumerate(users):
            ex[b, np.asarray(items[ptr[u]:ptr[u + 1]], np.int64)] = True
    return ex


def full_topk_ref(U, I, users, k, ptr=None, items=None):
    """(idx int32 [n, k], score fp64 [n, k]): the k best items outside each history, best first."""
    users = np.arange(len(U)) if users is None else np.asarray(users, np.int64)
    n_items = len(I)
    S = rr.scores64(U, I, users).reshape(len(users), n_items)
    ex = history_mask(users, n_items, ptr, items)
    idx = np.full((len(users), k), -1, np.int32)
    sc = np.full((len(users), k), -np.inf, np.float64)
    ar = np.arange(n_items)
    for b in range(len(users)):
        s = np.where(ex[b], -np.inf, S[b])
        order = np.lexsort((ar, -s))
        order = order[~ex[b][order]][:k]
        idx[b, :len(order)] = order
        sc[b, :len(order)] = S[b, order]
    return idx, sc


def gaussian_case(C, n_users=300, n_items=1500, n_query=384):
    """The Gaussian case of the rank test's shape, drawn in a fixed order from default_rng(C)."""
    rng = np.random.default_rng(C)
    U = rng.standard_normal((n_users, C)).astype(np.float32)
    I = rng.standard_normal((n_items, C)).astype(np.float32)
    users = rng.integers(0, n_users, n_query).astype(np.int64)
    hist = {u: np.sort(rng.choice(n_items, int(rng.integers(0, 60)), replace=False)) for u in range(n_users)}
    ptr, items = rr.csr_from_lists(hist, n_users)
    return {"U": U, "I": I, "users": users, "ptr": ptr, "items": items, "hist": hist}
