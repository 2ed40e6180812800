"""numpy reference of the full-catalogue ranking (ppgat_full_rank), shared by the host and GPU tests.

fp64 scores; exclusion by INDEX (the user's history and the positive itself), never by score;
the strict count and the tie count; and a band helper: the lowest and highest rank an
implementation may report when each score comparison carries a per-pair tolerance tau.
"""
from __future__ import annotations

import numpy as np


def excluded_mask(users, pos, n_items, ptr=None, items=None):
    """[n_eval, n_items] bool: True where item i is in history(users[b]) or is pos[b]."""
    users, pos = np.asarray(users, np.int64), np.asarray(pos, np.int64)
    ex = np.zeros((len(users), n_items), bool)
    ex[np.arange(len(users)), pos] = True
    if ptr is not None:
        for b, u in enumerate(users):
            ex[b, np.asarray(items[ptr[u]:ptr[u + 1]], np.int64)] = True
    return ex


def scores64(U, I, users):
    return np.asarray(U, np.float64)[np.asarray(users, np.int64)] @ np.asarray(I, np.float64).T


def full_rank_ref(U, I, users, pos, ptr=None, items=None):
    """(rank, ties) int64: rank = 1 + #{i not excluded: s(i) > s(p)}, ties = #{...: s(i) == s(p)}."""
    S = scores64(U, I, users)
    sp = S[np.arange(len(S)), np.asarray(pos, np.int64)][:, None]
    inc = ~excluded_mask(users, pos, I.shape[0], ptr, items)
    return 1 + ((S > sp) & inc).sum(1), ((S == sp) & inc).sum(1)


def rank_band(U, I, users, pos, ptr=None, items=None, scale=0.0):
    """(lo, hi, rank64): the ranks allowed when s(i) - s(p) is known only to within
    tau(b, i) = scale * (|u|^T |i| + |u|^T |i_pos|): lo counts the items surely above the
    positive, hi those possibly above it."""
    users, pos = np.asarray(users, np.int64), np.asarray(pos, np.int64)
    S = scores64(U, I, users)
    A = scores64(np.abs(U), np.abs(I), users)
    rows = np.arange(len(S))
    d = S - S[rows, pos][:, None]
    tau = scale * (A + A[rows, pos][:, None])
    inc = ~excluded_mask(users, pos, I.shape[0], ptr, items)
    lo = 1 + ((d > tau) & inc).sum(1)
    hi = 1 + ((d >= -tau) & inc).sum(1)
    return lo, hi, 1 + ((d > 0) & inc).sum(1)


def csr_from_lists(hist, n_users):
    """(ptr int64 [n_users + 1], items int64) from {user: iterable of items}, each list in its own order."""
    lens = np.array([len(hist.get(u, ())) for u in range(n_users)], np.int64)
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    flat = [np.asarray(hist[u], np.int64) for u in range(n_users) if lens[u]]
    return ptr, (np.concatenate(flat) if flat else np.zeros(0, np.int64))


def integer_case(C, n_users=90, n_items=700, n_eval=130, seed=0, max_hist=40):
    """Integer-valued fp32 embeddings in {-3..3} (every product and sum exact in fp32 and in the
    bf16 split), repeated users, histories of length 0..max_hist; user 0's history covers items
    0..255 entirely, users 1-3 hold item 0, the last item and (for the entries of users 1-3)
    their positive.  Returns a dict of arrays; ptr/items hold each history SORTED."""
    rng = np.random.default_rng(seed)
    U = rng.integers(-3, 4, (n_users, C)).astype(np.float32)
    I = rng.integers(-3, 4, (n_items, C)).astype(np.float32)
    users = rng.integers(0, n_users, n_eval).astype(np.int64)
    fixed = np.array([0, 1, 2, 3, 4, 0, 1, 2, 3])[:n_eval]
    users[:len(fixed)] = fixed
    pos = rng.integers(0, n_items, n_eval).astype(np.int64)
    hist = {}
    for u in range(n_users):
        k = int(rng.integers(0, min(max_hist, n_items) + 1))
        hist[u] = rng.choice(n_items, k, replace=False) if k else np.zeros(0, np.int64)
    hist[0] = np.arange(min(256, n_items))
    hist[4] = np.zeros(0, np.int64)  # an empty history for sure
    for u in (1, 2, 3):
        hist[u] = np.unique(np.concatenate([hist[u], [0, n_items - 1], pos[users == u]]))
    hist = {u: np.sort(np.asarray(v, np.int64)) for u, v in hist.items()}
    ptr, items = csr_from_lists(hist, n_users)
    return {"U": U, "I": I, "users": users, "pos": pos, "ptr": ptr, "items": items, "hist": hist}
