"""numpy references of the older selection kernels (ppgat_knn_topk, ppgat_serve_topk,
ppgat_sampled_rank), shared by the host and GPU tests, with the exact-arithmetic cases they run on.

Everything here is exact: the selection reference orders fp32 values it is handed (no arithmetic),
the serving and ranking references score integer-valued vectors in fp64, where every product and
sum is an integer multiple of a power of two far below 2^24 and so is the fp32 result whatever the
summation order.  The total order is (value descending, index ascending) by ``np.lexsort``.
"""
from __future__ import annotations

import numpy as np

SPECIAL_ROWS = ("equal", "ascending", "descending", "one_lane", "last_group")


def knn_topk_ref(S, n_cols, q0, k, min_sim):
    """ppgat_knn_topk on the host: S [rows, ld] fp32 -> (idx int32 [rows, k], sim fp32 [rows, k],
    cnt int32 [rows]).  Per row the self column q0 + r, every -inf and every NaN are removed; the
    rest is ordered (value descending, index ascending); the first k are written, padded with
    -1 / -inf; cnt = how many of the written values are >= min_sim."""
    S = np.asarray(S, np.float32)
    rows = S.shape[0]
    idx = np.full((rows, k), -1, np.int32)
    sim = np.full((rows, k), -np.inf, np.float32)
    cnt = np.zeros(rows, np.int32)
    cols = np.arange(n_cols)
    for r in range(rows):
        v = S[r, :n_cols]
        ok = ~np.isnan(v) & (v != -np.inf) & (cols != q0 + r)
        c = cols[ok]
        order = c[np.lexsort((c, -v[c].astype(np.float64)))][:k]
        idx[r, :len(order)] = order
        sim[r, :len(order)] = v[order]
        cnt[r] = int((v[order] >= np.float32(min_sim)).sum())
    return idx, sim, cnt


def knn_case(rows, n_cols, k, q0, ld, seed, n_special=5):
    """S [rows, ld] fp32 for the selection test.  Ordinary rows hold multiples of 1/16 in [-1, 1]
    (33 values: exact ties everywhere).  The first min(rows, n_special) rows are, in the order of
    SPECIAL_ROWS rotated by ``seed``: all equal; strictly ascending (every element displaces a
    lane's k-th value); strictly descending; the best values only in columns = c mod 64 (one lane's
    stride), in tied pairs; the best values only in the last partial group of 256 columns.  The
    self column, where it exists, holds the row's largest value (2.0): leaving it in would show.
    Columns n_cols .. ld - 1 hold +inf and must never be read."""
    rng = np.random.default_rng(seed)
    S = np.full((rows, ld), np.inf, np.float32)
    S[:, :n_cols] = rng.integers(-16, 17, (rows, n_cols)).astype(np.float32) / 16
    j = np.arange(n_cols)
    for r in range(min(rows, n_special)):
        kind = SPECIAL_ROWS[(r + seed) % len(SPECIAL_ROWS)]
        if kind == "equal":
            S[r, :n_cols] = 0.25
        elif kind == "ascending":
            S[r, :n_cols] = (j - n_cols // 2) / 1024.0
        elif kind == "descending":
            S[r, :n_cols] = (n_cols // 2 - j) / 1024.0
        elif kind == "one_lane":
            c = int(rng.integers(0, 64))
            S[r, :n_cols] = -np.abs(S[r, :n_cols])
            lane = j[j % 64 == c]
            S[r, lane] = 1.0 - (np.arange(len(lane)) // 2) / 64.0   # tied pairs, best first
        elif kind == "last_group":
            g0 = (n_cols - 1) // 256 * 256
            S[r, :n_cols] = -np.abs(S[r, :n_cols])
            S[r, g0:n_cols] = 0.5 + rng.integers(0, 5, n_cols - g0) / 16.0
    for r in range(rows):
        if 0 <= q0 + r < n_cols:
            S[r, q0 + r] = 2.0
    return S


def serve_scores64(V, histories):
    """[B, n_items] fp64: <item, mean of the history rows>, the history set to -1e9 by index."""
    V64 = np.asarray(V, np.float64)
    S = np.empty((len(histories), len(V64)), np.float64)
    for b, h in enumerate(histories):
        h = np.asarray(h, np.int64)
        S[b] = V64 @ V64[h].mean(0)   # a repeated item counts twice in the mean
        S[b, h] = -1e9                # and is masked once
    return S


def serve_topk_ref(V, histories, k):
    """(idx int64 [B, k], score fp64 [B, k]): serving/runtime.py:56-76 under the total order
    (score descending, item index ascending); masked items keep their place at -1e9."""
    S = serve_scores64(V, histories)
    ar = np.arange(S.shape[1])
    idx = np.stack([np.lexsort((ar, -s))[:k] for s in S]).astype(np.int64)
    return idx, np.take_along_axis(S, idx, 1)


def serve_case(C, B, n_items, seed, max_len=32):
    """Integer item vectors in [-3, 3] and B histories whose lengths are powers of two <= 32 (and
    <= n_items): the fp32 mean and every fp32 score are exact."""
    rng = np.random.default_rng(seed)
    V = rng.integers(-3, 4, (n_items, C)).astype(np.float32)
    lens = [l for l in (1, 2, 4, 8, 16, 32) if l <= min(max_len, n_items)]
    hists = [rng.choice(n_items, int(rng.choice(lens)), replace=False).tolist() for _ in range(B)]
    return V, hists


def sampled_rank_ref(Z, n_users, users, cands):
    """rank int64 [B] = #(s > s0) + 1 over candidates 1 .. K1 - 1, s = <Z[n_users + cand], Z[user]>
    in fp64, s0 the score of candidate 0 (strict: a tie, or the positive again, does not count)."""
    Z64 = np.asarray(Z, np.float64)
    users, cands = np.asarray(users, np.int64), np.asarray(cands, np.int64)
    s = np.einsum("bkc,bc->bk", Z64[n_users + cands], Z64[users])
    return (s[:, 1:] > s[:, :1]).sum(1).astype(np.int64) + 1


def rank_case(C, B, K1, seed, n_users=40, n_items=60):
    """Integer Z in [-3, 3]; items 0..9 repeat the rows of items 10..19 (ties under another index);
    where K1 > 3, candidate 3 is the positive again."""
    rng = np.random.default_rng(seed)
    Z = rng.integers(-3, 4, (n_users + n_items, C)).astype(np.float32)
    Z[n_users:n_users + 10] = Z[n_users + 10:n_users + 20]
    users = rng.integers(0, n_users, B).astype(np.int64)
    cands = rng.integers(0, n_items, (B, K1)).astype(np.int64)
    if K1 > 3:
        cands[:, 3] = cands[:, 0]
    if K1 > 2:
        cands[::2, 0] = rng.integers(0, 10, len(cands[::2]))       # a positive with a twin row,
        cands[::2, 2] = cands[::2, 0] + 10                          # and the twin among the candidates
        if K1 > 3:
            cands[:, 3] = cands[:, 0]
    return Z, users, cands
