"""Numpy reference of the fan-out neighbour sampling rule (include/ppgat.h "fan-out neighbour
sampling"; csrc/ppgat_nsample.hip), on the oracle's counter stream -- test infrastructure only.

Destination i with in-degree d and cap f numbers its in-edges p = 0 .. d - 1 in CSR slot order
(a stable sort by destination: ascending original edge id).  d <= f keeps all; d > f keeps Robert
Floyd's subset:  S = {};  for s < f:  j = d - f + s;  t = below(draw64(seed, i, s), j + 1);
add (j if t in S else t).
"""
from __future__ import annotations

import numpy as np

from oracle.sampler_oracle import below, draw64

MAX_FANOUT = 64
EPOCH_DRAW = 1023


def floyd(seed: int, i: int, d: int, f: int) -> list:
    """The kept positions of one row with d > f, in the order the algorithm adds them."""
    S = []
    for s in range(f):
        j = d - f + s
        t = int(below(draw64(seed, np.uint64(i), s), j + 1))
        S.append(j if t in S else t)
    return S


def floyd_rows(seed: int, rows: np.ndarray, d: np.ndarray, f: np.ndarray) -> np.ndarray:
    """``floyd`` for many rows at once (each with d > f >= 1): [n, max f] positions in the order
    added, -1 past a row's f."""
    rows, d, f = np.asarray(rows, np.uint64), np.asarray(d, np.int64), np.asarray(f, np.int64)
    S = np.full((len(rows), int(f.max()) if len(rows) else 0), -1, np.int64)
    for s in range(S.shape[1]):
        a = np.flatnonzero(f > s)
        j = d[a] - f[a] + s
        t = below(draw64(seed, rows[a], s), j + 1)
        hit = (S[a, :s] == t[:, None]).any(axis=1)
        S[a, s] = np.where(hit, j, t)
    return S


def caps(deg: np.ndarray, fanout: int, fanout_of=None) -> np.ndarray:
    """The cap of every destination (``deg`` where it keeps all)."""
    f = np.full(len(deg), int(fanout), np.int64)
    if fanout_of is not None:
        fo = np.asarray(fanout_of, np.int64)
        assert (fo <= MAX_FANOUT).all()
        f = np.where(fo >= 0, fo, deg)
    return f


def sample(edge_index: np.ndarray, n_nodes: int, fanout: int, seed: int, fanout_of=None):
    """-> (keep [E] bool by original edge id, edge_index_s [2, E'], eid [E'])."""
    ei = np.asarray(edge_index, np.int64)
    E = ei.shape[1]
    order = np.argsort(ei[1], kind="stable")  # CSR slot -> edge id
    deg = np.bincount(ei[1], minlength=n_nodes).astype(np.int64)
    rowptr = np.concatenate([[0], np.cumsum(deg)])
    f = caps(deg, fanout, fanout_of)
    keep = np.zeros(E, bool)
    whole = np.repeat(deg <= f, deg)  # per slot: its row keeps everything
    keep[order[whole]] = True
    big = np.flatnonzero((deg > f) & (f > 0))
    if len(big):
        S = floyd_rows(seed, big, deg[big], f[big])
        r, c = np.nonzero(S >= 0)
        keep[order[rowptr[big[r]] + S[r, c]]] = True
    eid = np.flatnonzero(keep)
    return keep, ei[:, eid], eid


def epoch_seed(seed: int, epoch: int) -> int:
    """The seed of epoch ``epoch``: draw64(seed, epoch, 1023) on the oracle's stream."""
    return int(draw64(seed & 0xFFFFFFFFFFFFFFFF, np.uint64(epoch), EPOCH_DRAW))
