"""BPR triple sampler on the GPU -- scripts/train_gat_pyg.py:179-190 (sample_bpr_epoch).

``BPRSampler(user_ptr, user_items, n_items, device)`` sorts each user's train items once
(``ppgat_bpr_sampler_prepare``); ``sample(S, seed, offset=0)`` returns device int64 tensors
(u, i, j) drawn by ``ppgat_bpr_sample`` with the reference's rule -- u uniform over users
with train items, i uniform over u's train list, j uniform over the items u has not
interacted with (rejection, as :185-188) -- from a counter-based stream: triple t depends
only on (seed, offset + t), so an epoch can be drawn in pieces.  The stream is not Python's
``random``; parity runs that need the reference's exact triples keep
``data.sample_bpr_epoch``.  No CPU path: the library must be loaded and tensors live on
a ROCm device.

``BPRSampler(..., item_weights=w)`` draws the negatives of ``sample``, ``sample_candidates`` and
``sample_pool`` in proportion to ``w`` instead of uniformly (``popularity_weights``: train count
^ 0.75).  The weights are quantised on the host to integers (``quantise_item_weights``), so the
distribution the device draws from, q_i = w_i / total, is known exactly; ``correction`` and
``pool_correction`` are the logQ terms the softmax losses subtract from the sampled logits.
``eval_candidates`` and ``sample_positives`` stay uniform: evaluation is a protocol.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _launch


def quantise_item_weights(item_weights, n_items: int):
    """Non-negative weights [n_items] -> (w uint64 [n_items], cdf uint64 [n_items], total int, log_q fp32):
    w_i = floor(weights_i / max(weights) * 2^32) in float64, a positive weight that floors to 0
    becomes 1 and a zero weight stays 0 (never drawn); cdf is the inclusive prefix sum, total =
    cdf[-1]; log_q = log(w_i / total) from float64, -inf where w_i = 0.  ValueError on a wrong
    length, a negative or non-finite weight, or no positive weight.  Host only (numpy)."""
    if isinstance(item_weights, torch.Tensor):
        item_weights = item_weights.detach().cpu().numpy()
    x = np.asarray(item_weights, dtype=np.float64).reshape(-1)
    if x.size != int(n_items):
        raise ValueError(f"item_weights: {x.size} weights for n_items = {int(n_items)}")
    if not np.isfinite(x).all():
        raise ValueError("item_weights: weights must be finite")
    if (x < 0).any():
        raise ValueError("item_weights: weights must be non-negative")
    if not (x > 0).any():
        raise ValueError("item_weights: at least one weight must be positive")
    w = np.floor(x / x.max() * 2.0 ** 32).astype(np.uint64)
    w[(x > 0) & (w == 0)] = 1
    cdf = np.cumsum(w, dtype=np.uint64)
    total = int(cdf[-1])
    with np.errstate(divide="ignore"):
        log_q = np.log(w.astype(np.float64)) - np.log(float(total))
    return w, cdf, total, log_q.astype(np.float32)


def _q64(w: np.ndarray, total: int) -> np.ndarray:
    return w.astype(np.float64) / float(total)


def logq_correction(w: np.ndarray, total: int, n_neg: int) -> np.ndarray:
    """log(M q_i), the log of the expected count of item i among M draws with replacement: fp32
    from float64, -inf where w_i = 0.  Host only."""
    with np.errstate(divide="ignore"):
        return np.log(float(n_neg) * _q64(w, total)).astype(np.float32)


def logq_pool_correction(w: np.ndarray, total: int, tries: int) -> np.ndarray:
    """log(1 - (1 - q_i)^T), the log of the probability that item i is among T draws with
    replacement, as log(-expm1(T log1p(-q_i))): fp32 from float64, -inf where w_i = 0.  Host only."""
    with np.errstate(divide="ignore"):
        return np.log(-np.expm1(float(tries) * np.log1p(-_q64(w, total)))).astype(np.float32)


class BPRSampler:
    def __init__(self, user_ptr, user_items, n_items: int, device=None, item_weights=None):
        self.weighted = item_weights is not None
        if self.weighted:  # host work first: a bad weight vector raises before anything touches a device
            self.w, cdf, self.total, log_q = quantise_item_weights(item_weights, n_items)
        dev = torch.device(device) if device is not None else (
            user_ptr.device if isinstance(user_ptr, torch.Tensor) else torch.device("cuda"))
        if dev.type != "cuda":
            raise RuntimeError("BPRSampler: needs a ROCm device (there is no CPU path)")
        ptr = torch.as_tensor(np.asarray(user_ptr) if not isinstance(user_ptr, torch.Tensor) else user_ptr)
        items = torch.as_tensor(np.asarray(user_items) if not isinstance(user_items, torch.Tensor) else user_items)
        self.ptr = ptr.to(dev, torch.int64).contiguous()
        items = items.to(dev, torch.int32).contiguous()
        self.n_users = self.ptr.numel() - 1
        self.nnz = items.numel()
        self.n_items = int(n_items)
        self.device = dev
        if self.n_users < 0:
            raise ValueError("BPRSampler: user_ptr must have n_users + 1 entries")
        self.items_orig = items  # the order given: sample_positives enumerates it
        self.items = torch.empty(max(self.nnz, 1), dtype=torch.int32, device=dev)
        self.eligible = torch.empty(max(self.n_users, 1), dtype=torch.int32, device=dev)
        self.n_eligible = torch.zeros(1, dtype=torch.int64, device=dev)
        _launch.bpr_sampler_prepare(self.ptr, items, self.n_users, self.nnz, self.items, self.eligible,
                                    self.n_eligible)
        self._bad = torch.zeros(1, dtype=torch.int32, device=dev)
        self.pool_tries = None
        if self.weighted:
            # uint64 bits in an int64 tensor (the kernels read them as uint64)
            self.cdf = torch.from_numpy(cdf.view(np.int64)).to(dev)
            self.log_q = torch.from_numpy(log_q).to(dev)
            self.n_positive = int((self.w > 0).sum())

    @staticmethod
    def popularity_weights(user_ptr, user_items, n_items: int, power: float = 0.75) -> np.ndarray:
        """(train count of each item) ^ power, float64 [n_items]: the usual popularity weighting of
        sampled negatives (0.75 as in word2vec); an item without train interactions gets 0."""
        if isinstance(user_items, torch.Tensor):
            user_items = user_items.detach().cpu().numpy()
        cnt = np.bincount(np.asarray(user_items, dtype=np.int64).reshape(-1), minlength=int(n_items))
        if cnt.size != int(n_items):
            raise ValueError("popularity_weights: an item id is outside [0, n_items)")
        return cnt.astype(np.float64) ** float(power)

    def _need_weights(self, what: str):
        if not self.weighted:
            raise ValueError(f"BPRSampler.{what}: the sampler was built without item_weights")

    def correction(self, n_neg: int) -> torch.Tensor:
        """fp32 [n_items] on the device: log(n_neg q_i), what ``hip_ops.softmax_loss(correction=)``
        subtracts from the logits of ``n_neg`` weighted negatives (-inf where q_i = 0: never drawn).
        q is the catalogue-wide distribution; its renormalisation by the mass of each user's
        excluded history is ignored, as is usual."""
        self._need_weights("correction")
        if int(n_neg) < 1:
            raise ValueError("correction: n_neg must be >= 1")
        return torch.from_numpy(logq_correction(self.w, self.total, int(n_neg))).to(self.device)

    def pool_correction(self, tries: int = None) -> torch.Tensor:
        """fp32 [n_items] on the device: log(1 - (1 - q_i)^tries), the log of the probability that
        item i is in a pool cut from ``tries`` weighted draws (default: ``pool_tries`` of the last
        ``sample_pool``), for ``hip_ops.shared_softmax_loss_corrected(correction=)``.  History renormalisation
        ignored, as in ``correction``."""
        self._need_weights("pool_correction")
        tries = self.pool_tries if tries is None else int(tries)
        if tries is None or tries < 1:
            raise ValueError("pool_correction: tries must be >= 1 (draw a pool first, or pass tries)")
        return torch.from_numpy(logq_pool_correction(self.w, self.total, tries)).to(self.device)

    def weighted_draws(self, n: int, seed: int = 42, offset: int = 0) -> torch.Tensor:
        """int64 [n]: weighted draw (seed, offset + k, 0) for k < n (ppgat_weighted_draws)."""
        self._need_weights("weighted_draws")
        out = torch.empty(int(n), dtype=torch.int64, device=self.device)
        _launch.weighted_draws(self.cdf, self.n_items, int(n), seed, int(offset), out)
        return out

    def sample(self, samples: int, seed: int = 42, offset: int = 0, check: bool = True):
        """-> (u, i, j) int64 [samples] on the sampler's device.  ``check`` syncs once to
        raise if no user has items or a negative could not be drawn (user holds ~all items)."""
        out = torch.empty(3, samples, dtype=torch.int64, device=self.device)
        # u and i the same either way; with item weights j is drawn under them
        _launch.bpr_sample(self.ptr, self.items, self.eligible, self.n_eligible, self.n_items, samples, seed,
                           int(offset), out, self._bad, cdf=self.cdf if self.weighted else None)
        if check and samples > 0:
            bad = int(self._bad.item())
            if bad & 1:
                raise ValueError("BPRSampler: no user has train items")
            if bad & 2:
                raise ValueError("BPRSampler: a user holds (almost) every item; no negative found")
        return out[0], out[1], out[2]

    def sample_candidates(self, samples: int, n_neg: int, seed: int = 42, offset: int = 0):
        """-> (u [samples], cand [samples, n_neg + 1]) for ``hip_ops.softmax_loss``: the (u, i) of
        ``sample(samples, seed, offset)`` and, per pair, ``eval_candidates(u, i, n_neg, seed)`` --
        column 0 the positive i, then n_neg negatives outside u's train list.  No kernel of its own.
        With item weights the negatives are ``train_candidates``' (weighted); (u, i) are the same bits."""
        u, i, _ = self.sample(samples, seed=seed, offset=offset)
        return u, self.train_candidates(u, i, n_neg, seed)

    def train_candidates(self, users, pos, n_neg: int, seed: int = 0, check: bool = True) -> torch.Tensor:
        """The training candidates of given (user, positive) pairs, [B, n_neg + 1] int64: with item
        weights, ``eval_candidates``' contract with every draw made under the weights
        (ppgat_weighted_eval_sample); without, ``eval_candidates`` itself."""
        if not self.weighted:
            return self.eval_candidates(users, pos, n_neg, seed, check=check)
        u = torch.as_tensor(users).to(self.device, torch.int64).contiguous()
        p = torch.as_tensor(pos).to(self.device, torch.int64).contiguous()
        if u.numel() != p.numel():
            raise ValueError("train_candidates: users and pos must have the same length")
        cands = torch.empty(u.numel(), int(n_neg) + 1, dtype=torch.int64, device=self.device)
        _launch.eval_sample(self.ptr, self.items, u, p, int(n_neg), self.n_items, seed, cands, self._bad, cdf=self.cdf)
        if check and u.numel() > 0 and int(self._bad.item()) & 2:
            raise ValueError("train_candidates: every item of positive weight is in a user's train list or is "
                             "its positive; no negative found")
        return cands

    def sample_pool(self, n_pool: int, seed: int = 42) -> torch.Tensor:
        """-> ``n_pool`` distinct item ids, uniform over the catalogue, ascending, int64 on the
        sampler's device: the shared negatives of ``hip_ops.shared_softmax_loss``.  A seeded
        torch permutation (not the hot path, no kernel of its own).
        With item weights: the distinct items among the first T weighted draws (seed, k, 0), k < T,
        T the smallest count whose draws hold ``n_pool`` distinct items; T is kept in
        ``self.pool_tries`` (``pool_correction`` needs it).  ValueError if fewer than ``n_pool`` items
        have positive weight or 64 n_pool draws do not suffice."""
        n_pool = int(n_pool)
        if not 1 <= n_pool <= self.n_items:
            raise ValueError(f"sample_pool: n_pool must be in [1, n_items = {self.n_items}], got {n_pool}")
        if self.weighted:
            return self._weighted_pool(n_pool, seed)
        gen = torch.Generator(device=self.device)
        gen.manual_seed(int(seed) & 0x7FFFFFFFFFFFFFFF)
        return torch.randperm(self.n_items, generator=gen, device=self.device)[:n_pool].sort().values.to(torch.int64)

    def _weighted_pool(self, n_pool: int, seed: int) -> torch.Tensor:
        if n_pool > self.n_positive:
            raise ValueError(f"sample_pool: n_pool = {n_pool} but only {self.n_positive} items have positive weight")
        cap = 64 * n_pool
        n = min(4 * n_pool, cap)
        while True:
            d = self.weighted_draws(n, seed)  # a prefix of the same stream whatever n is
            val, idx = torch.sort(d, stable=True)  # equal items stay in draw order: the first is the first draw
            first = torch.ones(n, dtype=torch.bool, device=self.device)
            first[1:] = val[1:] != val[:-1]
            new = torch.zeros(n, dtype=torch.int64, device=self.device)
            new[idx[first]] = 1
            distinct = torch.cumsum(new, 0)  # distinct items among draws 0 .. k
            if int(distinct[-1]) >= n_pool:
                tries = int(torch.searchsorted(distinct, n_pool)) + 1
                self.pool_tries = tries
                return torch.unique(d[:tries])  # sorted ascending
            if n >= cap:
                raise ValueError(f"sample_pool: {cap} weighted draws hold only {int(distinct[-1])} distinct items "
                                 f"(n_pool = {n_pool}): the weights are too concentrated for this pool size")
            n = min(4 * n, cap)

    def sample_positives(self, neg_per_pos: int, batch_size: int, batch: int, seed: int = 42, check: bool = True):
        """Mini-batch ``batch`` of an epoch of sample_bpr_batches (scripts/train_lightgcn.py:160-179)
        -> (u, i, j) int64 [S]: every train interaction in the order given (users in order, each
        user's items in list order) x ``neg_per_pos`` negatives, cut every ``batch_size`` triples
        (the last batch is partial).  (u, i) equal the reference's batches exactly; j is the first
        draw of the counter stream (seed, triple index, d) outside the user's items
        (``ppgat_bpr_sample_positives``)."""
        npp, bs, b = int(neg_per_pos), int(batch_size), int(batch)
        total = self.nnz * npp
        if npp < 1 or bs < 1 or b < 0 or b * bs >= max(total, 1):
            raise ValueError(f"sample_positives: batch {b} of {self.n_batches(npp, bs) if npp > 0 and bs > 0 else 0}")
        t0 = b * bs
        S = min(bs, total - t0)
        out = torch.empty(3, S, dtype=torch.int64, device=self.device)
        _launch.bpr_sample_positives(self.ptr, self.items_orig, self.items, self.n_users, self.nnz, self.n_items, npp,
                                     S, seed, t0, out, self._bad)
        if check and int(self._bad.item()) & 2:
            raise ValueError("BPRSampler: a user holds (almost) every item; no negative found")
        return out[0], out[1], out[2]

    def n_batches(self, neg_per_pos: int, batch_size: int) -> int:
        return -(-(self.nnz * int(neg_per_pos)) // int(batch_size))

    def eval_candidates(self, users, pos, n_neg: int, seed: int = 0, check: bool = True) -> torch.Tensor:
        """eval_sampled's candidates (train_gat_pyg.py:157-167) on the device: [B, n_neg + 1]
        int64, column 0 the held-out positive, then n_neg negatives drawn uniformly from the
        items outside the user's train list and != the positive (ppgat_eval_sample)."""
        u = torch.as_tensor(users).to(self.device, torch.int64).contiguous()
        p = torch.as_tensor(pos).to(self.device, torch.int64).contiguous()
        if u.numel() != p.numel():
            raise ValueError("eval_candidates: users and pos must have the same length")
        cands = torch.empty(u.numel(), int(n_neg) + 1, dtype=torch.int64, device=self.device)
        _launch.eval_sample(self.ptr, self.items, u, p, int(n_neg), self.n_items, seed, cands, self._bad)
        if check and u.numel() > 0 and int(self._bad.item()) & 2:
            raise ValueError("eval_candidates: a user holds (almost) every item; no negative found")
        return cands
