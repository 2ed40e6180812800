"""References for popularity-weighted negative sampling and the logQ-corrected softmax losses, all
on the CPU.

``quantise``        the host quantisation of item weights, restated: w_i = floor(x_i / max(x) 2^32) in
                    float64 (a positive weight never below 1), cdf = inclusive uint64 prefix sum
``wdraw``           one weighted draw: r = mulhi64(r64, total), item = first i with cdf[i] > r
``raw_draws``, ``weighted_eval_sample``, ``weighted_bpr_sample``
                    the three device samplers (csrc/ppgat_sample.hip) bit for bit, on
                    oracle.sampler_oracle's draw64 / below
``pool``            the pool rule: the distinct items of the first T draws, T minimal
``correction64``, ``pool_correction64``
                    log(M q) and log(1 - (1 - q)^T) in float64
``ssm_*`` / ``shs_*`` the float64 references of tests/_ssm_ref.py and tests/_shs_ref.py with the
                    correction subtracted from every negative's logit (never from the positive's)
"""
import numpy as np
import torch

import _shs_ref
import _ssm_ref
from oracle.sampler_oracle import MAX_NEG_DRAWS, below, draw64, prepare


def quantise(weights):
    """-> (w uint64, cdf uint64, total int, q float64)."""
    x = np.asarray(weights, dtype=np.float64)
    w = np.floor(x / x.max() * 2.0 ** 32).astype(np.uint64)
    w[(x > 0) & (w == 0)] = 1
    cdf = np.cumsum(w, dtype=np.uint64)
    total = int(cdf[-1])
    return w, cdf, total, w.astype(np.float64) / float(total)


def wdraw(cdf, r64):
    """Items of the 64-bit draws r64 under the table."""
    r = below(r64, cdf[-1]).astype(np.uint64)
    return np.searchsorted(cdf, r, side="right").astype(np.int64)  # first i with cdf[i] > r


def raw_draws(cdf, n: int, seed: int, t0: int = 0):
    return wdraw(cdf, draw64(seed, np.arange(t0, t0 + n, dtype=np.uint64), 0))


def _keys(user_ptr, user_items, n_items):
    user_ptr = np.asarray(user_ptr, dtype=np.int64)
    items_sorted, eligible = prepare(user_ptr, user_items)
    owner = np.repeat(np.arange(len(user_ptr) - 1, dtype=np.int64), np.diff(user_ptr))
    return user_ptr, items_sorted, eligible, owner * np.int64(n_items) + items_sorted


def _member(keys, q):
    if not len(keys):
        return np.zeros(len(q), dtype=bool)
    return keys[np.minimum(np.searchsorted(keys, q), len(keys) - 1)] == q


def weighted_eval_sample(user_ptr, user_items, users, pos, n_items: int, n_neg: int, seed: int, cdf):
    """ppgat_weighted_eval_sample -> (cands [B, n_neg + 1], bad)."""
    user_ptr, _, _, keys = _keys(user_ptr, user_items, n_items)
    users, pos = np.asarray(users, np.int64), np.asarray(pos, np.int64)
    B = len(users)
    t = (np.arange(B, dtype=np.int64)[:, None] * n_neg + np.arange(n_neg, dtype=np.int64)[None, :]).reshape(-1)
    ub, pb = np.repeat(users, n_neg), np.repeat(pos, n_neg)
    neg = np.full(B * n_neg, -1, np.int64)
    open_ = np.arange(B * n_neg)
    for d in range(MAX_NEG_DRAWS):
        if open_.size == 0:
            break
        c = wdraw(cdf, draw64(seed, t[open_].astype(np.uint64), d))
        hit = _member(keys, ub[open_] * np.int64(n_items) + c) | (c == pb[open_])
        neg[open_[~hit]] = c[~hit]
        open_ = open_[hit]
    bad = 0
    if open_.size:
        neg[open_] = 0
        bad = 2
    return np.concatenate([pos[:, None], neg.reshape(B, n_neg)], 1), bad


def weighted_bpr_sample(user_ptr, user_items, n_items: int, S: int, seed: int, cdf, t0: int = 0):
    """ppgat_weighted_bpr_sample -> (u, i, j, bad): u and i as oracle.sampler_oracle.bpr_sample."""
    user_ptr, items_sorted, eligible, keys = _keys(user_ptr, user_items, n_items)
    t = np.arange(t0, t0 + S, dtype=np.uint64)
    u = eligible[below(draw64(seed, t, 0), len(eligible))]
    lo, hi = user_ptr[u], user_ptr[u + 1]
    i = items_sorted[lo + below(draw64(seed, t, 1), hi - lo)]
    j = np.full(S, -1, dtype=np.int64)
    open_ = np.arange(S)
    for k in range(MAX_NEG_DRAWS):
        if open_.size == 0:
            break
        c = wdraw(cdf, draw64(seed, t[open_], 2 + k))
        hit = _member(keys, u[open_] * np.int64(n_items) + c)
        j[open_[~hit]] = c[~hit]
        open_ = open_[hit]
    bad = 0
    if open_.size:
        j[open_] = 0
        bad = 2
    return u, i.astype(np.int64), j, bad


def pool(w, cdf, n_pool: int, seed: int):
    """-> (items ascending int64 [n_pool], T): T the smallest number of draws (seed, k, 0), k < T, that
    hold n_pool distinct items; ValueError if too few items have positive weight or 64 n_pool draws
    do not suffice."""
    if n_pool > int((np.asarray(w) > 0).sum()):
        raise ValueError("fewer than n_pool items have positive weight")
    d = raw_draws(cdf, 64 * n_pool, seed)
    _, first = np.unique(d, return_index=True)
    if len(first) < n_pool:
        raise ValueError("64 n_pool draws do not hold n_pool distinct items")
    T = int(np.sort(first)[n_pool - 1]) + 1  # the draw that brings the n_pool-th distinct item
    return np.unique(d[:T]), T


def correction64(q, n_neg: int):
    with np.errstate(divide="ignore"):
        return np.log(float(n_neg) * np.asarray(q, np.float64))


def pool_correction64(q, tries: int):
    with np.errstate(divide="ignore"):
        return np.log(-np.expm1(float(tries) * np.log1p(-np.asarray(q, np.float64))))


def make_correction(n_items: int, seed: int = 0):
    """The parity tests' table: 2 N(0, 1), one entry of +80 and one of -80 (fp32 torch tensor)."""
    rng = np.random.default_rng(77 + seed)
    c = (2.0 * rng.standard_normal(n_items)).astype(np.float32)
    hi, lo = rng.choice(n_items, 2, replace=False)
    c[hi], c[lo] = 80.0, -80.0
    return torch.from_numpy(c)


# ---- sampled softmax with a correction (tests/_ssm_ref.py, s[t, m] -= corr[cand[t, m]] for m >= 1) ----
def _ssm_scores(Zd, n_users, u, cand, tau, corr):
    s = (Zd[u].unsqueeze(1) * Zd[n_users + cand]).sum(-1) / tau
    sub = corr.to(Zd.dtype)[cand]
    sub[:, 0] = 0.0
    return s - sub


def ssm_loss_autograd(Z, n_users: int, u, cand, tau: float, corr, upstream: float = 1.0, dtype=torch.float64):
    Zd = Z.detach().to(dtype).requires_grad_(True)
    s = _ssm_scores(Zd, n_users, u, cand, tau, corr)
    loss = (torch.logsumexp(s, dim=1) - s[:, 0]).mean()
    (upstream * loss).backward()
    return loss.detach(), Zd.grad.detach()


def ssm_formulas(Z, n_users: int, u, cand, tau: float, corr, upstream: float = 1.0, dtype=torch.float64):
    Zd = Z.detach().to(dtype)
    S, K1 = cand.shape
    zu, zc = Zd[u], Zd[n_users + cand]
    s = _ssm_scores(Zd, n_users, u, cand, tau, corr)
    loss = (torch.logsumexp(s, dim=1) - s[:, 0]).mean()
    p = torch.softmax(s, dim=1)
    p[:, 0] -= 1.0
    c = p / (max(S, 1) * tau)
    cu = c * upstream
    dZ = torch.zeros_like(Zd)
    dZ.index_add_(0, u, (cu.unsqueeze(-1) * zc).sum(1))
    dZ.index_add_(0, (n_users + cand).reshape(-1), (cu.unsqueeze(-1) * zu.unsqueeze(1)).reshape(S * K1, Zd.size(1)))
    return {"loss": loss, "coef": c, "dZ": dZ}


def ssm_term_scale(Z, n_users: int, u, cand, tau: float, corr, upstream: float = 1.0):
    f = ssm_formulas(Z, n_users, u, cand, tau, corr, upstream)
    Zd = Z.detach().double().abs()
    S, K1 = cand.shape
    ca = (f["coef"] * upstream).abs()
    sc = torch.zeros_like(Zd)
    sc.index_add_(0, u, (ca.unsqueeze(-1) * Zd[n_users + cand]).sum(1))
    sc.index_add_(0, (n_users + cand).reshape(-1), (ca.unsqueeze(-1) * Zd[u].unsqueeze(1)).reshape(S * K1, Zd.size(1)))
    return sc.max(dim=1).values


def ssm_restatement_error(Z, n_users, u, cand, tau, corr, upstream=3.0, abs_floor=0.0):
    f64 = ssm_formulas(Z, n_users, u, cand, tau, corr, upstream, torch.float64)
    f32 = ssm_formulas(Z, n_users, u, cand, tau, corr, upstream, torch.float32)
    sc = ssm_term_scale(Z, n_users, u, cand, tau, corr, upstream)
    lrel = float((f32["loss"].double() - f64["loss"]).abs() / f64["loss"].abs().clamp_min(1e-300))
    return lrel, _ssm_ref.scaled_rows(f32["dZ"], f64["dZ"], sc, abs_floor)[0]


# ---- shared negatives with a correction (tests/_shs_ref.py, s[t, j] -= corr[pool[j]]) ----
def shs_loss_autograd(Z, n_users: int, u, pos, pool_, mask, tau: float, corr, upstream: float = 1.0,
                      dtype=torch.float64):
    Zd = Z.detach().to(dtype).requires_grad_(True)
    U = Zd[u]
    s0 = (U * Zd[n_users + pos]).sum(-1) / tau
    s = (U @ Zd[n_users + pool_].T / tau - corr.to(dtype)[pool_].unsqueeze(0)).masked_fill(mask, float("-inf"))
    loss = (torch.logsumexp(torch.cat([s0.unsqueeze(1), s], 1), dim=1) - s0).mean()
    (upstream * loss).backward()
    return loss.detach(), Zd.grad.detach()


def _shs_coefficients(Z, n_users, u, pos, pool_, mask, tau, corr, dtype=torch.float64):
    Zd = Z.detach().to(dtype)
    S = u.numel()
    U = Zd[u]
    s0 = (U * Zd[n_users + pos]).sum(-1) / tau
    s = (U @ Zd[n_users + pool_].T / tau - corr.to(dtype)[pool_].unsqueeze(0)).masked_fill(mask, float("-inf"))
    m = torch.maximum(s0, s.max(dim=1).values)
    e = torch.exp(s - m.unsqueeze(1))
    en, e0 = e.sum(1), torch.exp(s0 - m)
    tot = en + e0
    term = torch.where(m == s0, torch.log1p(en), (m - s0) + torch.log(tot))
    return term, -(en / tot) / (max(S, 1) * tau), e / tot.unsqueeze(1) / (max(S, 1) * tau)


def shs_term_scale(Z, n_users: int, u, pos, pool_, mask, tau: float, corr, upstream: float = 1.0):
    _, c0, c = _shs_coefficients(Z, n_users, u, pos, pool_, mask, tau, corr)
    Za = Z.detach().double().abs()
    c0a, ca = (c0 * upstream).abs(), (c * upstream).abs()
    U, Ipos, Ipool = Za[u], Za[n_users + pos], Za[n_users + pool_]
    sc = torch.zeros_like(Za)
    sc.index_add_(0, u, c0a.unsqueeze(1) * Ipos + ca @ Ipool)
    sc.index_add_(0, n_users + pos, c0a.unsqueeze(1) * U)
    sc.index_add_(0, n_users + pool_, ca.T @ U)
    return sc.max(dim=1).values


class ShsReference:
    """One _shs_ref case with a correction and its float64 reference (upstream 3.0), computed once."""
    UPSTREAM = 3.0

    def __init__(self, P, C, tau, history=True):
        self.P, self.C, self.tau = P, C, tau
        self.Z, self.u, self.pos, self.pool, self.ptr, self.items = _shs_ref.make_case(P, C)
        if not history:
            self.ptr = self.items = None
        self.corr = make_correction(_shs_ref.N_ITEMS, seed=P)
        self.mask = _shs_ref.dense_mask(self.u, self.pos, self.pool, self.ptr, self.items)
        a = (self.Z, _shs_ref.N_USERS, self.u, self.pos, self.pool, self.mask, tau, self.corr, self.UPSTREAM)
        self.loss, self.dZ = shs_loss_autograd(*a)
        self.scale = shs_term_scale(*a)
