"""References for the sampled-softmax loss (hip_ops.softmax_loss), all on the CPU.

    s[t, m]  = <Z[u_t], Z[n_users + cand[t, m]]> / tau
    loss     = (1/S) sum_t ( logsumexp_m s[t, m] - s[t, 0] )
    c[t, m]  = (softmax_m(s[t, :]) - [m == 0]) / (S tau)
    dZ[u_t]               += sum_m c[t, m] Z[n_users + cand[t, m]]
    dZ[n_users+cand[t,m]] += c[t, m] Z[u_t]

``ref64``     float64 autograd of the loss, evaluated on the same fp32 Z
``formulas``  the explicit formulas in one dtype (float64: must equal autograd; float32: the plain
              fp32 restatement whose own error sets what an fp32 kernel can be asked for)
``term_scale`` scale[r] = sum |c| |source row| over the records that reach row r, per column, max
              over columns: what row r sums before anything cancels
``make_case`` the parity inputs: a hot item, a hot user, items with exactly 1 / 32 / 33 slots
"""
import numpy as np
import torch

N_USERS, N_ITEMS, N_SAMPLES = 300, 200, 2000
HOT_ITEM, HOT_USER = 7, 11
ITEM_ONE, ITEM_32, ITEM_33 = 197, 198, 199  # reserved: placed by construction, never drawn

# the parity cases (M, C, tau) of tests/test_gpu_softmax_loss.py
CASES = [(1, 32, 1.0), (7, 64, 1.0), (64, 64, 1.0), (16, 128, 0.1), (16, 256, 0.1), (16, 32, 0.02)]
EXTREME = (16, 64, 0.01)  # with Z ~ 0.5 N(0, 1): logits reach about +-900
EXTREME_SEED = 1          # (seed 0 makes the single-slot item a positive with p_0 -> 1, see the GPU test)


def make_case(M: int, C: int, seed: int = 0, z_std: float = 0.1, n_users: int = N_USERS, n_items: int = N_ITEMS,
              S: int = N_SAMPLES):
    """-> (Z fp32 [n_users + n_items, C], u int64 [S], cand int64 [S, M + 1]) as torch CPU tensors."""
    rng = np.random.default_rng(1000 * seed + 17 * M + C)
    Z = (z_std * rng.standard_normal((n_users + n_items, C))).astype(np.float32)
    u = rng.integers(0, n_users, S)
    u[rng.random(S) < 1 / 3] = HOT_USER
    K1 = M + 1
    cand = rng.integers(0, n_items - 3, (S, K1))           # the reserved items are the last three
    cand[rng.random((S, K1)) < 1 / 3] = HOT_ITEM           # column 0 included, duplicates in a row
    flat = cand.reshape(-1)
    slots = rng.permutation(flat.size)[:1 + 32 + 33]
    flat[slots[:1]] = ITEM_ONE
    flat[slots[1:33]] = ITEM_32
    flat[slots[33:]] = ITEM_33
    return torch.from_numpy(Z), torch.from_numpy(u.astype(np.int64)), torch.from_numpy(cand.astype(np.int64))


def loss_autograd(Z, n_users: int, u, cand, tau: float, upstream: float = 1.0, dtype=torch.float64):
    """(loss, dZ) by autograd in ``dtype``; dZ is the gradient of upstream * loss."""
    Zd = Z.detach().to(dtype).requires_grad_(True)
    s = (Zd[u].unsqueeze(1) * Zd[n_users + cand]).sum(-1) / tau
    loss = (torch.logsumexp(s, dim=1) - s[:, 0]).mean()
    (upstream * loss).backward()
    return loss.detach(), Zd.grad.detach()


def formulas(Z, n_users: int, u, cand, tau: float, upstream: float = 1.0, dtype=torch.float64):
    """The formulas at the top, written out in ``dtype`` -> dict(loss, coef [S, M + 1], dZ)."""
    Zd = Z.detach().to(dtype)
    S, K1 = cand.shape
    zu, zc = Zd[u], Zd[n_users + cand]                      # [S, C], [S, K1, C]
    s = (zu.unsqueeze(1) * zc).sum(-1) / tau
    loss = (torch.logsumexp(s, dim=1) - s[:, 0]).mean() if S else torch.zeros((), dtype=dtype)
    p = torch.softmax(s, dim=1)
    p[:, 0] -= 1.0
    c = p / (max(S, 1) * tau)
    cu = c * upstream
    dZ = torch.zeros_like(Zd)
    dZ.index_add_(0, u, (cu.unsqueeze(-1) * zc).sum(1))
    dZ.index_add_(0, (n_users + cand).reshape(-1), (cu.unsqueeze(-1) * zu.unsqueeze(1)).reshape(S * K1, Zd.size(1)))
    return {"loss": loss, "coef": c, "dZ": dZ}


def term_scale(Z, n_users: int, u, cand, tau: float, upstream: float = 1.0):
    """scale [n_rows] float64: per row, max over columns of sum |c| |source row| over its records."""
    f = formulas(Z, n_users, u, cand, tau, upstream)
    Zd = Z.detach().double().abs()
    S, K1 = cand.shape
    ca = (f["coef"] * upstream).abs()
    sc = torch.zeros_like(Zd)
    sc.index_add_(0, u, (ca.unsqueeze(-1) * Zd[n_users + cand]).sum(1))
    sc.index_add_(0, (n_users + cand).reshape(-1), (ca.unsqueeze(-1) * Zd[u].unsqueeze(1)).reshape(S * K1, Zd.size(1)))
    return sc.max(dim=1).values


# Softmax weights below the smallest normal fp32 number (exp(-87.3)) are zero or denormal in any
# fp32 evaluation while float64 keeps them, so a row reached only by such records has a term scale
# of 1e-40 and an fp32 error of 100 % of it.  Each such record is wrong by at most FLT_MIN |z|
# upstream / (S tau) < 1e-38 * 1e4; a row holds fewer than 1e6 records, hence this absolute
# allowance, far below any gradient that matters (the extreme-logit case needs it: logits +-900).
UNDERFLOW_ABS = 1e-28


def scaled_rows(a, b, scale, abs_floor: float = 0.0):
    """(max over the rows with scale > 0 of max_col (|a - b| - abs_floor)+ / scale, max |a| over the
    rows with scale == 0): the row-wise gradient figure and what must be exactly 0."""
    a, b, s = a.detach().double().cpu(), b.detach().double().cpu(), scale.detach().double().cpu()
    err = ((a - b).abs().max(dim=1).values - abs_floor).clamp_min(0.0)
    nz = s > 0
    worst = float((err[nz] / s[nz]).max()) if nz.any() else 0.0
    zmax = float(a[~nz].abs().max()) if (~nz).any() else 0.0
    return worst, zmax


def restatement_error(Z, n_users: int, u, cand, tau: float, upstream: float = 3.0, abs_floor: float = 0.0):
    """The plain fp32 CPU restatement against float64 on the same inputs -> (loss relative error,
    dZ per row over the term scale)."""
    f64 = formulas(Z, n_users, u, cand, tau, upstream, torch.float64)
    f32 = formulas(Z, n_users, u, cand, tau, upstream, torch.float32)
    sc = term_scale(Z, n_users, u, cand, tau, upstream)
    lrel = float((f32["loss"].double() - f64["loss"]).abs() / f64["loss"].abs().clamp_min(1e-300))
    return lrel, scaled_rows(f32["dZ"], f64["dZ"], sc, abs_floor)[0]
