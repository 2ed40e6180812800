"""References of ppgat_infonce and ppgat_relu_dropout, shared by the host and GPU tests.

``infonce`` is the formulae of csrc/ppgat_infonce.hip's header in torch, differentiated by
autograd, in the dtype of its inputs: float64 is the reference, float32 on the CPU is the "plain
fp32 restatement" whose own error against float64 sets the kernel's bound.  ``infonce_loops`` is
the same loss and the header's closed-form backward in plain Python loops, for the host self-check.
``relu_dropout`` restates the ReLU/dropout kernel in numpy, bit for bit.
"""
from __future__ import annotations

import math

import numpy as np
import torch

EPS = 1e-12
U32 = 2.0 ** -24   # fp32 unit roundoff: rounding an exact result to fp32 already costs up to this


def normalize(x, eps=EPS):
    """x / max(|x|, eps) per row (torch F.normalize): below eps the norm's gradient is cut by the
    clamp, so the backward there is dy / eps, as the kernel's |x| <= 1e-12 branch."""
    return x / x.norm(dim=1, keepdim=True).clamp_min(eps)


def infonce(F, T, I, tau):
    """-> (loss [3] = {loss, loss_t, loss_i}, dF, dT, dI, row maxima of S_t and S_i) in F's dtype."""
    F, T, I = (v.detach().clone().requires_grad_(True) for v in (F, T, I))
    Fn, Tn, In = normalize(F), normalize(T), normalize(I)
    St, Si = Fn @ Tn.t() / tau, Fn @ In.t() / tau
    lt = (torch.logsumexp(St, 1) - St.diagonal()).mean()
    li = (torch.logsumexp(Si, 1) - Si.diagonal()).mean()
    loss = (lt + li) / 2
    loss.backward()
    rowmax = torch.maximum(St.detach().max(1).values, Si.detach().max(1).values)
    return torch.stack([loss, lt, li]).detach(), F.grad, T.grad, I.grad, rowmax


def infonce_loops(F, T, I, tau, eps=EPS):
    """The same by loops over Python floats: the loss triple and dF, dT, dI (lists of lists) from
    dS = (softmax(S) - onehot) / (2B), dFn = (dS_t Tn + dS_i In) / tau, dTn = dS_t^T Fn / tau,
    dIn = dS_i^T Fn / tau, dx = (dy - y (y . dy)) / |x| for |x| > eps, dy / eps otherwise."""
    B, D = len(F), len(F[0])

    def norm_rows(X):
        n = [math.sqrt(sum(float(v) ** 2 for v in row)) for row in X]
        return [[float(v) / max(nb, eps) for v in row] for row, nb in zip(X, n)], n

    (Fn, nF), (Tn, nT), (In, nI) = norm_rows(F), norm_rows(T), norm_rows(I)

    def ce(Xn):
        S = [[sum(Fn[b][d] * Xn[c][d] for d in range(D)) / tau for c in range(B)] for b in range(B)]
        l, dS = 0.0, []
        for b in range(B):
            m = max(S[b])
            lse = m + math.log(sum(math.exp(s - m) for s in S[b]))
            l += (lse - S[b][b]) / B
            dS.append([(math.exp(S[b][c] - lse) - (1.0 if c == b else 0.0)) / (2 * B) for c in range(B)])
        return l, dS

    (lt, dSt), (li, dSi) = ce(Tn), ce(In)
    dFn = [[sum(dSt[b][c] * Tn[c][d] + dSi[b][c] * In[c][d] for c in range(B)) / tau for d in range(D)] for b in range(B)]
    dTn = [[sum(dSt[b][c] * Fn[b][d] for b in range(B)) / tau for d in range(D)] for c in range(B)]
    dIn = [[sum(dSi[b][c] * Fn[b][d] for b in range(B)) / tau for d in range(D)] for c in range(B)]

    def norm_bwd(Y, n, dY):
        out = []
        for y, nb, dy in zip(Y, n, dY):
            if nb > eps:
                dot = sum(a * b for a, b in zip(y, dy))
                out.append([(g - a * dot) / nb for a, g in zip(y, dy)])
            else:
                out.append([g / eps for g in dy])
        return out

    return [(lt + li) / 2, lt, li], norm_bwd(Fn, nF, dFn), norm_bwd(Tn, nT, dTn), norm_bwd(In, nI, dIn)


def batch(B, seed=None, D=128):
    """fused rows scaled over six decades down the batch (logspace(-3, 3)), txt_p plain Gaussian,
    img_p scaled by 5: fp32 CPU tensors."""
    g = torch.Generator().manual_seed(B if seed is None else seed)
    F = torch.randn(B, D, generator=g) * torch.logspace(-3, 3, B)[:, None]
    T = torch.randn(B, D, generator=g)
    I = torch.randn(B, D, generator=g) * 5
    return F.float().contiguous(), T.contiguous(), I.contiguous()


def aligned_batch(B=64, seed=7, D=128):
    """F = T + 0.01 noise, I = T + 0.01 noise: every row's own pair dominates its softmax."""
    g = torch.Generator().manual_seed(seed)
    T = torch.randn(B, D, generator=g)
    F = T + 0.01 * torch.randn(B, D, generator=g)
    I = T + 0.01 * torch.randn(B, D, generator=g)
    return F.contiguous(), T.contiguous(), I.contiguous()


def loss_rel(got, ref):
    """Largest relative error over the loss triple; a reference of exactly 0 (B = 1) must be met exactly."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(ref != 0, err / np.abs(ref), np.where(err == 0, 0.0, np.inf))
    return float(rel.max())


def term_scale_rows(got, ref, x, B, tau):
    """max_b |got_b - ref_b| / (1 / (2 B tau |x_b|)): a gradient row's absolute error on the scale of
    the terms it sums (each |dS| <= 1 / (2B), each normalised row has norm 1, then / tau / |x_b|),
    for batches where softmax - onehot cancels and the exact row is far smaller than its terms."""
    got, ref, x = (np.asarray(v.detach().double().cpu().numpy() if torch.is_tensor(v) else v, np.float64) for v in (got, ref, x))
    scale = 1.0 / (2 * B * tau * np.linalg.norm(x, axis=1))
    return float((np.linalg.norm(got - ref, axis=1) / scale).max())


def relu_dropout(z, p, seed, scale_fn, grad=None):
    """ppgat_relu_dropout in numpy fp32.  Forward (grad None): (z > 0 ? z : 0) * mask.  Backward:
    z > 0 ? grad * mask : 0.  ``scale_fn`` is oracle.mlp_dropout_scale (mask = 0 or 1 / (1 - p); 1
    everywhere at p = 0).  -0 and negatives give +0; a positive denormal passes."""
    z = np.asarray(z, np.float32)
    m = scale_fn(seed, z.size, p).reshape(z.shape)
    zero = np.zeros_like(z)
    if grad is None:
        return (np.where(z > 0, z, zero) * m).astype(np.float32)
    return np.where(z > 0, np.asarray(grad, np.float32) * m, zero).astype(np.float32)
