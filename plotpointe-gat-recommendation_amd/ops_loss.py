"""The fused losses behind hip_ops: BPR / BCE (with the prepared backward and the producer hand-off),
the sampled-softmax and shared-negatives softmax losses with their logQ corrections, and the
deferred index checks (``_BadIndex``).  Each loss keeps its workspace on its autograd context.
"""
from __future__ import annotations

import weakref
from typing import Optional

import torch

from . import _launch, _lib
from .ops_gat import _producer_fusion_enabled, _producer_of, _side_stream
from .ops_graph import _check_dev, _require


LOSS_KINDS = {"bpr": 0, "bce": 1}


class _BadIndex:
    """Out-of-range u/i/j are clamped on the device and counted; the count is copied to
    pinned host memory asynchronously and checked at the next loss call (or by
    ``check_bpr_indices()``), so the hot path never waits on the host."""
    pending = []

    @classmethod
    def track(cls, bad: torch.Tensor, error=None):
        """``error``: (exception type, message with one ``{}`` for the count) raised in place of
        the IndexError when the count is not zero."""
        if torch.cuda.is_current_stream_capturing():  # a captured step: no host copy / event query
            return
        host = torch.empty(1, dtype=torch.int32, pin_memory=True)
        host.copy_(bad, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        cls.pending.append((ev, host, error))

    @classmethod
    def raise_pending(cls, wait: bool = False):
        if torch.cuda.is_current_stream_capturing():
            return
        keep = []
        for ev, host, error in cls.pending:
            if wait:
                ev.synchronize()
            if wait or ev.query():
                if int(host.item()) != 0:
                    cls.pending = []
                    if error is not None:
                        raise error[0](error[1].format(int(host.item())))
                    raise IndexError(f"bpr_loss: {int(host.item())} triples with u/i/j out of range")
            else:
                keep.append((ev, host, error))
        cls.pending = keep


def check_bpr_indices():
    """Raise IndexError if any earlier bpr_loss call saw out-of-range indices (syncs)."""
    _BadIndex.raise_pending(wait=True)


class BprPrepared:
    """The triple-only half of the loss backward (ppgat_bpr_bwd_prepare), launched on a side
    stream: made before the model's forward it runs beside it.  Hand it to ``bpr_loss(...,
    prepared=)`` with the same triples and Z shape; the loss joins the side stream back into
    the current one after its own forward kernels, so nothing after the loss can see a
    half-built workspace and the workspace is not freed under the side stream."""

    def __init__(self, n_rows: int, n_users: int, n_items: int, C: int, u, i, j, row_map=None):
        dev = u.device
        _require(u.is_cuda, "bpr_prepare: ppgat runs on ROCm devices only; there is no CPU path")
        if C not in (32, 64, 128, 256):
            raise NotImplementedError("bpr_loss: hidden size must be 32/64/128/256")
        self.given = tuple(t.data_ptr() for t in (u, i, j))
        self.u, self.i, self.j = (t.contiguous().to(torch.int64) for t in (u, i, j))
        for name, t in (("u", self.u), ("i", self.i), ("j", self.j)):
            _check_dev(name, t, torch.int64, dev)
        if row_map is not None:
            _check_dev("row_map", row_map, torch.int32, dev)
        self.row_map = row_map
        self.meta = (int(n_rows), int(n_users), int(n_items), int(C), self.u.numel())
        self.ws = _launch.bpr_workspace(int(n_rows), self.u.numel(), int(C), dev)
        main = torch.cuda.current_stream(dev)
        self.side = _side_stream(dev)
        self.side.wait_stream(main)  # the triples and the workspace come from the current stream
        _launch.bpr_bwd_prepare(int(n_rows), int(n_users), int(n_items), row_map, int(C), self.u, self.i, self.j,
                                self.ws, self.side)
        # the side stream uses these blocks: if the handle is dropped unconsumed (a failed take(),
        # a forward that raised), the allocator must not hand them to current-stream work before
        # the prepare kernels are done
        for t in (self.ws, self.u, self.i, self.j):
            t.record_stream(self.side)
        self.used = False

    def take(self, n_rows, n_users, n_items, C, u, i, j, row_map):
        """(u, i, j, workspace) of this handle, after checking it was made for exactly this
        call (the same triple tensors, sizes and row map), once."""
        _require(not self.used, "bpr_loss: a prepared handle serves one loss call")
        _require(self.meta == (n_rows, n_users, n_items, C, u.numel())
                 and self.given == tuple(t.data_ptr() for t in (u, i, j))
                 and _lib.ptr(row_map) == _lib.ptr(self.row_map),
                 "bpr_loss: prepared for other triples / sizes")
        self.used = True
        return self.u, self.i, self.j, self.ws


def bpr_prepare(n_rows: int, n_users: int, n_items: int, C: int, u, i, j, row_map=None) -> BprPrepared:
    """Start the triple-only half of the loss backward on a side stream (see BprPrepared)."""
    return BprPrepared(n_rows, n_users, n_items, C, u, i, j, row_map)


class _BPRLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, Z, u, i, j, n_users: int, n_items: int, kind: int, row_map, prep=None, grad_rows: int = 0,
                grad_buf=None):
        ctx.grad_rows = int(grad_rows)
        ctx.grad_buf = grad_buf
        # Z straight from a heads = 1 GATLayer: the loss backward also does that layer's prologue
        ctx.producer = (_producer_of(Z, N=Z.size(0), C=Z.size(1))
                        if (row_map is None and prep is None and _producer_fusion_enabled()) else None)
        Z = Z.contiguous()
        _check_dev("Z", Z, torch.float32)
        n_rows, C = Z.shape
        S = u.numel()
        if prep is not None:
            u, i, j, ws = prep.take(n_rows, n_users, n_items, C, u, i, j, row_map)
        u, i, j = (t.contiguous().to(torch.int64) for t in (u, i, j))
        for name, t in (("u", u), ("i", i), ("j", j)):
            _check_dev(name, t, torch.int64, Z.device)
        if row_map is not None:
            _check_dev("row_map", row_map, torch.int32, Z.device)
        _BadIndex.raise_pending()
        if prep is None:
            ws = _launch.bpr_workspace(n_rows, S, C, Z.device)
        loss = torch.empty(1, dtype=torch.float32, device=Z.device)
        coef = torch.empty(max(S, 1), 2, dtype=torch.float32, device=Z.device)
        bad = torch.empty(1, dtype=torch.int32, device=Z.device)
        # the forward only touches the workspace's block partials, which the prepare leaves alone
        _launch.bpr_fwd(Z, n_users, n_items, row_map, u, i, j, kind, loss, coef, bad, ws)
        if prep is not None:
            torch.cuda.current_stream(Z.device).wait_stream(prep.side)
        _BadIndex.track(bad)
        ctx.save_for_backward(Z, u, i, j, coef)
        ctx.ws = ws
        ctx.prepared = prep is not None
        ctx.row_map = row_map
        ctx.meta = (n_rows, n_users, n_items, C, S)
        return loss.view(())  # (a view: its backward is a reshape, where loss[0]'s is a zero fill + copy)

    @staticmethod
    def backward(ctx, gl):
        Z, u, i, j, coef = ctx.saved_tensors
        n_rows, n_users, n_items, C, S = ctx.meta
        gl = gl.reshape(1).to(torch.float32).contiguous()
        # grad_rows > n_rows: dZ is the top of a [grad_rows, C] buffer (the halo partition's top
        # layer takes the buffer as its gradient table, dist._halo_xgat_backward_deferred_d)
        # (``grad_buf``: that buffer, the caller's persistent one -- its rows past n_rows are the caller's)
        buf, ctx.grad_buf = ctx.grad_buf, None
        if buf is not None:
            _require(buf.dim() == 2 and buf.size(0) >= n_rows and buf.size(1) == C and buf.dtype == Z.dtype and
                     buf.device == Z.device and buf.is_contiguous(), "bpr: grad_buf must be a contiguous "
                     "[>= n_rows, C] buffer of Z's dtype and device")
            dZ = buf[:n_rows]
        else:
            dZ = (torch.empty(ctx.grad_rows, C, dtype=Z.dtype, device=Z.device)[:n_rows] if ctx.grad_rows > n_rows
                  else torch.empty_like(Z))
        ws = ctx.ws
        prod, ctx.producer = ctx.producer, None
        if prod is not None and prod.pro_state is not None:
            # also the producing layer's backward prologue (its nstate and dbias) from dZ
            pb, ps_dst, pm, pinv_l = prod.pro_state
            p_nstate = torch.empty(n_rows, 1, 4, dtype=torch.float32, device=Z.device)
            p_dbias = torch.empty(C, dtype=torch.float32, device=Z.device) if pb is not None else None
            _launch.bpr_bwd_producer(Z, n_users, n_items, u, i, j, coef, gl, dZ, pb, ps_dst, pm, pinv_l, p_nstate,
                                     p_dbias, ws)
            prod.pro_result = (weakref.ref(dZ), dZ._version, p_nstate, p_dbias)
        else:
            _launch.bpr_bwd(Z, n_users, n_items, ctx.row_map, u, i, j, coef, gl, dZ, ws, prepared=ctx.prepared)
        ctx.ws = None
        return dZ, None, None, None, None, None, None, None, None, None, None


def bpr_loss(Z: torch.Tensor, n_users: int, u, i, j, loss: str = "bpr", prepared: BprPrepared = None) -> torch.Tensor:
    """Fused loss of train_gat_pyg.py:313-322 (``loss`` in {"bpr", "bce"}); ``prepared`` from
    ``bpr_prepare`` (made before the forward) moves the backward's sort off the critical path."""
    _require(Z.is_cuda, "bpr_loss: ppgat runs on ROCm devices only; there is no CPU path")
    if Z.size(1) not in (32, 64, 128, 256):
        raise NotImplementedError("bpr_loss: hidden size must be 32/64/128/256")
    return _BPRLoss.apply(Z, u, i, j, int(n_users), Z.size(0) - int(n_users), LOSS_KINDS[loss], None, prepared)


def _check_correction(who: str, correction, Z: torch.Tensor, n_items: int) -> torch.Tensor:
    """The logQ table of a softmax loss: fp32 [n_items] on Z's device, no gradient (raises before
    any launch otherwise)."""
    if not isinstance(correction, torch.Tensor) or correction.dtype != torch.float32 or correction.dim() != 1:
        raise ValueError(f"{who}: correction must be a 1-D float32 tensor")
    if correction.numel() != n_items:
        raise ValueError(f"{who}: correction must have one entry per item ({n_items}), got {correction.numel()}")
    if correction.device != Z.device:
        raise ValueError(f"{who}: correction must be on Z's device ({Z.device}), got {correction.device}")
    return correction.detach().contiguous()


def _track_correction(who: str, used: torch.Tensor):
    """One device check of the correction terms a call subtracts (``used`` = correction[negatives]):
    -inf (an item the sampler never draws) and NaN are refused, deferred like the index checks."""
    bad = (~(used > float("-inf"))).sum().to(torch.int32).reshape(1)  # NaN > -inf is False too
    _BadIndex.track(bad, (ValueError, who + ": {} correction terms of sampled negatives are -inf or NaN (an item of "
                                            "zero sampling weight among the negatives?)"))


class _SoftmaxLoss(torch.autograd.Function):
    """Sampled-softmax loss (ppgat_ssm_fwd / ppgat_ssm_bwd).  No producer hand-off: the layer
    that produced Z takes its ordinary backward prologue."""

    @staticmethod
    def forward(ctx, Z, u, cand, n_users: int, n_items: int, temperature: float, corr=None):
        # Z straight from a GATLayer: a hand-off an earlier consumer left on that node is stale
        # for the gradient this loss returns -- dropped in backward, never made here
        ctx.producer = _producer_of(Z, N=Z.size(0), C=Z.size(1))
        Z = Z.contiguous()
        _check_dev("Z", Z, torch.float32)
        n_rows, C = Z.shape
        S, K1 = cand.shape
        u, cand = u.contiguous(), cand.contiguous()
        _check_dev("u", u, torch.int64, Z.device)
        _check_dev("cand", cand, torch.int64, Z.device)
        _BadIndex.raise_pending()
        ws = _launch.ssm_workspace(n_rows, S, K1, C, Z.device)
        loss = torch.empty(1, dtype=torch.float32, device=Z.device)
        coef = torch.empty(max(S, 1), K1, dtype=torch.float32, device=Z.device)
        bad = torch.empty(1, dtype=torch.int32, device=Z.device)
        if corr is not None and S > 0:
            _track_correction("softmax_loss", corr[cand[:, 1:].clamp(0, n_items - 1)])
        _launch.ssm_fwd(Z, n_users, n_items, u, cand, temperature, loss, coef, bad, ws, corr)
        _BadIndex.track(bad)
        ctx.save_for_backward(Z, u, cand, coef)
        ctx.ws = ws
        ctx.meta = (n_rows, n_users, n_items, C, S, K1, temperature)
        ctx.corrected = corr is not None
        return loss.view(())

    @staticmethod
    def backward(ctx, gl):
        Z, u, cand, coef = ctx.saved_tensors
        n_rows, n_users, n_items, C, S, K1, temperature = ctx.meta
        gl = gl.reshape(1).to(torch.float32).contiguous()
        dZ = torch.empty_like(Z)
        prod, ctx.producer = ctx.producer, None
        if prod is not None:
            prod.pro_result = None
        _launch.ssm_bwd(Z, n_users, n_items, u, cand, temperature, coef, gl, dZ, ctx.ws)
        ctx.ws = None
        return (dZ,) + (None,) * (6 if ctx.corrected else 5)  # (one per input of this apply)


def softmax_loss(Z: torch.Tensor, n_users: int, u, cand, temperature: float = 1.0, correction=None) -> torch.Tensor:
    """Sampled-softmax loss: ``cand`` [S, M + 1] int64 item ids, column 0 the positive of user
    ``u[t]``, the rest its sampled negatives (``BPRSampler.sample_candidates``);
    ``mean_t(logsumexp_m s[t, m] - s[t, 0])`` with ``s = <Z[u], Z[n_users + cand]> / temperature``.
    Fused forward and a deterministic backward (no float atomics).
    ``correction`` (fp32 [n_items], e.g. ``BPRSampler.correction(M)``): the logQ term of negatives
    that were not drawn uniformly, ``s[t, m] -= correction[cand[t, m]]`` for m >= 1, never for the
    positive; it takes no gradient, and the terms the call uses must not be -inf or NaN."""
    if not isinstance(cand, torch.Tensor) or cand.dim() != 2 or cand.dtype != torch.int64 or cand.size(1) < 2:
        raise ValueError("softmax_loss: cand must be a 2-D int64 tensor [S, M + 1] with at least 2 columns")
    if not isinstance(u, torch.Tensor) or u.dtype != torch.int64 or u.numel() != cand.size(0):
        raise ValueError("softmax_loss: u must be an int64 tensor with one user per row of cand")
    temperature = float(temperature)
    if not (temperature > 0.0 and temperature != float("inf")):
        raise ValueError("softmax_loss: temperature must be finite and > 0")
    _require(Z.is_cuda, "softmax_loss: ppgat runs on ROCm devices only; there is no CPU path")
    if Z.dim() != 2 or Z.size(1) not in (32, 64, 128, 256):
        raise NotImplementedError("softmax_loss: hidden size must be 32/64/128/256")
    if correction is None:
        return _SoftmaxLoss.apply(Z, u.reshape(-1), cand, int(n_users), Z.size(0) - int(n_users), temperature)
    corr = _check_correction("softmax_loss", correction, Z, Z.size(0) - int(n_users))
    return _SoftmaxLoss.apply(Z, u.reshape(-1), cand, int(n_users), Z.size(0) - int(n_users), temperature, corr)


class _SharedSoftmaxLoss(torch.autograd.Function):
    """Shared-negatives softmax loss (ppgat_shs_fwd / ppgat_shs_bwd).  No producer hand-off: the
    layer that produced Z takes its ordinary backward prologue."""

    @staticmethod
    def forward(ctx, Z, u, pos, pool, hist_ptr, hist_items, n_users: int, n_items: int, temperature: float,
                corr=None):
        # Z straight from a GATLayer: a hand-off an earlier consumer left on that node is stale
        # for the gradient this loss returns -- dropped in backward, never made here
        ctx.producer = _producer_of(Z, N=Z.size(0), C=Z.size(1))
        Z = Z.contiguous()
        _check_dev("Z", Z, torch.float32)
        n_rows, C = Z.shape
        S, P = u.numel(), pool.numel()
        u, pos, pool = u.contiguous(), pos.contiguous(), pool.contiguous()
        for name, t in (("u", u), ("pos", pos), ("pool", pool)):
            _check_dev(name, t, torch.int64, Z.device)
        if hist_ptr is not None:
            _check_dev("history ptr", hist_ptr, torch.int64, Z.device)
            _check_dev("history items", hist_items, torch.int32, Z.device)
        _BadIndex.raise_pending()
        ws = _launch.shs_workspace(n_rows, S, P, C, corr is not None, Z.device)
        loss = torch.empty(1, dtype=torch.float32, device=Z.device)
        lse = torch.empty(max(S, 1), dtype=torch.float32, device=Z.device)
        c0 = torch.empty(max(S, 1), dtype=torch.float32, device=Z.device)
        bad = torch.empty(2, dtype=torch.int32, device=Z.device)
        if corr is not None:
            _track_correction("shared_softmax_loss", corr[pool.clamp(0, n_items - 1)])
        _launch.shs_fwd(Z, n_users, n_items, u, pos, pool, hist_ptr, hist_items, temperature, loss, lse, c0, bad, ws,
                        corr)
        _BadIndex.track(bad[1:], (ValueError, "shared_softmax_loss: pool must be strictly ascending "
                                              "({} entries not above their predecessor)"))
        _BadIndex.track(bad[:1], (IndexError, "shared_softmax_loss: {} of u/pos/pool out of range"))
        ctx.save_for_backward(Z, u, pos, pool, lse, c0)
        ctx.ws = ws  # the mask words (and gathered corrections) the forward left: the backward reads them
        ctx.corrected = corr is not None
        ctx.meta = (n_rows, n_users, n_items, C, S, P, temperature)
        return loss.view(())

    @staticmethod
    def backward(ctx, gl):
        Z, u, pos, pool, lse, c0 = ctx.saved_tensors
        n_rows, n_users, n_items, C, S, P, temperature = ctx.meta
        gl = gl.reshape(1).to(torch.float32).contiguous()
        dZ = torch.empty_like(Z)
        prod, ctx.producer = ctx.producer, None
        if prod is not None:
            prod.pro_result = None
        _launch.shs_bwd(Z, n_users, n_items, u, pos, pool, temperature, lse, c0, gl, dZ, ctx.ws, ctx.corrected)
        ctx.ws = None
        return (dZ,) + (None,) * (9 if ctx.corrected else 8)  # (one per input of this apply)


def shared_softmax_loss(Z: torch.Tensor, n_users: int, u, pos, pool, temperature: float = 1.0,
                        history=None) -> torch.Tensor:
    """Softmax loss with negatives shared across the batch: every positive ``pos[t]`` of user
    ``u[t]`` is scored against the same ``pool`` [P] of item ids (int64, strictly ascending, e.g.
    ``BPRSampler.sample_pool``); ``mean_t(log(exp(s0) + sum_j exp(s[t, j])) - s0)`` over the pool
    items that are neither the sample's positive nor in its user's ``history`` (a ``BPRSampler``
    or its ``(ptr, items)`` pair; None: only the positive is masked).  The scores are a
    matrix-core product that is never written; deterministic backward (no float atomics).
    A pool that was not drawn uniformly takes ``shared_softmax_loss_corrected``."""
    return shared_softmax_loss_corrected(Z, n_users, u, pos, pool, temperature, history=history, correction=None)


def shared_softmax_loss_corrected(Z: torch.Tensor, n_users: int, u, pos, pool, temperature: float = 1.0,
                                  history=None, correction=None) -> torch.Tensor:
    """``shared_softmax_loss`` with a logQ term: ``correction`` (fp32 [n_items], e.g.
    ``BPRSampler.pool_correction()``) is subtracted from the logit of every pool entry,
    ``s[t, j] -= correction[pool[j]]``, never from the positive's own logit; it takes no gradient,
    and the pool's terms must not be -inf or NaN.  ``None``: the uncorrected entries and code path."""
    for name, t in (("u", u), ("pos", pos), ("pool", pool)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or t.dim() != 1:
            raise ValueError(f"shared_softmax_loss: {name} must be a 1-D int64 tensor")
    if u.numel() != pos.numel():
        raise ValueError("shared_softmax_loss: u and pos must have one entry per sample")
    if pool.numel() < 1:
        raise ValueError("shared_softmax_loss: pool must hold at least one item")
    temperature = float(temperature)
    if not (temperature > 0.0 and temperature != float("inf")):
        raise ValueError("shared_softmax_loss: temperature must be finite and > 0")
    _require(Z.is_cuda, "shared_softmax_loss: ppgat runs on ROCm devices only; there is no CPU path")
    if Z.dim() != 2 or Z.size(1) not in (64, 128):
        raise NotImplementedError("shared_softmax_loss: hidden size must be 64/128")
    hist_ptr = hist_items = None
    if history is not None:
        hist_ptr, hist_items = (history.ptr, history.items) if hasattr(history, "ptr") else history
        if hist_ptr.numel() != int(n_users) + 1:
            raise ValueError("shared_softmax_loss: history ptr must have n_users + 1 entries")
    if correction is None:
        return _SharedSoftmaxLoss.apply(Z, u, pos, pool, hist_ptr, hist_items, int(n_users),
                                        Z.size(0) - int(n_users), temperature)
    corr = _check_correction("shared_softmax_loss", correction, Z, Z.size(0) - int(n_users))
    return _SharedSoftmaxLoss.apply(Z, u, pos, pool, hist_ptr, hist_items, int(n_users), Z.size(0) - int(n_users),
                                    temperature, corr)


def bpr_loss_mapped(Z: torch.Tensor, n_users: int, n_items: int, row_map: torch.Tensor, u, i, j,
                    loss: str = "bpr", prepared: BprPrepared = None, grad_rows: int = 0,
                    grad_buf: Optional[torch.Tensor] = None) -> torch.Tensor:
    """bpr_loss over a Z whose rows are laid out by row_map (node id -> row).  ``grad_rows``: the
    gradient of Z is the top of a buffer of that many rows (the rest is the caller's);
    ``grad_buf``: that buffer, supplied by the caller (kept across steps)."""
    if Z.size(1) not in (32, 64, 128, 256):
        raise NotImplementedError("bpr_loss: hidden size must be 32/64/128/256")
    return _BPRLoss.apply(Z, u, i, j, int(n_users), int(n_items), LOSS_KINDS[loss], row_map, prepared, grad_rows,
                          grad_buf)
