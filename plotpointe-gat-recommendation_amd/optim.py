"""Adam on the device in one launch per 16 tensors (include/ppgat.h ppgat_adam_step).

Drop-in for ``torch.optim.Adam(model.parameters(), lr=cfg.lr, weight_decay=cfg.l2)``
(scripts/train_gat_pyg.py:299, train_gat_custom.py's equivalent) with the same
hyper-parameters, the same per-parameter state keys (``step``, ``exp_avg``,
``exp_avg_sq``) and the same update rule (L2 weight decay added to the gradient, bias
corrections, eps after the square root), so optimizer state_dicts move between the two.
Supported: fp32 dense tensors on one ROCm device, amsgrad=False, maximize=False.

``capturable=True`` (torch.optim.Adam's flag of the same name): every parameter's step
count ``state["step"]`` is a device float (as in torch's capturable Adam), incremented with
one multi-tensor launch and turned into the bias corrections on the stream
(``ppgat_adam_step_device``), so ``step()`` can be captured in a hipGraph and replayed; a
parameter without a gradient keeps its count, and saved state has one count per parameter.

Row-sparse gradients (``torch.sparse_coo_tensor`` with one sparse dimension, as
``hip_ops.embedding_rows`` and ``nn.Embedding(sparse=True)`` return them) take the lazy step of
``ppgat_adam_rows``: the same element rule on the rows the gradient names and on no other, so an
untouched row receives no momentum step and no weight decay.  State keys are unchanged and
``step`` stays the parameter's global count.  ``rows="coalesce"`` (default) coalesces a gradient
that is not flagged coalesced -- correct for any sparse gradient; ``rows="ascending"`` takes the
indices as they are under the kernel's contract (strictly ascending, in range), which the kernel
checks into a device flag that ``check_rows()`` reads: one sync there, none in ``step()``.
"""
from __future__ import annotations

import math

import torch

from . import _launch


class Adam(torch.optim.Optimizer):
    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                 amsgrad: bool = False, maximize: bool = False, capturable: bool = False,
                 rows: str = "coalesce"):
        if rows not in ("coalesce", "ascending"):
            raise ValueError(f"ppgat Adam: rows={rows!r} (expected 'coalesce' or 'ascending')")
        if amsgrad or maximize:
            raise NotImplementedError("ppgat Adam: amsgrad / maximize not implemented")
        if not 0.0 <= lr or not 0.0 <= eps or not 0.0 <= weight_decay:
            raise ValueError("invalid Adam hyper-parameter")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"invalid betas {betas}")
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=False,
                                      maximize=False, capturable=bool(capturable)))
        self.rows = rows  # how a sparse gradient's row indices are taken (_step_rows)
        self._row_flags = {}  # device -> int32 [1], OR'd by ppgat_adam_rows, read by check_rows

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        cap = _launch.adam_max_tensors()
        for group in self.param_groups:
            b1, b2 = group["betas"]
            batch = []
            if group.get("capturable", False):
                self._step_device(cap, group)
                continue
            for p in group["params"]:
                if p.grad is None:
                    continue
                g = p.grad
                if g.is_sparse:
                    self._step_rows(p, g, group, b1, b2)
                    continue
                if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() and g.is_contiguous()
                        and g.dtype == torch.float32):
                    raise RuntimeError("ppgat Adam: fp32 contiguous ROCm parameters and gradients only")
                st = self.state[p]
                if len(st) == 0:
                    st["step"] = torch.tensor(0.0)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                st["step"] += 1
                t = float(st["step"].item())
                batch.append((p, g, st["exp_avg"], st["exp_avg_sq"], group["lr"] / (1.0 - b1 ** t),
                              math.sqrt(1.0 - b2 ** t)))
                if len(batch) == cap:
                    self._step_dense(batch, group, b1, b2)
                    batch = []
            if batch:
                self._step_dense(batch, group, b1, b2)
        return loss

    def _step_device(self, cap, group):
        b1, b2 = group["betas"]
        ps = [p for p in group["params"] if p.grad is not None]
        if not ps:
            return
        for p in ps:
            g = p.grad
            if g.is_sparse:
                raise NotImplementedError("ppgat Adam: capturable=True with a sparse gradient is not implemented "
                                          "(the number of rows varies from step to step)")
            if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() and g.is_contiguous()
                                   and g.dtype == torch.float32):
                raise RuntimeError("ppgat Adam: fp32 contiguous dense ROCm parameters and gradients only")
            st = self.state[p]
            if len(st) == 0:
                st["step"] = torch.zeros((), dtype=torch.float32, device=p.device)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            elif not (st["step"].is_cuda and st["step"].device == p.device and st["step"].dtype == torch.float32):
                # a state_dict loaded from a host-step run: the count moves to the device once
                st["step"] = st["step"].to(device=p.device, dtype=torch.float32).reshape(())
        steps = [self.state[p]["step"] for p in ps]
        torch._foreach_add_(steps, 1.0)  # one launch, on the stream: graph replays advance every count
        for k in range(0, len(ps), cap):
            chunk = ps[k:k + cap]
            st = [self.state[p] for p in chunk]
            _launch.adam_step_device(chunk, [p.grad for p in chunk], [s["exp_avg"] for s in st],
                                     [s["exp_avg_sq"] for s in st], [s["step"] for s in st], group["lr"], b1, b2,
                                     group["eps"], group["weight_decay"])

    def _step_rows(self, p, g, group, b1, b2):
        """The lazy step of one 2-D table on the rows its sparse gradient names (ppgat_adam_rows)."""
        if not (p.is_cuda and p.dtype == torch.float32 and p.dim() == 2 and p.is_contiguous()):
            raise RuntimeError("ppgat Adam: a sparse gradient needs a 2-D fp32 contiguous ROCm parameter")
        if not (g.sparse_dim() == 1 and g.dense_dim() == 1 and g.dtype == torch.float32 and g.shape == p.shape
                and g.device == p.device):
            raise RuntimeError("ppgat Adam: sparse gradients must be fp32 row-sparse (sparse_dim 1) of the parameter's "
                               "shape")
        st = self.state[p]
        if len(st) == 0:
            st["step"] = torch.tensor(0.0)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
        st["step"] += 1
        t = float(st["step"].item())
        if not g.is_coalesced() and self.rows == "coalesce":
            g = g.coalesce()
        idx, val = g._indices()[0].contiguous(), g._values().contiguous()
        if idx.numel() == 0:  # no row touched: the count advanced, nothing to launch
            return
        flag = self._row_flags.get(p.device)
        if flag is None:
            flag = self._row_flags[p.device] = torch.zeros(1, dtype=torch.int32, device=p.device)
        _launch.adam_rows(p, st["exp_avg"], st["exp_avg_sq"], val, idx, group["lr"] / (1.0 - b1 ** t),
                          math.sqrt(1.0 - b2 ** t), b1, b2, group["eps"], group["weight_decay"], flag)

    def check_rows(self):
        """Read and clear the row-contract flag of every sparse step so far (one sync): raises
        RuntimeError if a gradient's row indices were out of range or not strictly ascending --
        the steps since the last check are then invalid (``rows="ascending"`` trusts the caller)."""
        bad = 0
        for flag in self._row_flags.values():
            bad |= int(flag.item())
            flag.zero_()
        what = []
        if bad & 1:
            what.append("a row index outside the range [0, n_table_rows) (skipped, not applied)")
        if bad & 2:
            what.append("row indices out of order: not strictly ascending (repeated or descending)")
        if what:
            raise RuntimeError("ppgat Adam: sparse-gradient contract violated: " + "; ".join(what))

    @staticmethod
    def _step_dense(batch, group, b1, b2):
        dev = batch[0][0].device
        for p, *_ in batch:
            if p.device != dev:
                raise RuntimeError("ppgat Adam: all parameters of a group must be on one device")
        P, G, M, V, SS, BC = (list(c) for c in zip(*batch))
        _launch.adam_step(P, G, M, V, SS, BC, b1, b2, group["eps"], group["weight_decay"])
