"""The matrix-core GEMM wrappers behind hip_ops: the fused projection, the TN weight-gradient products
(small, segmented and the big fp16-split kernel with its column bounds), the general NN GEMM and
its zero-padding front end, the ``linear`` autograd function, row joins and row-sparse embedding
rows.  ``_CONST_BOUNDS`` (the cached column bounds of constant operands) is this module's state.
"""
from __future__ import annotations

import weakref
from typing import Optional

import torch

from . import _launch
from .ops_graph import _check_dev, _check_rows, _require


def project_supported(k: int, out_cols: int) -> bool:
    return _launch.project_supported(k, out_cols)


def project(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None,
            att_src: Optional[torch.Tensor] = None, att_dst: Optional[torch.Tensor] = None,
            x_items: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None):
    """y = [x; x_items] W^T (+ bias) on the matrix cores (include/ppgat.h ppgat_project), with
    s_src = y.att_src and s_dst = y.att_dst fused when att_src is given (heads = 1).
    Returns y (``out`` if given: contiguous [rows, HC]), or (y, s_src, s_dst)."""
    _check_dev("x", x, torch.float32)
    _check_dev("weight", weight, torch.float32, x.device)
    if x_items is not None and x.size(0) == 0:
        x, x_items = x_items, None
    split = x.size(0)
    n = split + (x_items.size(0) if x_items is not None else 0)
    if x_items is not None:
        _check_dev("x_items", x_items, torch.float32, x.device)
    K, HC = weight.size(1), weight.size(0)
    dev = x.device
    y = out if out is not None else torch.empty(n, HC, dtype=torch.float32, device=dev)
    s_src = s_dst = None
    if att_src is not None:
        s_src = torch.empty(n, dtype=torch.float32, device=dev)
        s_dst = torch.empty(n, dtype=torch.float32, device=dev)
    _launch.project(x, x.stride(0) if x.dim() == 2 and split > 1 else K, x_items,
                    (x_items.stride(0) if x_items.size(0) > 1 else K) if x_items is not None else 0, split, n, weight,
                    bias, att_src, att_dst, y, s_src, s_dst)
    return y if att_src is None else (y, s_src, s_dst)


def weight_grads(G, GV, W, a_s, a_d, heads: int, C: int):
    """dW, datt_src, datt_dst from G = dh_msg^T x and GV = [ds_src; ds_dst]^T x (ppgat_weight_grads)."""
    HC, K = W.shape
    dev = W.device
    dW = torch.empty(HC, K, dtype=torch.float32, device=dev)
    datt_src = torch.empty(heads, C, dtype=torch.float32, device=dev)
    datt_dst = torch.empty(heads, C, dtype=torch.float32, device=dev)
    _launch.weight_grads(G, GV, W, a_s, a_d, heads, C, dW, datt_src, datt_dst)
    return dW, datt_src, datt_dst


# ---------------------------------------------------------------------------
# the TN weight-gradient product and the projection built on it
# ---------------------------------------------------------------------------
_CONST_BOUNDS = {}


def _const_colmax(t: torch.Tensor) -> torch.Tensor:
    """colmax_abs(t) for a tensor the step does not change (the item features of the config-5
    projection's weight gradient): computed once per (tensor object, version, storage and data
    pointers, shape), so the column-max pass over it leaves the training step.  Only tensors the
    step does not differentiate reach it (_Linear's ``x_const``); a raw-pointer write that keeps
    all of these is the caller's to avoid."""
    key = (t._version, t.data_ptr(), t.untyped_storage().data_ptr(), tuple(t.shape), tuple(t.stride()))
    e = _CONST_BOUNDS.get(id(t))
    if e is not None and e[0]() is t and e[1] == key:
        return e[2]
    bits = colmax_abs(t)
    for k in [k for k, v in _CONST_BOUNDS.items() if v[0]() is None]:
        del _CONST_BOUNDS[k]
    _CONST_BOUNDS[id(t)] = (weakref.ref(t), key, bits)
    return bits


def gemm_tn(A: torch.Tensor, B: torch.Tensor, want_colsum: bool = False, V: Optional[torch.Tensor] = None,
            B_items: Optional[torch.Tensor] = None, b_const: bool = False):
    """A [N,M], B [N,K] (row strides may exceed the widths) -> (A^T B [M,K], colsum(A) [M]
    or None, V^T B [nv,K] or None), deterministic.  With ``B_items`` the B rows are
    cat(B, B_items) (two row segments, not concatenated).  ``b_const``: B does not change between
    calls (its column bound for the fp16 TN kernel is cached, _const_colmax)."""
    for name, t in (("A", A), ("B", B)) + ((("B_items", B_items),) if B_items is not None else ()):
        _require(isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32,
                 f"gemm_tn: {name} must be an fp32 ROCm tensor")
        _require(t.dim() == 2 and t.stride(1) == 1, f"gemm_tn: {name} must be 2-D with unit column stride")
    split = B.size(0)
    nb = split + (B_items.size(0) if B_items is not None else 0)
    _require(A.size(0) == nb, "gemm_tn: A [N,M], B [N,K]")
    if A.size(1) == 0 or B.size(1) == 0 or nb == 0:  # empty product or empty reduction: zeros
        M0, K0, nv0 = A.size(1), B.size(1), (0 if V is None else V.size(1))
        z = A.new_zeros
        return z(M0, K0), (z(M0) if want_colsum else None), (z(nv0, K0) if nv0 else None)
    if not all(_aligned_rows(t) for t in (A, B) + ((B_items,) if B_items is not None else ())):
        # the kernels read 16-byte row segments: zero-pad the columns of any operand whose rows
        # are not 16-byte aligned (e.g. the [B, B] logit gradient of a ragged InfoNCE batch);
        # the zero columns only add output rows / columns that are dropped here
        M0, K0 = A.size(1), B.size(1)
        out, cs, vout = gemm_tn(_pad_cols4(A), _pad_cols4(B), want_colsum, V,
                                _pad_cols4(B_items) if B_items is not None else None)
        return (out[:M0, :K0].contiguous(), cs[:M0].contiguous() if cs is not None else None,
                vout[:, :K0].contiguous() if vout is not None else None)
    N, M, K = A.size(0), A.size(1), B.size(1)
    nv = 0 if V is None else V.size(1)
    if B_items is None and M * K > 128 * 128 and gemm_tn_big_supported(M, K):
        # beyond one 128 x 128 tile (config 5: 1024 x 256 over 1.9M rows): the matrix-core TN
        # kernel (ppgat_gemm_tn_big); column sums and V^T B through the small kernels
        bb = (_const_colmax(B), K, 1.0) if b_const else None
        if want_colsum:  # colsum(A) from the same pass over A
            out, cs = gemm_tn_big(A, B, b_bound=bb, want_colsum=True)
        else:
            out, cs = gemm_tn_big(A, B, b_bound=bb), None
        vout = None
        if nv:  # V^T B by the small kernel, V padded to a multiple of 4 columns (16-byte rows)
            Vp = torch.zeros(N, (nv + 3) // 4 * 4, dtype=torch.float32, device=A.device)
            Vp[:, :nv] = V
            vout = gemm_tn(Vp, B)[0][:nv].contiguous()
        return out, cs, vout
    if V is not None:
        _require(V.is_cuda and V.dtype == torch.float32 and V.dim() == 2 and V.stride(1) == 1 and V.size(0) == N,
                 "gemm_tn: V must be fp32 [N, nv] with unit column stride")
    out = torch.empty(M, K, dtype=torch.float32, device=A.device)
    cs = torch.empty(M, dtype=torch.float32, device=A.device) if want_colsum else None
    vout = torch.empty(max(nv, 1), K, dtype=torch.float32, device=A.device) if nv else None
    lda = A.stride(0) if N > 1 else max(M + (-M) % 4, 4)
    ldb = B.stride(0) if split > 1 else max(K + (-K) % 4, 4)
    ldv = (V.stride(0) if N > 1 else nv) if nv else 0
    ldb1 = (B_items.stride(0) if B_items.size(0) > 1 else max(K + (-K) % 4, 4)) if B_items is not None else 0
    _launch.gemm_tn(A, lda, B, ldb, B_items, ldb1, V, ldv, out, cs, vout)
    return out, cs, vout


class _Linear(torch.autograd.Function):
    """y = x W^T + b on the matrix cores: the fused 128-column projection (ppgat_project) or
    the general GEMM (ppgat_gemm_nn, config 5's 256-wide layers; other widths zero-padded by
    ``mm_nn``); dx by ppgat_gemm_nn, dW (and db) through ppgat_gemm_tn (N = 10^5..10^7 rows
    split over the chip).  No vendor BLAS on any shape."""

    @staticmethod
    def forward(ctx, x, weight, bias, out_holder=None):
        # no gradient reached the output (the halo partition's locally computed halo item rows,
        # whose gradients are their owners' business): skip the backward instead of running it on
        # a materialised zero gradient (a zero fill, two column-max passes and a TN GEMM over the
        # 2.8M halo rows per step at world 8 on config 5)
        ctx.set_materialize_grads(False)
        x_const = not x.requires_grad  # (an input the step does not differentiate: the item features)
        x = x.contiguous()
        ctx.save_for_backward(x, weight)
        ctx.x_keep = x if x_const else None  # the object itself: its cached column bound is found by identity
        ctx.has_bias = bias is not None
        W = weight.detach().contiguous()
        b = bias.detach().contiguous() if bias is not None else None
        out = out_holder[0] if out_holder is not None else None  # (in a list: a buffer, not an autograd input)
        if project_supported(x.size(1), weight.size(0)):
            return project(x, W, b, out=out)
        elif gemm_nn_supported(x.size(0), x.size(1), weight.size(0), 1):
            return gemm_nn(x, W, 1, weight.size(0), bias=b, out=out)
        else:
            y = mm_nn(x, W, 1, weight.size(0), bias=b)
        return y if out is None else out.copy_(y)

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return None, None, None, None
        x, weight = ctx.saved_tensors
        g = g.contiguous()
        dx = None
        if ctx.needs_input_grad[0]:
            W = weight.detach().contiguous()
            if gemm_nn_supported(g.size(0), g.size(1), W.size(1), 0):
                dx = gemm_nn(g, W, 0, W.size(1))
            else:
                dx = mm_nn(g, W, 0, W.size(1))
        dW = db = None
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            xk = ctx.x_keep
            dW, db, _ = gemm_tn(g, xk if xk is not None else x, want_colsum=ctx.has_bias, b_const=xk is not None)
        return dx, dW, db if ctx.has_bias else None, None


def linear(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None,
           out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x W^T + b; with ``out`` (contiguous [rows, out_features]) written there and returned."""
    _require(x.is_cuda, "linear: ppgat runs on ROCm devices only; there is no CPU path")
    if x.dtype != torch.float32 or x.dim() != 2:
        raise NotImplementedError("ppgat linear: fp32 2-D input only")
    if out is not None:
        _require(out.is_cuda and out.dtype == torch.float32 and out.is_contiguous()
                 and out.shape == (x.size(0), weight.size(0)), "linear: out must be contiguous [rows, out_features]")
    return _Linear.apply(x, weight, bias, [out] if out is not None else None)


class _JoinRows(torch.autograd.Function):
    """cat([a, b]) of two row blocks that already lie back to back in one storage: the joined
    tensor is a new header on that storage (no copy); the gradient splits at the seam."""

    @staticmethod
    def forward(ctx, a, b):
        ctx.n = a.size(0)
        return a.new_empty(0).set_(a.untyped_storage(), a.storage_offset(), (a.size(0) + b.size(0), a.size(1)),
                                   (a.size(1), 1))

    @staticmethod
    def backward(ctx, g):
        return g[:ctx.n], g[ctx.n:]


def rows_adjacent(a: torch.Tensor, b: torch.Tensor) -> bool:
    """b's rows start where a's end, in one storage, both contiguous with the same width."""
    return (a.dim() == 2 and b.dim() == 2 and a.size(1) == b.size(1) and a.dtype == b.dtype and a.device == b.device
            and a.is_contiguous() and b.is_contiguous()
            and a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr()
            and b.storage_offset() == a.storage_offset() + a.numel())


def join_rows(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """torch.cat([a, b], 0), without the copy when the blocks are adjacent (model.node_table)."""
    return _JoinRows.apply(a, b) if rows_adjacent(a, b) else torch.cat([a, b], 0)


class _EmbeddingRows(torch.autograd.Function):
    """weight.index_select(0, idx) whose gradient for ``weight`` is row-sparse: a COO tensor with
    ``idx`` as its one sparse dimension and the incoming rows as its values -- no zero-filled
    [n_rows, d] gradient.  Not flagged coalesced: repeated ids in ``idx`` stay separate entries
    (they add on coalesce(), as index_select's backward adds them)."""

    @staticmethod
    def forward(ctx, weight, idx):
        ctx.save_for_backward(idx)
        ctx.shape = weight.shape
        return weight.index_select(0, idx)

    @staticmethod
    def backward(ctx, g):
        (idx,) = ctx.saved_tensors
        return torch.sparse_coo_tensor(idx[None], g.contiguous(), ctx.shape), None


def embedding_rows(weight: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """``weight.index_select(0, idx)`` for a 2-D table and int64 ``idx``, with a row-sparse gradient
    (``optim.Adam`` takes it: the lazy row step).  Pure torch on any device; launches no kernel."""
    _require(weight.dim() == 2 and idx.dim() == 1 and idx.dtype == torch.int64,
             "embedding_rows: weight [n, d] and int64 idx [k] expected")
    return _EmbeddingRows.apply(weight, idx)


# ---------------------------------------------------------------------------
# general fp32 matrix-core GEMMs (include/ppgat.h ppgat_gemm_nn / ppgat_gemm_tn_big)
# ---------------------------------------------------------------------------
def gemm_nn_supported(m: int, k: int, n: int, b_layout: int) -> bool:
    return _launch.gemm_nn_supported(m, k, n, b_layout)


def gemm_nn(x: torch.Tensor, B: torch.Tensor, b_layout: int, n: int, alpha: float = 1.0,
            bias: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
            rank: Optional[tuple] = None) -> torch.Tensor:
    """alpha x B (+ bias): B [K, n] row-major (b_layout 0) or [n, K] (b_layout 1: x B^T).
    rank=(S [M, nv], A [nv, n]): + S A as well (ppgat_gemm_nn_rank; in the GEMM's epilogue on
    the large-M fp16 path, the same bits as gemm_nn followed by rank_update_)."""
    _check_rows("x", x, torch.float32)
    _check_rows("B", B, torch.float32, x.device)
    M, K = x.shape
    y = out if out is not None else torch.empty(M, n, dtype=torch.float32, device=x.device)
    ldx, ldy = (x.stride(0) if M > 1 else K), (y.stride(0) if M > 1 else n)
    lds = 0
    if rank is not None:
        S, A = rank
        nv = S.size(1)
        _require(S.dim() == 2 and S.size(0) == M and S.stride(1) == 1 and A.is_contiguous() and A.shape == (nv, n),
                 "gemm_nn: rank=(S [M, nv], A [nv, n] contiguous)")
        lds = S.stride(0) if M > 1 else nv
    _launch.gemm_nn(x, ldx, B, b_layout, n, alpha, bias, y, ldy, rank, lds)
    return y


def _aligned_rows(t: torch.Tensor) -> bool:
    return t.dim() == 2 and t.stride(1) == 1 and (t.size(0) <= 1 or t.stride(0) % 4 == 0) and t.data_ptr() % 16 == 0


def _pad_cols4(t: torch.Tensor) -> torch.Tensor:
    """``t`` itself when its rows are 16-byte aligned, else a copy with its columns zero-padded
    to a multiple of 4."""
    if _aligned_rows(t):
        return t
    n, c = t.shape
    tp = torch.zeros(n, c + (-c) % 4, dtype=t.dtype, device=t.device)
    tp[:, :c] = t
    return tp


def mm_nn(x: torch.Tensor, B: torch.Tensor, b_layout: int, n: int, alpha: float = 1.0,
          bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """alpha x B (+ bias) for ANY shape on ppgat_gemm_nn: the reduction width is zero-padded to
    a multiple of 32 and the output width to a multiple of 128 where the kernel needs it (the
    padding adds exact zeros, so the result is the unpadded product).  B [K, n] (b_layout 0)
    or [n, K] (b_layout 1, i.e. x B^T).  No vendor BLAS on any shape."""
    _require(x.is_cuda and x.dtype == torch.float32 and x.dim() == 2, "mm_nn: x must be a 2-D fp32 ROCm tensor")
    M, K = x.shape
    if M == 0:
        return torch.zeros(0, n, dtype=torch.float32, device=x.device)
    Kp, Np = -(-max(K, 1) // 32) * 32, -(-max(n, 1) // 128) * 128
    if Kp != K or not _aligned_rows(x):
        xp = torch.zeros(M, Kp, dtype=torch.float32, device=x.device)
        xp[:, :K] = x
        x = xp
    B = B.detach()
    if Kp != K or Np != n or not _aligned_rows(B):
        Bp = torch.zeros((Kp, Np) if b_layout == 0 else (Np, Kp), dtype=torch.float32, device=x.device)
        if b_layout == 0:
            Bp[:K, :n] = B
        else:
            Bp[:n, :K] = B
        B = Bp
    if bias is not None and Np != n:
        bias = torch.cat([bias.detach().reshape(-1), bias.new_zeros(Np - n)])
    y = gemm_nn(x, B, b_layout, Np, alpha=alpha, bias=bias.detach().contiguous() if bias is not None else None)
    return y if Np == n else y[:, :n].contiguous()


def att_proj(W: torch.Tensor, a_s: torch.Tensor, a_d: torch.Tensor, heads: int, channels: int) -> torch.Tensor:
    """[2H, K] = [W_h^T att_src[h]; W_h^T att_dst[h]] (ppgat_att_proj)."""
    A = torch.empty(2 * heads, W.size(1), dtype=torch.float32, device=W.device)
    _launch.att_proj(W, a_s, a_d, heads, channels, A)
    return A


def rank_update_(dx: torch.Tensor, S: torch.Tensor, A: torch.Tensor) -> torch.Tensor:
    """dx += S A in place (ppgat_rows_rank_update; S [n, nv] with nv <= 16, A [nv, K])."""
    n, K = dx.shape
    nv = S.size(1)
    _require(K % 4 == 0 and _aligned_rows(dx) and A.is_contiguous() and S.stride(1) == 1 and nv <= 16,
             "rank_update_: dx rows 16-byte aligned with K % 4 == 0, nv <= 16")
    _launch.rows_rank_update(S, S.stride(0) if n > 1 else nv, A, dx, dx.stride(0) if n > 1 else K)
    return dx


def gemm_tn_big_supported(ma: int, nb: int) -> bool:
    return ma % 128 == 0 and nb % 128 == 0 and ma >= 128 and nb >= 128


def colmax_abs(X: torch.Tensor, src_ptr: Optional[torch.Tensor] = None) -> torch.Tensor:
    """IEEE bits (int32 view) of max_i |X[i, c]| per column (ppgat_colmax_abs; deterministic);
    with ``src_ptr`` (CSC pointers [n + 1]) over the rows that are an edge's source only
    (ppgat_colmax_abs_sources)."""
    _check_rows("X", X, torch.float32)
    n, c = X.shape
    out = torch.empty(c, dtype=torch.int32, device=X.device)
    ld = X.stride(0) if n > 1 else c
    if src_ptr is not None:
        _check_dev("src_ptr", src_ptr, torch.int32, X.device)
        _require(src_ptr.numel() == n + 1, "colmax_abs: src_ptr must hold n + 1 CSC pointers")
    _launch.colmax_abs(X, ld, out, src_ptr)
    return out


def gemm_tn_big(A: torch.Tensor, B: torch.Tensor, b_bound=None, a_bits=None, want_colsum: bool = False):
    """A [M, ma]^T B [M, nb] on the matrix cores (ppgat_gemm_tn_big), deterministic.  ``b_bound``
    = (bits [period] from colmax_abs, period, scale >= 1): an upper bound of |B| per column
    (column j: bits[j % period] * scale) that replaces the fp16 kernel's column-max pass over B
    (ppgat_gemm_tn_big_bounded).  ``a_bits`` [ma]: a bound of |A| over the rows whose B row is not
    zero (ppgat_gemm_tn_big_bounds: the other rows are clamped) in place of A's pass.
    ``want_colsum``: returns (out, colsum(A)), the column sums from the same pass over A
    (ppgat_gemm_tn_big_colsum)."""
    _check_rows("A", A, torch.float32)
    _check_rows("B", B, torch.float32, A.device)
    M, ma = A.shape
    nb = B.size(1)
    ws, nbytes = _launch.gemm_tn_big_workspace(M, ma, nb, A.device)
    out = torch.empty(ma, nb, dtype=torch.float32, device=A.device)
    lda, ldb = A.stride(0) if M > 1 else ma, B.stride(0) if M > 1 else nb
    if a_bits is not None:
        _require(a_bits.dtype == torch.int32 and a_bits.numel() == ma and a_bits.device == A.device,
                 "gemm_tn_big: a_bits must be int32 [ma] on A's device")
    if b_bound is not None and (b_bound[0] is not None if want_colsum else a_bits is None):
        bits, period, _ = b_bound  # (with a_bits and no column sums the bound is taken as given)
        _require(bits.dtype == torch.int32 and bits.numel() == period and bits.device == A.device,
                 "gemm_tn_big: b_bound bits must be int32 [period] on A's device")
    cs = torch.empty(ma, dtype=torch.float32, device=A.device) if want_colsum else None
    _launch.gemm_tn_big(A, lda, B, ldb, out, ws, nbytes, b_bound, a_bits, cs)
    return (out, cs) if want_colsum else out


def colsum(Y: torch.Tensor) -> torch.Tensor:
    """Column sums of Y [n, c] (ppgat_colsum over 128- or 256-column slabs; torch for widths not a multiple of 128)."""
    _check_rows("Y", Y, torch.float32)
    n, c = Y.shape
    if c not in (128, 256) and c % 256 == 0:  # wider: 256-column slabs
        return torch.cat([colsum(Y[:, s:s + 256]) for s in range(0, c, 256)])
    if c not in (128, 256) and c % 128 == 0:
        return torch.cat([colsum(Y[:, s:s + 128]) for s in range(0, c, 128)])
    if c not in (128, 256):
        return Y.sum(0)
    ws, nbytes = _launch.colsum_workspace(n, c, Y.device)
    out = torch.empty(c, dtype=torch.float32, device=Y.device)
    _launch.colsum(Y, Y.stride(0) if n > 1 else c, out, ws, nbytes)
    return out
