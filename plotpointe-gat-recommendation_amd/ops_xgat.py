"""The aggregate-then-transform multi-head layer behind hip_ops (include/ppgat.h ppgat_xgat_*): its
edge-list views and phases, forward, the three backward formulations and the choice between them,
the weight gradients, and the ``GATLayerX`` autograd function.
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Callable, Optional

import torch

from . import _launch
from .ops_gemm import colmax_abs, colsum, gemm_nn, gemm_tn, gemm_tn_big
from .ops_graph import CSRGraph, Schedule, _csr2csc, _require, _tap_kinks, seed_buffer


# ---------------------------------------------------------------------------
# multi-head layer, aggregate-then-transform (include/ppgat.h ppgat_xgat_*)
# ---------------------------------------------------------------------------
@dataclass
class XViews:
    """The edge lists the aggregate-then-transform layer runs on: CSR over the n_dst
    destination rows (forward, destination sums) and CSC over the n_src source rows
    (backward edge pass); source ids index x rows [0, n_src)."""
    n_dst: int
    n_src: int
    n_edges: int
    col: torch.Tensor
    csr_eid: torch.Tensor
    fwd_sched: Schedule
    row: torch.Tensor
    csc_eid: torch.Tensor
    dz_slot: torch.Tensor
    bwd_sched: Schedule
    bwd_sched_own: Optional[Schedule] = None   # sources [0, n_dst) (halo partition)
    bwd_sched_halo: Optional[Schedule] = None  # sources [n_dst, n_src), rows relative to n_dst
    # dz_slot None: dz in CSC order, summed per destination through csr2csc
    csr2csc: Optional[torch.Tensor] = None
    rowptr: Optional[torch.Tensor] = None  # CSR row pointers over the destinations (KINK_TAP only)
    colptr: Optional[torch.Tensor] = None  # CSC pointers over the sources [n_src + 1] (agg's column bound)

    @staticmethod
    def of_graph(g: "CSRGraph") -> "XViews":
        return XViews(g.n_nodes, g.n_nodes, g.n_edges, g.col, g.csr_eid, g.fwd_sched, g.row, g.csc_eid, None,
                      g.bwd_sched, csr2csc=_csr2csc(g), rowptr=g.rowptr, colptr=g.colptr)


def xgat_supported(in_channels: int, heads: int, channels: int) -> bool:
    return _launch.xgat_supported(in_channels, heads, channels)


@dataclass
class XPhase:
    """One step of a phased aggregate-then-transform forward (dist._HaloLayerX): the destination
    rows [d0, d1) with their schedule (rows relative to d0), the source row ranges whose node
    scores this phase computes first (rows outside the own destination rows, e.g. halo rows that
    have just arrived), ``before()`` (e.g. make the stream wait for those rows' exchange) and
    ``after(out)`` (e.g. start sending the phase's output rows to the peers)."""
    d0: int
    d1: int
    sched: Schedule
    src_ranges: tuple = ()
    before: Optional[Callable] = None
    after: Optional[Callable] = None


def xgat_att_proj(weight, att_src, att_dst, heads: int, C: int) -> torch.Tensor:
    """A [2, H, K]: A_v[h] = W_h^T att_v[h] (ppgat_xgat_weights) -- the node scores are x . A."""
    W = weight.detach().contiguous()
    a_s = att_src.detach().reshape(heads, C).contiguous()
    a_d = att_dst.detach().reshape(heads, C).contiguous()
    A = torch.empty(2, heads, W.size(1), dtype=torch.float32, device=W.device)
    _launch.xgat_weights(W, a_s, a_d, heads, C, A=A)
    return A


def xgat_scores_rows(x_rows, A, s_src, s_dst=None):
    """s_src (and, given, s_dst) [n, H] of the rows x_rows [n, K] (row stride x_rows.stride(0))
    under A [2, H, K] (ppgat_xgat_scores; per row the same arithmetic whatever the launch)."""
    if x_rows.size(0):
        _launch.xgat_scores(x_rows, 0, x_rows.size(0), A, s_src, s_dst)


def xgat_forward(x, weight, att_src, att_dst, bias, v: "XViews", heads: int, C: int, slope: float, p: float,
                 seed: int, phases: Optional[list] = None, out: Optional[torch.Tensor] = None, scores=None,
                 keep_agg: Optional[bool] = None):
    """Forward of the aggregate-then-transform layer; returns (out [n_dst, C], saved state).

    ``phases`` (a list of XPhase partitioning [0, n_dst) in order): the node scores of the
    destination rows first, then per phase its sources' scores, the edge pass over its
    destination rows and their rows of the output GEMM.  Per destination the result is the
    same as the one-phase forward (same per-row kernels and order): bitwise equal.  ``out``: a
    contiguous [n_dst, C] destination (the next halo layer's own rows: no copy there).
    ``scores`` = (s_src [n_src, H], s_dst [>= n_dst, H]): the node scores, already computed
    (the halo partition: the owners computed them with the rows and sent them along, ready by
    each phase's ``before``) -- no score pass here.  ``keep_agg``: keep the aggregates for the
    backward (None: _xgat_keep_agg decides; the halo partition's backward needs them)."""
    x = x.contiguous()
    dev = x.device
    K = x.size(1)
    H = heads
    _require(x.size(0) == v.n_src, f"x has {x.size(0)} rows, the edge lists {v.n_src} sources")
    W = weight.detach().contiguous()
    a_s = att_src.detach().reshape(H, C).contiguous()
    a_d = att_dst.detach().reshape(H, C).contiguous()
    b = bias.detach().contiguous() if bias is not None else None
    A = torch.empty(2, H, K, dtype=torch.float32, device=dev)
    Wt = torch.empty(H * K, C, dtype=torch.float32, device=dev)
    _launch.xgat_weights(W, a_s, a_d, H, C, A=A, Wt=Wt)
    if phases is None:
        phases = [XPhase(0, v.n_dst, v.fwd_sched, ((v.n_dst, v.n_src),) if v.n_src > v.n_dst else ())]
    if scores is not None:
        s_src, s_dst = scores
        _require(s_src.shape == (v.n_src, H) and s_dst.size(0) >= max(v.n_dst, 1) and s_dst.size(1) == H
                 and s_src.is_contiguous() and s_dst.is_contiguous(), "xgat_forward: scores must be [n_src, H], [n_dst, H]")
    else:
        s_src = torch.empty(v.n_src, H, dtype=torch.float32, device=dev)
        s_dst = torch.empty(max(v.n_dst, 1), H, dtype=torch.float32, device=dev)
        # the destination rows' scores (s_src and s_dst), then each phase's other sources
        _launch.xgat_scores(x, 0, v.n_dst, A, s_src, s_dst)
    agg = torch.empty(v.n_dst, H, K, dtype=torch.float32, device=dev)
    m = torch.empty(v.n_dst, H, dtype=torch.float32, device=dev)
    inv_l = torch.empty(v.n_dst, H, dtype=torch.float32, device=dev)
    if out is None:
        out = torch.empty(v.n_dst, C, dtype=torch.float32, device=dev)
    _require(out.shape == (v.n_dst, C) and out.is_contiguous(), "xgat_forward: out must be contiguous [n_dst, C]")
    seed_buf = seed_buffer(p, dev)
    E = v.n_edges
    # column maxima of |x| over the rows the edge pass gathers (every source): the weight
    # gradient's bound of |agg| (_xgat_weight_grads), with no pass of its own over x
    xbits = torch.zeros(K, dtype=torch.int32, device=dev)
    for ph in phases:
        if ph.before is not None:
            ph.before()
        for r0, r1 in (ph.src_ranges if scores is None else ()):
            if r1 > r0:
                _launch.xgat_scores(x, r0, r1 - r0, A, s_src)
        nd = ph.d1 - ph.d0
        _launch.xgat_fwd_colmax(ph.sched, v, ph.d0, nd, x, s_src, s_dst, slope, p, seed, seed_buf, agg, m, inv_l,
                                xbits)
        if nd > 0:
            gemm_nn(agg[ph.d0:ph.d1].view(nd, H * K), Wt, 0, C, alpha=1.0 / H, bias=b, out=out[ph.d0:ph.d1])
        if ph.after is not None:
            ph.after(out)
    _tap_kinks(v.rowptr, v.col, v.csr_eid, s_src, s_dst, H)
    if not (keep_agg if keep_agg is not None else _xgat_keep_agg(v.n_dst, v.n_src, H, K, C, dev, E)):
        agg = None  # the backward's weight gradient comes from acc^T x (_xgat_weight_grads)
    saved = dict(x=x, W=W, a_s=a_s, a_d=a_d, A=A, s_src=s_src, s_dst=s_dst, agg=agg, m=m, inv_l=inv_l,
                 seed_buf=seed_buf, v=v, xbits=xbits, meta=(H, C, K, slope, p, seed, bias is not None))
    return out, saved


def _xgat_keep_agg(n_dst: int, n_src: int, H: int, K: int, C: int, dev, n_edges: int = 0) -> bool:
    """Whether the forward's aggregates agg [n_dst, H, C_in] stay alive for the backward's weight
    gradient G = g^T agg.  The same G is acc^T x (permuted): G[c, (h, k)] = sum_i g_i[c] agg^h_i[k]
    = sum_i sum_j beta^h_ij g_i[c] x_j[k] = sum_j acc^h_j[c] x_j[k], and the default backward
    builds acc [n_src, H, C] anyway -- so agg is only worth keeping while memory is not short: the
    acc^T x form costs an exact column-max pass over acc (4 H C bytes per source) instead of one
    over g (4 C per destination).  PPGAT_XGAT_AGG=keep / free forces a form; by default agg is
    dropped when four tensors of its size -- two layers' agg, the backward's hs and acc -- would
    take more than half of the device's memory: the whole 200M-edge graph on one GPU (61 GB each;
    tools/mem_probe.py: the agg-free step's peak is 239 GB there), not its 1/8 share (7.7 GB)."""
    mode = os.environ.get("PPGAT_XGAT_AGG", "auto")
    if mode == "keep":
        return True
    if _xgat_gather_mode(C, H, n_src, n_dst, n_edges, K) != "gd":  # the backward's own choice, same inputs
        return True  # the gt / g passes read agg in their prologue
    if mode == "free":
        return False
    total = torch.cuda.get_device_properties(dev).total_memory
    return 4 * (4.0 * H * max(K, C) * max(n_dst, n_src)) <= 0.5 * total


def xgat_backward(saved: dict, g: torch.Tensor, want_bias_grad: bool, halo_hook=None):
    """Backward of the aggregate-then-transform layer -> (dx [n_src, C_in], dW, datt_src [H, C],
    datt_dst [H, C], dbias).  With ``halo_hook`` and a view split into own sources [0, n_own)
    and halo sources (XViews.bwd_sched_own / bwd_sched_halo), the halo rows' input gradients
    are finished first and handed to halo_hook(dx_halo) -- which starts returning them to
    their owners -- before the own rows' edge pass and the weight-gradient GEMMs run."""
    x, W, a_s, a_d, A = saved["x"], saved["W"], saved["a_s"], saved["a_d"], saved["A"]
    s_src, s_dst, agg, m, inv_l, v = saved["s_src"], saved["s_dst"], saved["agg"], saved["m"], saved["inv_l"], saved["v"]
    H, C, K, slope, p, seed, has_bias = saved["meta"]
    dev = x.device
    g = g.contiguous()
    E = v.n_edges
    S = torch.zeros(v.n_src, 2 * H, dtype=torch.float32, device=dev)
    dz = torch.empty(max(E, 1) * H, dtype=torch.float32, device=dev)
    nstate = torch.empty(max(v.n_dst, 1), H, 4, dtype=torch.float32, device=dev)
    mode = _xgat_gather_mode(C, H, v.n_src, v.n_dst, E, K)
    if mode == "gd":
        return _xgat_backward_deferred_d(saved, g, S, dz, nstate, want_bias_grad, halo_hook)
    Wg = torch.empty(C, H * K, dtype=torch.float32, device=dev)
    _launch.xgat_weights(W, None, None, H, C, Wg=Wg)
    gt = gemm_nn(g, Wg, 0, H * K)
    _launch.xgat_bwd_prologue(gt, agg, s_dst, m, inv_l, v.n_dst, K, H, nstate)
    if mode == "g":
        # gather g_i per edge (C floats) instead of gt_i (H * C_in): hs = x W^T / H per source,
        # the per-head message gradient acc [n_src, H * C], then dx = acc W / H + S A_att with the
        # attention terms in the GEMM's epilogue
        hs = gemm_nn(x, W, 1, H * C, alpha=1.0 / H)
        acc = torch.empty(v.n_src, H * C, dtype=torch.float32, device=dev)
        dx = torch.empty(v.n_src, K, dtype=torch.float32, device=dev)
        A2 = A.view(2 * H, K)
        gargs = (hs, s_src, nstate, g, acc, S, dz, H, C, slope, p, seed, saved["seed_buf"])
        n0 = v.n_dst
        if halo_hook is not None and v.bwd_sched_halo is not None:
            # the halo sources first: their rows of dx (no destination terms) go back to their
            # owners while the own sources' edge pass runs
            _launch.xgat_bwd_edges_g(v.bwd_sched_halo, v, n0, *gargs)
            if v.n_src > n0:
                gemm_nn(acc[n0:], W, 0, K, alpha=1.0 / H, out=dx[n0:], rank=(S[n0:, :H], A2[:H]))
            halo_hook(dx[n0:])
            _launch.xgat_bwd_edges_g(v.bwd_sched_own, v, 0, *gargs)
            _xgat_dst_sum(v, dz, S[:, H:], H)
            gemm_nn(acc[:n0], W, 0, K, alpha=1.0 / H, out=dx[:n0], rank=(S[:n0], A2))
        else:
            _launch.xgat_bwd_edges_g(v.bwd_sched, v, 0, *gargs)
            _xgat_dst_sum(v, dz, S[:, H:], H)
            gemm_nn(acc, W, 0, K, alpha=1.0 / H, out=dx, rank=(S, A2))  # + sum_h ds_src^h A_src^h + ds_dst^h A_dst^h
            if halo_hook is not None:
                halo_hook(dx[n0:])
        del hs, acc
        return _xgat_weight_grads(None, saved, g, S, dx, want_bias_grad, None)
    dx = torch.empty(v.n_src, K, dtype=torch.float32, device=dev)
    args = (x, s_src, nstate, gt, A, S, dz, dx, H, slope, p, seed, saved["seed_buf"])
    if halo_hook is not None and v.bwd_sched_halo is not None:
        _launch.xgat_bwd_edges(v.bwd_sched_halo, v, v.n_dst, *args)
        halo_hook(dx[v.n_dst:])
        _launch.xgat_bwd_edges(v.bwd_sched_own, v, 0, *args)
    else:
        _launch.xgat_bwd_edges(v.bwd_sched, v, 0, *args)
        if halo_hook is not None:
            halo_hook(dx[v.n_dst:])
    _xgat_dst_sum(v, dz, S[:, H:], H)
    _launch.xgat_bwd_epilogue(S, A, v.n_dst, H, dx)
    return _xgat_weight_grads(None, saved, g, S, dx, want_bias_grad, None)


def _xgat_bytes(mode: str, n_src: int, n_dst: int, n_edges: int, C: int, H: int, K: int) -> float:
    """HBM bytes of one multi-head layer backward per formulation: per edge the
    gathered row (g_i: 4C, or gt_i: 4HK) and the per-edge terms; per source the hs and acc rows
    of the g-gathering passes (written, read back: 4 x 4HC) and x / dx (2 x 4K), or x / dx only;
    per destination the gt GEMM and its prologue (3 x 4HK) in the gt-gathering pass."""
    if mode == "gt":
        return n_edges * (4 + 24 * H + 4 * H * K) + n_dst * 12 * H * K + n_src * 8 * K
    return n_edges * (4 + 24 * H + 4 * C) + n_src * (8 * K + 16 * H * C)


def _xgat_gather_mode(C: int, H: int, n_src: Optional[int] = None, n_dst: Optional[int] = None,
                      n_edges: Optional[int] = None, K: Optional[int] = None) -> str:
    """Which multi-head backward runs (read per call): "gd" gathers g_i per edge and defers D (no
    gt GEMM: ppgat_xgat_bwd_edges_gd + D by a destination sum + ppgat_xgat_bwd_dz); "g" gathers
    g_i with D from the gt GEMM's prologue (ppgat_xgat_bwd_edges_g); "gt" gathers gt_i
    (ppgat_xgat_bwd_edges, round 2's pass).  DESIGN.md §4.2.  PPGAT_XGAT_GATHER picks one; by
    default "gd", except where the layer's sources far outnumber its destinations (the halo
    partition at 8 ranks: 11M local rows for 1.9M own) and the g-gathering passes' per-source
    GEMMs would move more bytes than gathering gt_i per edge (_xgat_bytes)."""
    if C != 256 or H not in (2, 4):
        return "gt"
    mode = os.environ.get("PPGAT_XGAT_GATHER")
    if mode in ("g", "gt", "gd"):
        return mode
    if n_src is not None and n_src > n_dst and \
            _xgat_bytes("gt", n_src, n_dst, n_edges, C, H, K) < _xgat_bytes("gd", n_src, n_dst, n_edges, C, H, K):
        return "gt"
    return "gd"


def _xgat_backward_deferred_d(saved: dict, g, S, dz, nstate, want_bias_grad: bool, halo_hook):
    """The default multi-head backward: D^h_i = sum_j beta dalpha from the edge
    pass itself instead of gt^h_i . agg^h_i, so neither gt = g W_grad nor its prologue runs."""
    x, W, A = saved["x"], saved["W"], saved["A"]
    s_src, s_dst, m, inv_l, v = saved["s_src"], saved["s_dst"], saved["m"], saved["inv_l"], saved["v"]
    H, C, K, slope, p, seed, has_bias = saved["meta"]
    dev = x.device
    E = v.n_edges
    n0 = v.n_dst
    seed_buf = saved["seed_buf"]
    _launch.xgat_nstate(s_dst, m, inv_l, None, n0, H, nstate)
    hs = gemm_nn(x, W, 1, H * C, alpha=1.0 / H)
    acc = torch.empty(v.n_src, H * C, dtype=torch.float32, device=dev)
    pdal = torch.empty(max(E, 1) * H, dtype=torch.float32, device=dev)
    gbits = torch.zeros(C, dtype=torch.int32, device=dev)  # |g| over the gathered rows: the G product's A bound
    split = halo_hook is not None and v.bwd_sched_halo is not None
    scheds = [(v.bwd_sched_halo, n0), (v.bwd_sched_own, 0)] if split else [(v.bwd_sched, 0)]
    for sched, base in scheds:  # dalpha (into dz) and beta dalpha per edge, acc per source
        _launch.xgat_bwd_edges_gd_colmax(sched, v, base, hs, s_src, nstate, g, acc, dz, pdal, gbits, H, C, slope, p,
                                         seed, seed_buf)
    del hs
    D = torch.empty(max(n0, 1), H, dtype=torch.float32, device=dev)
    _xgat_dst_sum(v, pdal, D, H)  # D_i = sum_j beta dalpha
    del pdal
    _launch.xgat_nstate(s_dst, m, inv_l, D, n0, H, nstate)
    dza = (s_src, nstate, dz, S, H, slope, p, seed, seed_buf)  # the dz pass: dz in place over dalpha, ds_src into S
    dx = torch.empty(v.n_src, K, dtype=torch.float32, device=dev)
    A2 = A.view(2 * H, K)
    if split:
        # the halo sources first: their rows of dx (no destination terms) go back to their owners
        # while the own sources' dz pass, the destination sums and the GEMMs run
        _launch.xgat_bwd_dz(v.bwd_sched_halo, v, n0, *dza)
        if v.n_src > n0:
            gemm_nn(acc[n0:], W, 0, K, alpha=1.0 / H, out=dx[n0:], rank=(S[n0:, :H], A2[:H]))
        halo_hook(dx[n0:])
        _launch.xgat_bwd_dz(v.bwd_sched_own, v, 0, *dza)
        _xgat_dst_sum(v, dz, S[:, H:], H)
        gemm_nn(acc[:n0], W, 0, K, alpha=1.0 / H, out=dx[:n0], rank=(S[:n0], A2))
    else:
        _launch.xgat_bwd_dz(v.bwd_sched, v, 0, *dza)
        _xgat_dst_sum(v, dz, S[:, H:], H)
        gemm_nn(acc, W, 0, K, alpha=1.0 / H, out=dx, rank=(S, A2))
        if halo_hook is not None:
            halo_hook(dx[n0:])
    if saved["agg"] is not None:
        del acc
        return _xgat_weight_grads(None, saved, g, S, dx, want_bias_grad, None, gbits=gbits)
    return _xgat_weight_grads(None, saved, g, S, dx, want_bias_grad, None, acc=acc)


def _xgat_dst_sum(v: "XViews", dz, out, H: int):
    """Per-destination sums of dz (per edge and head) into ``out`` [n_dst, H], fixed order: ds_dst
    into the column view S[:, H:], or a table of its own."""
    # a thread per short destination (k_dst_sum_vh_short) pays off on the halo tables' rows of
    # ~2 edges (4 x 1.48 -> 4 x 0.71 ms per step at the world-8 probe); at the share's ~13 it
    # measured slower than 16 lanes per item (0.70 vs 0.54 ms per call, profiles/r06/
    # x13_cfg5_kernel_stats.csv against r05/w43): all items on the 16-lane kernel (same bits)
    _launch.bwd_dst_sum(v.fwd_sched, v.n_dst, v.n_edges, H, dz, v.csr2csc, out, csc=v.dz_slot is None,
                        all_long=v.n_edges > 6 * max(v.n_dst, 1))


def _xgat_weight_grads(lib, saved: dict, g, S, dx, want_bias_grad: bool, st, x_rows=None, xbits=None, acc=None,
                       gbits=None):
    """dW, datt, dbias from G = g^T agg and GV = S^T x (``x_rows``: the rows of x that S covers,
    default all of the layer's source rows; ``xbits``: a column bound of the source rows of x,
    colmax_abs bits -- default the forward's, gathered by its edge pass; ``gbits``: a column bound
    of |g| over the destinations with an in-edge, from the backward's edge pass).  Without a
    saved agg (_xgat_keep_agg): G from ``acc`` [n_src, H * C] as (acc^T x) permuted.
    ``lib`` and ``st`` are not used (the launches find the library and the stream themselves);
    they keep their places for the tools and tests that wrap this function by position."""
    x, W, a_s, a_d, agg, v = saved["x"], saved["W"], saved["a_s"], saved["a_d"], saved["agg"], saved["v"]
    H, C, K, slope, p, seed, has_bias = saved["meta"]
    dev = x.device
    GV = gemm_tn(S, x if x_rows is None else x_rows)[0]
    if agg is None:
        _require(acc is not None and x_rows is None, "xgat weight gradients: no agg saved and no acc given")
        # G'[(h, c), k] = sum_j acc^h_j[c] x_j[k]; B = x with its exact column maxima over ALL rows
        # (a row without out-edges has acc_j = 0 but its x_j still meets the fp16 split)
        Gp = gemm_tn_big(acc, x, b_bound=(colmax_abs(x), K, 1.0))
        G = Gp.view(H, C, K).permute(1, 0, 2).reshape(C, H * K).contiguous()
        del Gp
        return (dx,) + _xgat_weight_grads_from_G(saved, G, GV, g, want_bias_grad)
    # |agg^h_i[k]| = |sum_j beta_ij x_j[k]| <= max_j |x_j[k]| / (1 - p) over i's sources j (the
    # attention weights sum to 1, the kept ones scaled by 1 / (1 - p)): a column bound of agg from
    # the column maxima of the SOURCE rows of x (1 KB per row; a row with no out-edge -- however
    # large -- never enters an aggregate and must not loosen the bound: the fp16 split's error is
    # relative to it) instead of a pass over agg (4 KB per row); 2^-10 margin for fp32 rounding
    if xbits is None:
        xbits = saved.get("xbits")
    xbound = (colmax_abs(x, v.colptr) if xbits is None else xbits, K,
              (1.0 / (1.0 - p) if p > 0 else 1.0) * (1.0 + 2.0 ** -10))
    # (rows of g without an in-edge are outside gbits; their agg rows are zero: clamped, they add 0)
    if saved["meta"][6] and want_bias_grad:  # dbias = colsum(g) from the same pass over g
        G, gsum = gemm_tn_big(g, agg.view(v.n_dst, H * K), b_bound=xbound, a_bits=gbits, want_colsum=True)
    else:
        G, gsum = gemm_tn_big(g, agg.view(v.n_dst, H * K), b_bound=xbound, a_bits=gbits), None
    dW, datt_src, datt_dst, dbias = _xgat_weight_grads_from_G(saved, G, GV, g, want_bias_grad, gsum)
    return dx, dW, datt_src, datt_dst, dbias


def _xgat_weight_grads_from_G(saved: dict, G, GV, g, want_bias_grad: bool, gsum=None):
    W, a_s, a_d = saved["W"], saved["a_s"], saved["a_d"]
    H, C, K, slope, p, seed, has_bias = saved["meta"]
    dev = W.device
    dW = torch.empty_like(W)
    datt_src = torch.empty(H, C, dtype=torch.float32, device=dev)
    datt_dst = torch.empty(H, C, dtype=torch.float32, device=dev)
    _launch.xgat_weight_grads(G, GV, W, a_s, a_d, H, C, dW, datt_src, datt_dst)
    dbias = (gsum if gsum is not None else colsum(g)) if (has_bias and want_bias_grad) else None
    return dW, datt_src, datt_dst, dbias


class GATLayerX(torch.autograd.Function):
    """x [n_src, C_in] -> out [n_dst, C]: GATConv with H heads in the aggregate-then-transform
    form (include/ppgat.h ppgat_xgat_*): the edge pass gathers x_j once per edge for all heads,
    the per-head aggregates are transformed by one matrix-core GEMM; backward gt = g W / H
    (GEMM), one edge pass by source, dW = g^T agg (TN GEMM) + attention terms."""

    @staticmethod
    def forward(ctx, x, weight, att_src, att_dst, bias, v: "XViews", heads: int, C: int, slope: float, p: float,
                seed: int):
        out, ctx.saved = xgat_forward(x, weight, att_src, att_dst, bias, v, heads, C, slope, p, seed)
        ctx.att_shapes = (att_src.shape, att_dst.shape)
        return out

    @staticmethod
    def backward(ctx, g):
        dx, dW, datt_src, datt_dst, dbias = xgat_backward(ctx.saved, g, ctx.needs_input_grad[4])
        ctx.saved = None
        return (dx, dW, datt_src.view(ctx.att_shapes[0]), datt_dst.view(ctx.att_shapes[1]), dbias,
                None, None, None, None, None, None)


def gat_layer_x(x, weight, att_src, att_dst, bias, views: XViews, heads: int, channels: int, slope: float,
                dropout_p: float = 0.0, seed: int = 0, edge_v=None, edge_attr=None):
    if edge_v is not None or edge_attr is not None:
        raise NotImplementedError("gat_layer_x: edge features on the aggregate-then-transform layer are not "
                                  "implemented")
    _require(x.is_cuda, "gat_layer_x: ppgat runs on ROCm devices only; there is no CPU path")
    return GATLayerX.apply(x, weight, att_src, att_dst, bias, views, heads, channels, float(slope), float(dropout_p),
                           int(seed))
