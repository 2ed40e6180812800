"""The aggregate-then-transform layer's float64 reference (tests/_xgat_ref.py) without a GPU: its
explicit formulas and intermediates anchored to autograd and to the pinned restatement
(oracle.gat_oracle.pyg_gat_conv), the degree ladder of its graph, the LeakyReLU-kink condition the
GPU parity cases rely on (with the input seeds it settles), the exactness of the sharp scores, and
what the row-wise figures see that a whole-tensor maximum does not -- CPU.

Settled seeds (ref.SEEDS) and their kink ratios: (4, 256) seed 1, 3.29e-5; (2, 256) seed 2, 1.46e-4
(seed 1: 8.1e-6); (2, 128) seed 2, 5.5e-5 (seed 1: 3.1e-6)."""
import functools

import numpy as np
import pytest
import torch

import _xgat_ref as ref
from conftest import row_rel

N = ref.N_NODES
L = ref.LADDER


@pytest.fixture(scope="module")
def graph():
    return ref.make_graph()


@functools.lru_cache(maxsize=None)
def _formulas(H, C, seed):
    return ref.formulas(ref.inputs(H, C, seed), ref.make_graph(), H)


def _mask(E, H, p=0.2, seed=5):
    from oracle import gat_oracle
    return torch.from_numpy(np.stack([gat_oracle.dropout_scale(seed, np.arange(E), h, p) for h in range(H)], 1))


def test_graph_has_the_promised_degrees(graph):
    src, dst = graph
    E = graph.shape[1]
    assert graph.dtype == np.int64 and 19_000 <= E <= 20_500
    ind, outd = np.bincount(dst, minlength=N), np.bincount(src, minlength=N)
    T = len(L)
    assert ind[:T].tolist() == L and outd[:T].sum() == 0
    assert outd[ref.OUT_BASE:ref.OUT_BASE + T].tolist() == L and ind[ref.OUT_BASE:ref.OUT_BASE + T].sum() == 0
    lo, hi = ref.POOL
    for a in (slice(T, ref.OUT_BASE), slice(ref.OUT_BASE + T, lo), slice(hi, N)):
        assert ind[a].sum() == 0 and outd[a].sum() == 0
    assert hi == 1300 and N == 1400
    # the ladder nodes' other end points, and the background, lie in the pool
    assert src[dst < T].min() >= lo and src[dst < T].max() < hi
    assert dst[(src >= ref.OUT_BASE) & (src < ref.OUT_BASE + T)].min() >= lo
    assert int(((src == ref.TRIPLE[0]) & (dst == ref.TRIPLE[1])).sum()) == 3
    assert int(((src == dst)).sum()) == 1 and int(((src == ref.LOOP) & (dst == ref.LOOP)).sum()) == 1
    assert 5900 <= int(((src >= lo) & (dst >= lo)).sum()) <= 6010
    # shuffled: the ladder's columns are not contiguous, and the draw is repeatable
    assert not np.array_equal(np.sort(dst), dst) and np.array_equal(ref.make_graph(), graph)
    # the pieces the ladder promises (oracle.work_schedule: rows above T edges cut into ceil(deg / T))
    pieces = lambda T_: [-(-d // T_) for d in L if d > T_]
    assert pieces(256) == [2, 2, 3, 3, 17] and max(pieces(32)) == 129 and pieces(32)[-4:-2] == [16, 17]
    assert ind[T:].max() <= 32 and outd[ref.OUT_BASE + T:].max() <= 32  # no hub but the ladder's, at either setting
    assert int((ind > 16).sum()) > T - 10 and int(((ind > 0) & (ind <= 16)).sum()) > 100  # both sides of the 16-edge cut


@pytest.mark.parametrize("H", [2, 4])
@pytest.mark.parametrize("masked", [False, True])
def test_formulas_equal_autograd_small(H, masked):
    """Every output, gradient and intermediate (z, alpha, dz, mask dalpha, ds_src, ds_dst) against
    float64 autograd, and D = <gt, agg>, dW from G_mat and GV, dx from gt: the three backward
    formulations state one gradient."""
    assert ref.self_check(H, 8, masked) <= 1e-10


@pytest.mark.parametrize("H,C,masked", [(2, 128, True), (2, 128, False), (4, 256, True), (4, 256, False)])
def test_formulas_equal_autograd_on_the_ladder(graph, H, C, masked):
    P = ref.inputs(H, C, ref.SEEDS[(H, C)])
    mask = _mask(graph.shape[1], H) if masked else None
    taps = {}
    a, f = ref.autograd_grads(P, graph, H, ref.SLOPE, mask, taps), ref.formulas(P, graph, H, ref.SLOPE, mask)
    for k in ("out",) + ref.GRADS:
        assert ref.rel(f[k].reshape(a[k].shape), a[k]) <= 1e-10, (k, ref.rel(f[k].reshape(a[k].shape), a[k]))
    assert ref.rel(f["dz"], taps["z"].grad) <= 1e-10 and ref.rel(f["ds_src"], taps["s_src"].grad) <= 1e-10
    assert ref.rel((f["gt"] * f["agg"]).sum(-1), f["D"]) <= 1e-10
    iso = np.flatnonzero(np.bincount(graph[1], minlength=N) == 0)
    assert float(f["m"][iso].abs().max()) == 0.0 and float(f["agg"][iso].abs().max()) == 0.0
    assert float(f["inv_l"][iso].min()) == 1e16


@pytest.mark.parametrize("H,C,p", [(2, 128, 0.2), (4, 256, 0.0)])
def test_formulas_equal_the_pinned_layer(oracle, graph, H, C, p):
    """out and every gradient equal oracle.pyg_gat_conv's on the ladder graph."""
    P = ref.inputs(H, C, ref.SEEDS[(H, C)])
    mask = _mask(graph.shape[1], H, p, 5) if p > 0 else None
    f = ref.formulas(P, graph, H, ref.SLOPE, mask)
    T = {k: torch.from_numpy(P[k]).double().requires_grad_(True) for k in ("x", "W", "att_src", "att_dst", "bias")}
    out = oracle.pyg_gat_conv(T["x"], torch.from_numpy(graph), T["W"], T["att_src"], T["att_dst"], T["bias"], H,
                              negative_slope=ref.SLOPE, dropout_p=p, seed=5)
    (out * torch.from_numpy(P["G"]).double()).sum().backward()
    assert ref.rel(f["out"], out) <= 1e-12
    for k, g in (("x", "dx"), ("W", "dW"), ("att_src", "datt_src"), ("att_dst", "datt_dst"), ("bias", "dbias")):
        assert ref.rel(f[g], T[k].grad) <= 1e-10, (g, ref.rel(f[g], T[k].grad))


@pytest.mark.parametrize("H,C", ref.CASES)
def test_no_logit_near_the_kink(H, C):
    """The condition of the GPU parity cases, from the float64 reference alone: every
    |z| >= 1e-5 (|s_src| + |s_dst|), so the fp32 logit (off by a few hundred 2^-24 of that magnitude
    at worst) cannot land on the other side of the LeakyReLU kink.  ref.SEEDS holds the first
    integer seed from 1 that meets it; the seeds before it do not."""
    seed = ref.SEEDS[(H, C)]
    for s in range(1, seed):
        assert _formulas(H, C, s)["kink_ratio"] < 1e-5, s
    f = _formulas(H, C, seed)
    print(f"kink_ratio h{H} c{C} seed {seed}: {f['kink_ratio']:.3e}  z_absmax {f['z_absmax']:.3f}")
    assert f["kink_ratio"] >= 1e-5, f["kink_ratio"]


@pytest.mark.parametrize("H", [2, 4])
def test_sharp_scores_are_exact(graph, H):
    s_src, s_dst = ref.sharp_scores(0, H)
    assert s_src.dtype == np.float32 and s_src.shape == s_dst.shape == (N, H)
    assert np.array_equal(s_src * 512, np.round(s_src * 512)) and s_src.min() >= -16 and s_src.max() < 16
    d = (s_dst.astype(np.float64) - 2.0 ** -10) * 512
    assert np.array_equal(d, np.round(d)) and d.min() >= -8192 and d.max() < 8192
    src, dst = graph
    z32 = s_src[src] + s_dst[dst]                                         # fp32 sum
    z64 = s_src[src].astype(np.float64) + s_dst[dst].astype(np.float64)
    assert z32.dtype == np.float32 and np.array_equal(z32.astype(np.float64), z64)
    assert np.abs(z64).min() >= 2.0 ** -10 and np.abs(z64).max() < 32
    # the formulas take them as given, and many destinations end one-hot
    f = ref.formulas(ref.inputs(H, 128 if H == 2 else 256, 1), graph, H, scores=(s_src, s_dst))
    assert np.array_equal(f["z"].numpy(), z64) and f["kink_ratio"] > 1e-5
    amax = torch.zeros(N, H, dtype=torch.float64).scatter_reduce(0, torch.from_numpy(dst)[:, None].expand(-1, H),
                                                                  f["alpha"], "amax")
    ind = np.bincount(dst, minlength=N)
    assert int((amax[ind >= 2] > 0.99).sum()) > 100


def test_row_figures_see_what_a_whole_tensor_maximum_does_not(graph):
    """One row off by 1e-4 of its norm, or one (row, head) of ds_src off by 1e-4 of its term scale:
    max|a - b| / max|b| over the tensor stays under 1e-5, row_rel and scaled_rows do not.

    For out the wrong row is the degree-1 destination's: row_rel reports its 1e-4 exactly.  On this
    recipe that row is no small one -- a single unaveraged message, it holds the largest entries
    of out, and no out row is below a quarter of the tensor's maximum (the bias sets a floor) -- so
    the whole-tensor figure is not blind to it here; the blindness is shown where rows do differ in
    size by more than 10: the aggregate of the 4100-edge destination (0.03 of the largest
    aggregate entry) and ds_src."""
    H, C = ref.CASES[0]
    f = _formulas(H, C, ref.SEEDS[(H, C)])
    old = lambda a, b: float((a - b).abs().max() / b.abs().max())
    out = f["out"].clone()
    assert np.bincount(graph[1], minlength=N)[0] == 1
    out[0] *= 1 + 1e-4
    r, row, _ = row_rel(out, f["out"])
    assert r > 1e-5 and row == 0 and abs(r - 1e-4) < 1e-8
    print("degree-1 out row off by 1e-4: whole-tensor figure", old(out, f["out"]), "row_rel", r)
    hub = len(L) - 1
    agg = f["agg"].reshape(N * H, -1)
    bad = agg.clone()
    bad[hub * H] *= 1 + 1e-4
    assert old(bad, agg) <= 1e-5
    r, row, _ = row_rel(bad, agg)
    assert r > 1e-5 and row == hub * H and abs(r - 1e-4) < 1e-8
    # the source of a two-edge out-ladder node, head 1
    j = ref.OUT_BASE + 1
    ds, sc = f["ds_src"], f["scale_ds_src"]
    assert np.bincount(graph[0], minlength=N)[j] == 2 and float(sc[j, 1]) > 0
    bad = ds.clone()
    bad[j, 1] += 1e-4 * sc[j, 1]
    assert old(bad, ds) <= 1e-5
    worst, zmax = ref.scaled_rows(bad.reshape(-1, 1), ds.reshape(-1, 1), sc.reshape(-1))
    assert worst > 1e-5 and abs(worst - 1e-4) < 1e-8 and zmax == 0.0
    # sources without out-edges have scale 0 and ds_src exactly 0
    none = np.flatnonzero(np.bincount(graph[0], minlength=N) == 0)
    assert float(sc[none].abs().max()) == 0.0 and float(ds[none].abs().max()) == 0.0
