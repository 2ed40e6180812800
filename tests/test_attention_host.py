"""Attention weights without a GPU: the references of tests/_attn_ref.py against a brute-force loop
over the destinations of the degree ladder, the new library entries and their argument checks
(which return before any device work), the Python surface, and the float32 restatement's own
error figure -- the quantity the GPU tests' tolerance is four times of.  CPU."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import _attn_ref as R

SLOPE = 0.2


@pytest.fixture(scope="module")
def ladder():
    ei = R.ladder_graph()
    return ei, ei.shape[1]


def _scores(n, H, scale, seed):
    rng = np.random.default_rng(seed)
    return ((scale * rng.uniform(-1, 1, (n, H))).astype(np.float32) for _ in range(2))


def test_ladder_graph_has_the_stated_degrees(ladder):
    ei, E = ladder
    deg = np.bincount(ei[1], minlength=R.N_NODES)
    assert tuple(deg[:len(R.LADDER)]) == R.LADDER and deg[len(R.LADDER):].sum() == 0
    assert E == sum(R.LADDER) and ei.max() < R.N_NODES
    assert (ei[0] == ei[1]).sum() >= 13                       # self-loops
    assert len(np.unique(ei, axis=1).T) < E                   # duplicate edges
    assert (np.diff(ei[1]) < 0).any()                         # columns are not sorted by destination


@pytest.mark.parametrize("mode", [R.MODE_PYG, R.MODE_CUSTOM])
@pytest.mark.parametrize("edge", [False, True])
def test_v1_reference_matches_the_brute_force_loop(ladder, mode, edge):
    ei, E = ladder
    H = 2
    s_src, s_dst = _scores(R.N_NODES, H, 40.0, 1)
    et = (np.random.default_rng(2).uniform(-3, 3, (E, H))).astype(np.float32) if edge else None
    ref = R.v1_alpha(s_src, s_dst, ei, mode, SLOPE, et).numpy()

    def logit(k, h):
        z = float(s_src[ei[0, k], h]) + float(s_dst[ei[1, k], h]) + (float(et[k, h]) if edge else 0.0)
        e = z if z > 0 else SLOPE * z
        return min(max(e, -10.0), 10.0) if mode == R.MODE_CUSTOM else e

    brute = R.brute_alpha(logit, ei, R.N_NODES, H, 1e-9 if mode == R.MODE_CUSTOM else 1e-16, mode == R.MODE_PYG)
    assert np.abs(ref - brute).max() <= 1e-13
    sums = np.zeros((R.N_NODES, H))
    np.add.at(sums, ei[1], ref)
    has = np.bincount(ei[1], minlength=R.N_NODES) > 0
    # a row's weights sum to l / (l + eps): custom mode's l is at least exp(-10) against eps 1e-9
    tol = 1e-9 / np.exp(-10.0) * 1.01 if mode == R.MODE_CUSTOM else 1e-8
    assert np.abs(sums[has] - 1).max() <= tol and np.abs(sums[~has]).max() == 0


def test_v2_reference_matches_the_brute_force_loop(ladder):
    ei, _ = ladder
    H, C = 2, 8
    rng = np.random.default_rng(3)
    xl, xr = (rng.standard_normal((R.N_NODES, H * C)).astype(np.float32) for _ in range(2))
    att = rng.standard_normal((H, C)).astype(np.float32)
    ref = R.v2_alpha(xl, xr, att, ei, H, SLOPE).numpy()

    def logit(k, h):
        t = xl[ei[0, k], h * C:(h + 1) * C].astype(np.float64) + xr[ei[1, k], h * C:(h + 1) * C]
        return float((np.where(t > 0, t, SLOPE * t) * att[h]).sum())

    assert np.abs(ref - R.brute_alpha(logit, ei, R.N_NODES, H, 1e-16, True)).max() <= 1e-13


@pytest.mark.parametrize("H", [1, 2, 4])
def test_topk_reference_matches_a_plain_sort(ladder, H):
    ei, E = ladder
    val = (np.random.default_rng(4).integers(0, 4, (E, H)) / 16.0).astype(np.float32)
    mean = val.astype(np.float64).mean(1)                      # exact for multiples of 1/16
    for k in (1, 17, 32):
        eid, v, cnt = R.topk_ref(val, ei, R.N_NODES, k)
        for i in range(len(R.LADDER) + 2):
            ks = sorted(np.flatnonzero(ei[1] == i).tolist(), key=lambda c: (-mean[c], c))[:k]
            assert cnt[i] == len(ks) == min(k, (ei[1] == i).sum())
            assert eid[i, :cnt[i]].tolist() == ks and (eid[i, cnt[i]:] == -1).all()
            assert (v[i, :cnt[i]] == mean[ks].astype(np.float32)).all() and (v[i, cnt[i]:] == 0).all()


def test_restatement_error_figures(ladder):
    """The float32 restatement against float64 on logits spanning +-80: the figure is of the
    order of the logits' own rounding (|z| 2^-24), far below 1, and is printed for the record."""
    ei, E = ladder
    figs = {}
    for H in (1, 4):
        s_src, s_dst = _scores(R.N_NODES, H, 40.0, 10 + H)
        et = np.random.default_rng(5).uniform(-3, 3, (E, H)).astype(np.float32)
        for name, mode, term in (("pyg", R.MODE_PYG, None), ("pyg_edge", R.MODE_PYG, et), ("custom", R.MODE_CUSTOM, None)):
            a64 = R.v1_alpha(s_src, s_dst, ei, mode, SLOPE, term)
            a32 = R.v1_alpha(s_src, s_dst, ei, mode, SLOPE, term, dtype=torch.float32)
            assert a32.dtype == torch.float32
            figs[f"{name}_h{H}"] = R.metric(a32, a64, ei, R.N_NODES)
    rng = np.random.default_rng(6)
    xl, xr = (0.5 * rng.standard_normal((R.N_NODES, 128)).astype(np.float32) for _ in range(2))
    att = (0.2 * rng.standard_normal((2, 64))).astype(np.float32)
    figs["gatv2_h2_c64"] = R.metric(R.v2_alpha(xl, xr, att, ei, 2, SLOPE, dtype=torch.float32),
                                    R.v2_alpha(xl, xr, att, ei, 2, SLOPE), ei, R.N_NODES)
    print("[attention] float32 restatement, max |alpha - alpha64| / max_dest alpha64:", figs)
    for k, f in figs.items():
        assert 0 < f < 1e-3, (k, f)
        assert R.bound(f) == max(4 * f, 2.0 ** -24)


def test_entries_exist_and_refuse_bad_arguments_without_a_gpu(pkg):
    lib = pkg._lib.load()
    for name in ("ppgat_attention", "ppgat_dynatt_attention", "ppgat_attention_topk"):
        assert hasattr(lib, name) and name in pkg._lib.SIGNATURES
    assert lib.ppgat_version() == 3
    err = lib.ppgat_last_error
    for k in (0, 33):
        assert lib.ppgat_attention_topk(None, None, None, 10, 0, 1, k, None, None, None, None) == 1
        assert b"k must be" in err()
    assert lib.ppgat_attention_topk(None, None, None, 10, 0, 1, 8, None, None, None, None) == 1  # null outputs
    # an unsupported GATv2 shape: refused before anything else is looked at
    assert lib.ppgat_dynatt_attention(None, None, None, 10, 0, 3, 64, None, None, None, None, None, SLOPE, 0, None,
                                      None) == 2
    assert b"heads, channels" in err()
    sched = pkg._lib.Schedule(None, None, None, 0, 0, None, None, 0, -1)
    v1 = lambda s, order, heads=1, mode=0: lib.ppgat_attention(s, None, None, None, 0, 0, heads, None, None, None, None,
                                                                mode, SLOPE, order, None, None)
    assert v1(ctypes.byref(sched), 2) == 1 and b"order" in err()
    assert lib.ppgat_dynatt_attention(ctypes.byref(sched), None, None, 0, 0, 1, 64, None, None, None, None, None,
                                      SLOPE, 2, None, None) == 1 and b"order" in err()
    assert v1(None, 0) == 1 and b"schedule" in err()
    assert lib.ppgat_dynatt_attention(None, None, None, 0, 0, 1, 64, None, None, None, None, None, SLOPE, 0, None,
                                      None) == 1 and b"schedule" in err()
    assert v1(ctypes.byref(sched), 0, heads=9) == 2
    assert v1(ctypes.byref(sched), 0, mode=2) == 1
    assert v1(ctypes.byref(sched), 0) == 0 and v1(ctypes.byref(sched), 1) == 0        # an empty graph: nothing to do
    bad = pkg._lib.Schedule(None, None, None, 3, 5, None, None, 0, -1)
    assert v1(ctypes.byref(bad), 0) == 1 and b"inconsistent" in err()


def test_python_surface(pkg):
    for name in ("attention_weights", "gatv2_attention_weights", "attention_topk", "gat_layer_attention",
                 "gatv2_layer_attention"):
        assert callable(getattr(pkg.hip_ops, name))
    assert inspect.signature(pkg.hip_ops.attention_weights).parameters["order"].default == "edge"
    for cls in (pkg.GATConv, pkg.GATv2Conv, pkg.SimpleGATLayer):
        for fn in (cls.forward, cls.forward_segments):
            assert "return_attention_weights" in inspect.signature(fn).parameters, (cls, fn)
        assert callable(cls.attention)
    model = import_module_of(pkg, "model")
    for cls in (model.PyGGAT, model.PyGGATv2, model.CustomGAT):
        assert list(inspect.signature(cls.attention).parameters)[:4] == ["self", "item_feats", "edge_index", "edge_attr"]
    ev = import_module_of(pkg, "evaluation")
    assert list(inspect.signature(ev.attention_topk).parameters) == ["model", "item_feats", "edge_index", "k", "layer",
                                                                      "edge_attr"]
    # no CPU path, as everywhere in the package
    s = torch.zeros(4, 1)
    with pytest.raises(RuntimeError, match="ROCm"):
        pkg.hip_ops.attention_weights(None, s, s, s, s, 1, 0, SLOPE)
    with pytest.raises(RuntimeError, match="ROCm"):
        pkg.hip_ops.attention_topk(None, s, 4)
    conv = pkg.GATConv(8, 8, heads=1, concat=False, add_self_loops=False)
    with pytest.raises(RuntimeError, match="ROCm"):
        conv(torch.randn(5, 8), torch.tensor([[0, 1], [1, 2]]), return_attention_weights=True)


def import_module_of(pkg, name):
    from importlib import import_module
    return import_module(f"{pkg.__name__}.{name}")


def test_trainer_refuses_attention_out_where_it_cannot_run(pkg):
    train = import_module_of(pkg, "train")
    with pytest.raises(NotImplementedError, match="attention-out"):
        train.main(["--synthetic", "cfg1", "--attention-out", "x.npz", "--world-size", "2"])
    with pytest.raises(NotImplementedError, match="attention-out"):
        train.main(["--synthetic", "cfg1", "--attention-out", "x.npz", "--model-family", "lightgcn"])
    args = train.build_parser().parse_args(["--attention-out", "a.npz"])
    assert args.attention_k == 10 and args.attention_out == "a.npz"
