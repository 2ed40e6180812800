"""The multi-head aggregate-then-transform layer (csrc/ppgat_xgat.hip) stage by stage on the GPU,
against the float64 restatement tests/_xgat_ref.py evaluated on the same fp32 inputs: the whole
layer on the degree-ladder graph in every backward formulation and both weight-gradient forms, on
256- and 32-edge schedules (hubs of 2..17 and of 2..129 pieces: the one-wave and the workgroup
merges, their unrolled loops entered with a remainder), then each forward and deferred-D backward
stage on its own with its inputs given in fp32, and the rectangular (n_src > n_dst) view with its
phased forward and split backward.  The host test (tests/test_xgat_host.py) checks that no logit of
the recipe sits within 1e-5 of the LeakyReLU kink; the sharp scores are exact in fp32 by
construction, so both sides take the same branch on every edge.

The asserted bounds are the project's: 1e-5 for rows, scaled rows, per-edge figures and matrix
gradients, 1e-4 for attention vectors.  The measured figures (write_report; profiles/r16/parity/
xgat_*.json) are in DESIGN.md section 15.1: whole layer out rows 3.9e-7, dx rows on their term scale
9.0e-8, dW 4.9e-7, datt 1.4e-6; agg rows 7.5e-7 (sharp scores), m 0 ulp, inv_l 3.4e-7; dalpha 4.3e-8,
acc rows 6.5e-7, dz 9.5e-7, ds_src 8.2e-7 at worst."""
import functools
import importlib
import json
import types

import numpy as np
import pytest
import torch

import _xgat_ref as ref
from conftest import row_rel, write_report

pytestmark = pytest.mark.gpu

TOL, TOL_ATT = 1e-5, 1e-4  # the project's bounds: rows, per-edge figures and gradients; attention vectors
SEED = 20250114
N = ref.N_NODES
K = ref.K_IN
SLOPE = ref.SLOPE
LEAVES = ("x", "W", "att_src", "att_dst", "bias")
N_DST = 1000  # the rectangular view's destination rows


@pytest.fixture(scope="module")
def hip_ops(pkg):
    return importlib.import_module(pkg.__name__ + ".hip_ops")


@pytest.fixture(scope="module")
def launch(pkg):
    return importlib.import_module(pkg.__name__ + "._launch")


@pytest.fixture(scope="module", autouse=True)
def _epoch_zero(pkg, cuda):
    pkg._lib.dropout_set_epoch(0, cuda)
    yield
    pkg._lib.dropout_set_epoch(0, cuda)


def _pieces(deg, T):
    return {int(r): int(-(-deg[r] // T)) for r in np.flatnonzero(deg > T)}


def _check_schedule(sched, deg, T):
    """Hubs, pieces and the short/long cut of a device schedule against the degrees."""
    want = _pieces(deg, T)
    assert sched.n_hubs == len(want) and sched.n_hub_items == sum(want.values()) and sched.n_items == \
        sum(want.values()) + int((deg <= T).sum())
    rows = sched.hub_row[:sched.n_hubs].cpu().tolist()
    cnt = np.diff(sched.hub_ptr[:sched.n_hubs + 1].cpu().numpy()).tolist()
    assert dict(zip(rows, cnt)) == want
    assert sched.n_long_items == sched.n_hub_items + int(((deg > 16) & (deg <= T)).sum())
    assert sched.n_hub_items < sched.n_long_items < sched.n_items  # both k_xgat_dz launches run


@pytest.fixture(scope="module")
def graphs(pkg, hip_ops, cuda):
    """{max_edges: CSRGraph} over the ladder graph, with the hubs and pieces the ladder promises."""
    ei = ref.make_graph()
    eid = torch.from_numpy(ei).to(cuda)
    by = {256: hip_ops.csr_build(eid, N), 32: hip_ops.csr_build(eid, N, max_edges=32)}
    ind, outd = np.bincount(ei[1], minlength=N), np.bincount(ei[0], minlength=N)
    for T, g in by.items():
        _check_schedule(g.fwd_sched, ind, T)
        _check_schedule(g.bwd_sched, outd, T)
    L = ref.LADDER
    assert [_pieces(ind, 256)[t] for t in range(len(L)) if L[t] > 256] == [2, 2, 3, 3, 17]   # both merge kinds
    p32 = _pieces(outd, 32)
    assert [p32[ref.OUT_BASE + t] for t in range(len(L)) if L[t] > 32] == [2, 2, 3, 4, 5, 8, 9, 16, 17, 22, 129]
    return types.SimpleNamespace(ei=ei, by_max=by, E=ei.shape[1], ind=ind, outd=outd)


@functools.lru_cache(maxsize=None)
def _mask(E: int, H: int, p: float):
    from oracle import gat_oracle
    if p <= 0:
        return None
    return torch.from_numpy(np.stack([gat_oracle.dropout_scale(SEED, np.arange(E), h, p) for h in range(H)], 1))


@functools.lru_cache(maxsize=None)
def _inputs(H: int, C: int):
    return ref.inputs(H, C, ref.SEEDS[(H, C)])  # shared: callers copy before they change anything


@functools.lru_cache(maxsize=None)
def _scores32(H: int, C: int, kind: str):
    """The fp32 node scores the stage tests feed: the recipe's (the float64 x A^T rounded) or the sharp ones."""
    if kind == "sharp":
        return ref.sharp_scores(0, H)
    f = _reference(H, C, 0.0)
    return f["s_src"].float().numpy(), f["s_dst"].float().numpy()


@functools.lru_cache(maxsize=None)
def _reference(H: int, C: int, p: float, kind: str = "layer"):
    """The float64 layer, gradients and intermediates on the recipe's fp32 inputs, once per case.
    ``kind`` "layer": scores from x A^T; "recipe" / "sharp": the fp32 scores of _scores32 given."""
    ei = ref.make_graph()
    scores = None if kind == "layer" else _scores32(H, C, kind)
    return ref.formulas(_inputs(H, C), ei, H, SLOPE, _mask(ei.shape[1], H, p), scores=scores)


def _dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _run(hip_ops, pkg, g, P, H, C, p, cuda):
    """out and the gradients of LEAVES through hip_ops.gat_layer, which hands layers wider than
    their input (H C > 256) to gat_layer_x; (2, 128) is exactly as wide, so it is handed there here."""
    T = {k: _dev(P[k], cuda).requires_grad_(True) for k in LEAVES}
    if H * C > K:
        out = hip_ops.gat_layer(T["x"], T["W"], T["att_src"], T["att_dst"], T["bias"], g, H, C, pkg._lib.MODE_PYG,
                                SLOPE, p, SEED)
    else:
        assert hip_ops.xgat_supported(K, H, C)
        ops_gat = importlib.import_module(pkg.__name__ + ".ops_gat")  # the name gat_layer calls (and the test counts)
        out = ops_gat.gat_layer_x(T["x"], T["W"], T["att_src"], T["att_dst"], T["bias"], hip_ops.XViews.of_graph(g), H,
                                  C, SLOPE, p, SEED)
    return (out.detach(),) + tuple(torch.autograd.grad(out, [T[k] for k in LEAVES], _dev(P["G"], cuda)))


def _figures(got, want):
    out, dx, dW, das, dad, db = got[:6]
    n = out.size(0)
    fig = {"z_absmax": want["z_absmax"], "kink_ratio": want["kink_ratio"]}
    fig["out_row_rel"] = row_rel(out, want["out"][:n])[0]
    fig["dx_whole"] = ref.rel(dx, want["dx"])
    fig["dx_scaled_rows"], fig["dx_zero_scale_rows_absmax"] = ref.scaled_rows(dx, want["dx"], want["scale_x"])
    fig["dx_plain_rows"] = row_rel(dx, want["dx"])[0]  # reported, not asserted (rows whose terms cancel)
    fig["dW"], fig["dbias"] = ref.rel(dW, want["dW"]), ref.rel(db, want["dbias"])
    fig["datt_src"], fig["datt_dst"] = ref.rel(das, want["datt_src"]), ref.rel(dad, want["datt_dst"])
    return fig


def _check(fig):
    print(json.dumps(fig))
    assert fig["out_row_rel"] <= TOL, fig
    assert fig["dx_whole"] <= TOL and fig["dx_scaled_rows"] <= TOL and fig["dx_zero_scale_rows_absmax"] == 0.0, fig
    assert fig["dW"] <= TOL and fig["dbias"] <= TOL, fig
    assert fig["datt_src"] <= TOL_ATT and fig["datt_dst"] <= TOL_ATT, fig
    return fig


# ---------------------------------------------------------------------------------------------
# the whole layer on the ladder
# ---------------------------------------------------------------------------------------------
LAYER_CASES = [(H, C, gm, am) for (H, C) in ref.CASES if C == 256
               for gm, am in (("gd", "keep"), ("gd", "free"), ("g", "keep"), ("gt", "keep"))] + \
              [(2, 128, gm, "keep") for gm in ("gd", "g", "gt")]


@pytest.mark.parametrize("H,C,gather,agg_mode", LAYER_CASES)
def test_layer_on_the_ladder(pkg, hip_ops, graphs, cuda, monkeypatch, H, C, gather, agg_mode):
    """hip_ops.gat_layer -> gat_layer_x (asserted: five calls arrive there): out rows, dx rows on their term scale and the parameter
    gradients against float64 at p = 0 and 0.2 on both schedules; zero-in-degree rows are the bias
    bit for bit; a second run gives the same bits; the two schedules agree within the bound."""
    monkeypatch.setenv("PPGAT_XGAT_GATHER", gather)
    monkeypatch.setenv("PPGAT_XGAT_AGG", agg_mode)
    calls = []
    real = hip_ops.gat_layer_x
    ops_gat = importlib.import_module(pkg.__name__ + ".ops_gat")  # where gat_layer looks gat_layer_x up
    monkeypatch.setattr(ops_gat, "gat_layer_x", lambda *a, **k: calls.append(1) or real(*a, **k))
    mode = hip_ops._xgat_gather_mode(C, H)
    if C == 128:
        assert mode == "gt"  # whatever the variable says: the g-gathering passes are C == 256 only
    else:
        assert mode == gather
        assert hip_ops._xgat_keep_agg(N, N, H, K, C, cuda, graphs.E) == (agg_mode == "keep" or gather != "gd")
    P = _inputs(H, C)
    iso = _dev(np.flatnonzero(graphs.ind == 0), cuda)
    bias = _dev(P["bias"], cuda)
    record, runs = {}, {}
    for p in (0.0, 0.2):
        want = _reference(H, C, p)
        for T, g in graphs.by_max.items():
            got = _run(hip_ops, pkg, g, P, H, C, p, cuda)
            assert iso.numel() >= 100 + 22 + 56 and torch.equal(got[0][iso], bias.expand(iso.numel(), C))
            record[f"p{p}_max_edges{T}"] = _check(_figures(got, want))
            runs[(p, T)] = got
    again = _run(hip_ops, pkg, graphs.by_max[32], P, H, C, 0.2, cuda)
    assert all(torch.equal(a, b) for a, b in zip(again, runs[(0.2, 32)]))
    assert len(calls) == 5
    for p in (0.0, 0.2):
        a, b = runs[(p, 256)], runs[(p, 32)]
        sched = {"out_rows": row_rel(a[0], b[0])[0]}
        sched.update({k: ref.rel(a[i], b[i]) for i, k in ((1, "dx"), (2, "dW"), (3, "datt_src"), (4, "datt_dst"),
                                                           (5, "dbias"))})
        record[f"p{p}_schedules_256_vs_32"] = sched
        print(json.dumps(sched))
        assert all(v <= TOL for v in sched.values()), sched
    write_report(f"xgat_layer_h{H}_c{C}_{gather}_{agg_mode}", record)


# ---------------------------------------------------------------------------------------------
# forward pieces
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,C", ref.CASES)
def test_weights(hip_ops, launch, cuda, H, C):
    """A against float64, each entry on the scale sum_c |att| |W|; Wt bitwise the permutation; Wg
    bitwise W / H (H a power of two)."""
    P = _inputs(H, C)
    W, a_s, a_d = (_dev(P[k], cuda) for k in ("W", "att_src", "att_dst"))
    A = torch.empty(2, H, K, device=cuda)
    Wt = torch.empty(H * K, C, device=cuda)
    Wg = torch.empty(C, H * K, device=cuda)
    launch.xgat_weights(W, a_s, a_d, H, C, A=A, Wt=Wt, Wg=Wg)
    assert torch.equal(A, hip_ops.xgat_att_proj(W, a_s, a_d, H, C))
    W3 = torch.from_numpy(P["W"]).double().view(H, C, K)
    att = torch.stack([torch.from_numpy(P["att_src"]), torch.from_numpy(P["att_dst"])]).double()   # [2, H, C]
    want = torch.einsum("vhc,hck->vhk", att, W3)
    scale = torch.einsum("vhc,hck->vhk", att.abs(), W3.abs())
    fig = {"A_on_term_scale": float(((A.double().cpu() - want).abs() / scale).max())}
    assert fig["A_on_term_scale"] <= TOL, fig
    Wc = torch.from_numpy(P["W"]).view(H, C, K)
    assert torch.equal(Wt.cpu(), Wc.permute(0, 2, 1).reshape(H * K, C))
    assert torch.equal(Wg.cpu(), (Wc * np.float32(1.0 / H)).permute(1, 0, 2).reshape(C, H * K))
    write_report(f"xgat_weights_h{H}_c{C}", fig)


@pytest.mark.parametrize("H", [2, 4])
def test_scores_rows(pkg, hip_ops, launch, cuda, H):
    """s = x A^T with the fp32 A given, each entry on the scale sum_k |x_k| |A_k|: 1, 3, 4, 5, 17
    and 1400 rows (four rows per wave and iteration), a nonzero first row, and s_dst written below
    n_dst only -- everything else keeps its sentinel."""
    C = 256
    P = _inputs(H, C)
    x = _dev(P["x"], cuda)
    A = hip_ops.xgat_att_proj(_dev(P["W"], cuda), _dev(P["att_src"], cuda), _dev(P["att_dst"], cuda), H, C)
    A64, x64 = A.double().cpu().view(2 * H, K), torch.from_numpy(P["x"]).double()
    want, scale = x64 @ A64.t(), x64.abs() @ A64.abs().t()                                       # [N, 2 H]
    worst = 0.0

    def err(got, rows, half):
        return float(((got.double().cpu() - want[rows, half]).abs() / scale[rows, half]).max())

    src_h, dst_h = slice(0, H), slice(H, 2 * H)
    for n in (1, 3, 4, 5, 17, N):
        s_src = torch.full((n + 3, H), 7.0, device=cuda)
        s_dst = torch.full((n + 3, H), 7.0, device=cuda)
        hip_ops.xgat_scores_rows(x[:n], A, s_src, s_dst)
        assert bool((s_src[n:] == 7.0).all()) and bool((s_dst[n:] == 7.0).all())
        worst = max(worst, err(s_src[:n], slice(0, n), src_h), err(s_dst[:n], slice(0, n), dst_h))
        only = torch.full((n + 3, H), 7.0, device=cuda)
        hip_ops.xgat_scores_rows(x[:n], A, only)
        assert torch.equal(only, s_src)  # per row the same arithmetic whatever the launch
    # rows [r0, r0 + n) into s_src[r0:], nothing else touched
    full = torch.full((N, H), 7.0, device=cuda)
    hip_ops.xgat_scores_rows(x, A, full)
    for r0, n in ((1, 1), (3, 6), (1001, 399), (1203, 197)):
        s_src = torch.full((N, H), 7.0, device=cuda)
        launch.xgat_scores(x, r0, n, A, s_src)
        assert bool((s_src[:r0] == 7.0).all()) and bool((s_src[r0 + n:] == 7.0).all())
        assert torch.equal(s_src[r0:r0 + n], full[r0:r0 + n])
    # more rows than destinations: s_dst below n_dst only
    lib, _lib = pkg._lib.load(), pkg._lib
    for n_rows, n_dst in ((17, 5), (N, N_DST), (9, 0)):
        s_src = torch.full((N, H), 7.0, device=cuda)
        s_dst = torch.full((N, H), 7.0, device=cuda)
        _lib.check(lib.ppgat_xgat_scores(x.data_ptr(), K, n_rows, n_dst, K, H, A.data_ptr(), s_src.data_ptr(),
                                         s_dst.data_ptr(), _lib.stream_handle(cuda)), "xgat_scores")
        assert bool((s_dst[n_dst:] == 7.0).all()) and bool((s_src[n_rows:] == 7.0).all())
        assert torch.equal(s_src[:n_rows], full[:n_rows])
        if n_dst:
            worst = max(worst, err(s_dst[:n_dst], slice(0, n_dst), dst_h))
    fig = {"scores_on_term_scale": worst}
    assert worst <= TOL, fig
    write_report(f"xgat_scores_h{H}", fig)


def _host_m(s_src, s_dst, ei, n):
    """max over in-edges of lrelu(z) as fp32 arithmetic does it (0 where there is none)."""
    z = s_src[ei[0]] + s_dst[ei[1]]
    assert z.dtype == np.float32
    e = np.where(z > 0, z, z * np.float32(SLOPE)).astype(np.float32)
    m = np.full((n, z.shape[1]), -np.inf, np.float32)
    np.maximum.at(m, ei[1], e)
    return np.where(np.isinf(m), np.float32(0), m)


@pytest.mark.parametrize("kind", ["recipe", "sharp"])
@pytest.mark.parametrize("H,C", [(4, 256), (2, 256)])
def test_forward_pass_with_given_scores(hip_ops, graphs, cuda, H, C, kind):
    """hip_ops.xgat_forward(scores=..., keep_agg=True) on both schedules, p = 0 and 0.2: agg per
    (destination, head) row, m within one ulp of the fp32 host maximum, inv_l, the zero-in-degree
    rows, and xbits = the column maxima of |x| over the SOURCES of an edge, bit for bit (the rows
    without an out-edge are 1e3 larger here: no all-rows maximum passes)."""
    P = _inputs(H, C)
    s32, d32 = _scores32(H, C, kind)
    x = np.array(P["x"])
    x[graphs.outd == 0] *= np.float32(1e3)
    xbits_want = torch.from_numpy(np.abs(x[graphs.outd > 0]).max(0)).view(torch.int32)
    assert not np.array_equal(np.abs(x).max(0), np.abs(x[graphs.outd > 0]).max(0))
    xd, W, a_s, a_d, bias = (_dev(a, cuda) for a in (x, P["W"], P["att_src"], P["att_dst"], P["bias"]))
    m_host = _host_m(s32, d32, graphs.ei, N)
    iso = np.flatnonzero(graphs.ind == 0)
    record = {}
    for p in (0.0, 0.2):
        want = _reference(H, C, p, kind)
        if kind == "sharp":
            assert np.array_equal(want["z"].numpy(), (s32[graphs.ei[0]] + d32[graphs.ei[1]]).astype(np.float64))
        for T, g in graphs.by_max.items():
            v = hip_ops.XViews.of_graph(g)
            out, saved = hip_ops.xgat_forward(xd, W, a_s, a_d, bias, v, H, C, SLOPE, p, SEED,
                                              scores=(_dev(s32, cuda), _dev(d32, cuda)), keep_agg=True)
            agg, m, inv_l = saved["agg"], saved["m"].cpu().numpy(), saved["inv_l"].double().cpu()
            fig = {"z_absmax": want["z_absmax"]}
            fig["agg_row_rel"], _, fig["agg_zero_rows_absmax"] = row_rel(agg.view(N * H, K), want["agg"].view(N * H, K))
            fig["m_ulps"] = float((np.abs(m.astype(np.float64) - m_host) / np.spacing(np.abs(m_host))).max())
            fig["m_vs_float64"] = float((torch.from_numpy(m).double() - want["m"]).abs().max())
            fig["inv_l_rel"] = float(((inv_l - want["inv_l"]).abs() / want["inv_l"]).max())
            fig["out_row_rel"] = row_rel(out, want["out"])[0]
            print(json.dumps(fig))
            assert fig["agg_row_rel"] <= TOL and fig["agg_zero_rows_absmax"] == 0.0, fig
            assert fig["m_ulps"] <= 1.0 and fig["inv_l_rel"] <= TOL and fig["out_row_rel"] <= TOL, fig
            assert not m[iso].any() and not agg[_dev(iso, cuda)].any()
            assert torch.equal(saved["xbits"].cpu(), xbits_want)
            if p > 0:
                assert int(saved["seed_buf"].item()) == SEED  # epoch 0: the mask seed is the call's
            record[f"p{p}_max_edges{T}"] = fig
        if p == 0.0:  # many destinations one-hot under the sharp scores (a wide softmax otherwise)
            top = torch.zeros(N, H, dtype=torch.float64).scatter_reduce(
                0, torch.from_numpy(graphs.ei[1])[:, None].expand(-1, H), want["alpha"], "amax")
            record["one_hot_rows"] = int((top[graphs.ind >= 2] > 0.99).sum())
            assert kind != "sharp" or record["one_hot_rows"] > 100
    write_report(f"xgat_fwd_{kind}_h{H}", record)


# ---------------------------------------------------------------------------------------------
# deferred-D backward pieces
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [2, 4])
def test_nstate_packs(launch, cuda, H):
    """{s_dst, m, inv_l, D or 0} per (row, head), bit for bit; set_d changes the fourth component only."""
    for n in (1, 255, N):
        g = torch.Generator().manual_seed(n)
        s_dst, m, inv_l, D = (torch.randn(n, H, generator=g).to(cuda) for _ in range(4))
        ns = torch.full((n + 1, H, 4), 7.0, device=cuda)
        launch.xgat_nstate(s_dst, m, inv_l, None, n, H, ns)
        assert torch.equal(ns[:n], torch.stack([s_dst, m, inv_l, torch.zeros_like(D)], -1)) and bool((ns[n] == 7.0).all())
        launch.xgat_nstate_set_d(ns, D, n, H)
        assert torch.equal(ns[:n], torch.stack([s_dst, m, inv_l, D], -1)) and bool((ns[n] == 7.0).all())
        ns2 = torch.full((n + 1, H, 4), 7.0, device=cuda)
        launch.xgat_nstate(s_dst, m, inv_l, D, n, H, ns2)
        assert torch.equal(ns2, ns)


def _stage_inputs(H, C, p, kind, graphs, g, cuda):
    """The edge passes' fp32 inputs derived from the reference, and what they must give, in float64
    FROM those fp32 inputs (so the comparison carries no rounding of the inputs), per CSC slot."""
    P = _inputs(H, C)
    want = _reference(H, C, p, kind)
    s32, d32 = _scores32(H, C, kind)
    f32 = lambda t: t.float().numpy()
    hs, m, inv_l, D = f32(want["hs"]).reshape(N, H * C), f32(want["m"]), f32(want["inv_l"]), f32(want["D"])
    G = np.array(P["G"])
    G[graphs.ind == 0] *= np.float32(1e3)  # never gathered: outside gbits, and no term of any sum
    eid = g.csc_eid.cpu().numpy().astype(np.int64)
    src, dst = graphs.ei[0][eid], graphs.ei[1][eid]
    assert np.array_equal(src, np.sort(src))
    d = lambda a: torch.from_numpy(np.asarray(a)).double()
    z = d(s32)[src] + d(d32)[dst]
    af = torch.exp(torch.nn.functional.leaky_relu(z, SLOPE) - d(m)[dst]) * d(inv_l)[dst]
    mk = torch.ones(len(eid), H, dtype=torch.float64) if p <= 0 else _mask(graphs.E, H, p)[eid].double()
    beta = af * mk
    gi = d(G)[dst]
    dal, dal_scale = torch.zeros(len(eid), H, dtype=torch.float64), torch.zeros(len(eid), H, dtype=torch.float64)
    acc, acc_mag = torch.zeros(N, H, C, dtype=torch.float64), torch.zeros(N, H, C, dtype=torch.float64)
    ts = torch.from_numpy(src)
    for h in range(H):
        hj = d(hs).view(N, H, C)[:, h][src]
        dal[:, h], dal_scale[:, h] = (gi * hj).sum(-1), (gi.abs() * hj.abs()).sum(-1)
        acc[:, h].index_add_(0, ts, beta[:, h, None] * gi)
        acc_mag[:, h].index_add_(0, ts, beta[:, h, None] * gi.abs())
    a1 = af * torch.where(z > 0, torch.ones_like(z), torch.full_like(z, SLOPE))
    return types.SimpleNamespace(
        P=P, want=want, s32=s32, d32=d32, hs=hs, m=m, inv_l=inv_l, D=D, G=G, src=src, dst=dst, ts=ts, beta=beta,
        dal=dal, dal_scale=dal_scale, acc=acc.view(N, H * C), acc_scale=acc_mag.view(N, H * C).norm(dim=1), a1=a1, mk=mk,
        gbits=torch.from_numpy(np.abs(G[graphs.ind > 0]).max(0)).view(torch.int32))


def _per_edge(got, want, scale):
    """max over the entries with scale > 0 of |got - want| / scale, and max |got| where scale == 0."""
    got, nz = got.double().cpu(), scale > 0
    worst = float(((got - want).abs()[nz] / scale[nz]).max())
    return worst, (float(got[~nz].abs().max()) if (~nz).any() else 0.0)


@pytest.mark.parametrize("kind", ["recipe", "sharp"])
@pytest.mark.parametrize("H", [4, 2])
def test_edge_pass_deferred_d(hip_ops, launch, graphs, cuda, H, kind):
    """ppgat_xgat_bwd_edges_gd_colmax as _xgat_backward_deferred_d calls it: dalpha and beta dalpha
    per edge and head on the scale of the dot product's terms, acc rows on theirs, gbits bit for
    bit over the destinations with an in-edge (the others' g is 1e3 larger), and the acc of
    ppgat_xgat_bwd_edges_g bit for bit (one accumulation in k_bwd_g)."""
    C = 256
    record = {}
    for p in (0.0, 0.2):
        for T, g in graphs.by_max.items():
            I = _stage_inputs(H, C, p, kind, graphs, g, cuda)
            v = hip_ops.XViews.of_graph(g)
            E = v.n_edges
            seed_buf = torch.tensor([SEED], dtype=torch.int64, device=cuda) if p > 0 else None
            hs, s_src, Gd = _dev(I.hs, cuda), _dev(I.s32, cuda), _dev(I.G, cuda)
            nstate = torch.empty(N, H, 4, device=cuda)
            launch.xgat_nstate(_dev(I.d32, cuda), _dev(I.m, cuda), _dev(I.inv_l, cuda), None, N, H, nstate)
            acc = torch.full((N, H * C), 7.0, device=cuda)
            dz = torch.full((E * H,), 7.0, device=cuda)
            pdal = torch.full((E * H,), 7.0, device=cuda)
            gbits = torch.zeros(C, dtype=torch.int32, device=cuda)
            launch.xgat_bwd_edges_gd_colmax(v.bwd_sched, v, 0, hs, s_src, nstate, Gd, acc, dz, pdal, gbits, H, C, SLOPE,
                                            p, SEED, seed_buf)
            fig = {}
            fig["dalpha"], z0 = _per_edge(dz.view(E, H), I.dal, I.dal_scale)
            fig["pdalpha"], fig["pdalpha_masked_absmax"] = _per_edge(pdal.view(E, H), I.beta * I.dal, I.beta * I.dal_scale)
            fig["acc_scaled_rows"], fig["acc_zero_scale_rows_absmax"] = ref.scaled_rows(acc, I.acc, I.acc_scale)
            print(json.dumps(fig))
            assert z0 == 0.0 and fig["dalpha"] <= TOL and fig["pdalpha"] <= TOL and fig["pdalpha_masked_absmax"] == 0.0, fig
            assert fig["acc_scaled_rows"] <= TOL and fig["acc_zero_scale_rows_absmax"] == 0.0, fig
            assert torch.equal(gbits.cpu(), I.gbits)
            # the reference's own dalpha (float64 hs) agrees with the one from the fp32 hs
            eid = g.csc_eid.cpu().long()
            assert _per_edge(I.want["dalpha"][eid].float(), I.dal, I.dal_scale)[0] <= 1e-6
            # the g-gathering pass: the same acc, bit for bit
            launch.xgat_nstate_set_d(nstate, _dev(I.D, cuda), N, H)
            acc2 = torch.full((N, H * C), 7.0, device=cuda)
            S = torch.zeros(N, 2 * H, device=cuda)
            dz2 = torch.empty(E * H, device=cuda)
            launch.xgat_bwd_edges_g(v.bwd_sched, v, 0, hs, s_src, nstate, Gd, acc2, S, dz2, H, C, SLOPE, p, SEED, seed_buf)
            assert torch.equal(acc2, acc)
            record[f"p{p}_max_edges{T}"] = fig
    write_report(f"xgat_edges_gd_{kind}_h{H}", record)


@pytest.mark.parametrize("kind", ["recipe", "sharp"])
@pytest.mark.parametrize("H", [4, 2])
def test_dz_pass(hip_ops, launch, graphs, cuda, H, kind):
    """ppgat_xgat_bwd_dz given fp32 dalpha and D: dz per edge on the scale alpha e'(z) (|mask dalpha|
    + |D|), ds_src per (source, head) on the sum of its edges' scales, exactly 0 for sources
    without an out-edge, and the right half of S [n_src, 2 H] untouched."""
    C = 256
    record = {}
    none = _dev(np.flatnonzero(graphs.outd == 0), cuda)
    for p in (0.0, 0.2):
        for T, g in graphs.by_max.items():
            I = _stage_inputs(H, C, p, kind, graphs, g, cuda)
            v = hip_ops.XViews.of_graph(g)
            E = v.n_edges
            seed_buf = torch.tensor([SEED], dtype=torch.int64, device=cuda) if p > 0 else None
            dal32 = I.dal.float()
            nstate = torch.empty(N, H, 4, device=cuda)
            launch.xgat_nstate(_dev(I.d32, cuda), _dev(I.m, cuda), _dev(I.inv_l, cuda), _dev(I.D, cuda), N, H, nstate)
            dz = dal32.to(cuda).reshape(E * H).contiguous()
            S = torch.full((N, 2 * H), 7.0, device=cuda)
            launch.xgat_bwd_dz(v.bwd_sched, v, 0, _dev(I.s32, cuda), nstate, dz, S, H, SLOPE, p, SEED, seed_buf)
            D = torch.from_numpy(I.D).double()[I.dst]
            want = I.a1 * (I.mk * dal32.double() - D)
            scale = I.a1 * ((I.mk * dal32.double()).abs() + D.abs())
            ds = torch.zeros(N, H, dtype=torch.float64).index_add_(0, I.ts, want)
            ds_scale = torch.zeros(N, H, dtype=torch.float64).index_add_(0, I.ts, scale)
            fig = {}
            fig["dz"], fig["dz_zero_scale_absmax"] = _per_edge(dz.view(E, H), want, scale)
            fig["ds_src_scaled"], fig["ds_src_zero_scale_absmax"] = ref.scaled_rows(
                S[:, :H].reshape(-1, 1), ds.reshape(-1, 1), ds_scale.reshape(-1))
            print(json.dumps(fig))
            assert fig["dz"] <= TOL and fig["dz_zero_scale_absmax"] == 0.0, fig
            assert fig["ds_src_scaled"] <= TOL and fig["ds_src_zero_scale_absmax"] == 0.0, fig
            assert none.numel() >= 100 + 22 and not S[none, :H].any()
            assert bool((S[:, H:] == 7.0).all())
            record[f"p{p}_max_edges{T}"] = fig
    write_report(f"xgat_dz_{kind}_h{H}", record)


@pytest.mark.parametrize("H,C", ref.CASES)
def test_weight_grads_from_given_products(launch, cuda, H, C):
    """ppgat_xgat_weight_grads given fp32 G = g^T agg and GV = S^T x: dW and datt against the
    formulas evaluated in float64 on those fp32 products."""
    P, want = _inputs(H, C), _reference(H, C, 0.2)
    Gm, GV = want["G_mat"].float(), want["GV"].float()
    W, a_s, a_d = (torch.from_numpy(P[k]) for k in ("W", "att_src", "att_dst"))
    dW = torch.empty(H * C, K, device=cuda)
    das, dad = torch.empty(H, C, device=cuda), torch.empty(H, C, device=cuda)
    launch.xgat_weight_grads(Gm.to(cuda), GV.to(cuda), W.to(cuda), a_s.to(cuda), a_d.to(cuda), H, C, dW, das, dad)
    G3, V = Gm.double().view(C, H, K).permute(1, 0, 2), GV.double()
    dW_want = G3 / H + a_s.double().unsqueeze(-1) * V[:H].unsqueeze(1) + a_d.double().unsqueeze(-1) * V[H:].unsqueeze(1)
    W3 = W.double().view(H, C, K)
    fig = {"dW": ref.rel(dW, dW_want.reshape(H * C, K)), "dW_rows": row_rel(dW, dW_want.reshape(H * C, K))[0],
           "datt_src": ref.rel(das, torch.einsum("hck,hk->hc", W3, V[:H])),
           "datt_dst": ref.rel(dad, torch.einsum("hck,hk->hc", W3, V[H:])),
           "dW_vs_layer_reference": ref.rel(dW, want["dW"])}
    print(json.dumps(fig))
    assert fig["dW"] <= TOL and fig["dW_rows"] <= TOL and fig["dW_vs_layer_reference"] <= TOL, fig
    assert fig["datt_src"] <= TOL_ATT and fig["datt_dst"] <= TOL_ATT, fig
    write_report(f"xgat_weight_grads_h{H}_c{C}", fig)


@pytest.mark.parametrize("H", [4, 2])
def test_prologue_and_epilogue_of_the_gt_passes(launch, cuda, H):
    """ppgat_xgat_bwd_prologue: {s_dst, m, inv_l} packed bit for bit and D = <gt, agg> per (row, head)
    on the scale of the dot product's terms, for n rows of a longer table; ppgat_xgat_bwd_epilogue:
    dx[:n_dst] += S[:, H:] A_dst on the scale of its terms, the rows from n_dst on untouched."""
    C = 256
    want = _reference(H, C, 0.2)
    gt, agg = want["gt"].float(), want["agg"].float()
    s_dst, m, inv_l = (want[k].float().to(cuda) for k in ("s_dst", "m", "inv_l"))
    D64 = (gt.double() * agg.double()).sum(-1)
    Dscale = (gt.double().abs() * agg.double().abs()).sum(-1)
    fig = {}
    for n in (5, N):
        ns = torch.full((N + 1, H, 4), 7.0, device=cuda)
        launch.xgat_bwd_prologue(gt.to(cuda), agg.to(cuda), s_dst, m, inv_l, n, K, H, ns)
        assert torch.equal(ns[:n, :, :3], torch.stack([s_dst, m, inv_l], -1)[:n]) and bool((ns[n:] == 7.0).all())
        fig[f"D_rows{n}"], z0 = _per_edge(ns[:n, :, 3], D64[:n], Dscale[:n])
        assert fig[f"D_rows{n}"] <= TOL and z0 == 0.0, fig   # rows without an in-edge: agg = 0, D exactly 0
    assert ref.rel(D64, want["D"]) <= 1e-6
    g = torch.Generator().manual_seed(H)
    dx0, S = torch.randn(N, K, generator=g), torch.randn(N, 2 * H, generator=g)
    A = want["A"].float()
    dx = dx0.to(cuda)
    launch.xgat_bwd_epilogue(S.to(cuda), A.to(cuda), N_DST, H, dx)
    add = S[:, H:].double() @ A[1].double()
    scale = dx0.double().abs() + S[:, H:].double().abs() @ A[1].double().abs()
    assert torch.equal(dx[N_DST:].cpu(), dx0[N_DST:])
    fig["epilogue"] = float(((dx[:N_DST].double().cpu() - (dx0.double() + add)[:N_DST]).abs() / scale[:N_DST]).max())
    print(json.dumps(fig))
    assert fig["epilogue"] <= TOL, fig
    write_report(f"xgat_prologue_epilogue_h{H}", fig)


# ---------------------------------------------------------------------------------------------
# the rectangular view (more source rows than destination rows)
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rect(hip_ops, graphs, cuda):
    """The ladder graph without the edges into rows >= N_DST, as the halo partition's views are
    built (dist.build_halo_graph): one CSR / CSC over all n_src rows, the forward schedule over the
    first n_dst row pointers, the backward's own / halo schedules over the two ranges of colptr."""
    ei = np.ascontiguousarray(graphs.ei[:, graphs.ei[1] < N_DST])
    E = ei.shape[1]
    assert int((ei[0] >= N_DST).sum()) > 500 and E < graphs.E
    ind = np.bincount(ei[1], minlength=N)
    out = {}
    for T in (256, 32):
        g = hip_ops.csr_build(_dev(ei, cuda), N, max_edges=T)
        sb = lambda ptr: hip_ops.schedule_build(ptr.contiguous(), E, T)
        v = hip_ops.XViews(N_DST, N, E, g.col, g.csr_eid, sb(g.rowptr[:N_DST + 1]), g.row, g.csc_eid, None, g.bwd_sched,
                           bwd_sched_own=sb(g.colptr[:N_DST + 1]), bwd_sched_halo=sb(g.colptr[N_DST:]),
                           csr2csc=hip_ops._csr2csc(g), rowptr=g.rowptr[:N_DST + 1].contiguous(), colptr=g.colptr)
        assert v.bwd_sched_own.n_items + v.bwd_sched_halo.n_items == v.bwd_sched.n_items
        assert v.bwd_sched_own.n_hub_items == v.bwd_sched.n_hub_items > 0
        d = 19  # the 512-edge hub in the first phase; the 513-, 700- and 4100-edge hubs in the second
        phases = [hip_ops.XPhase(0, d, sb(g.rowptr[:d + 1]), ((N_DST, 1203), (1203, N))),
                  hip_ops.XPhase(d, N_DST, sb(g.rowptr[d:N_DST + 1]))]
        assert phases[0].sched.n_hubs >= 1 and phases[1].sched.n_hubs >= 3
        out[T] = types.SimpleNamespace(g=g, v=v, phases=phases)
    return types.SimpleNamespace(ei=ei, E=E, ind=ind, by_max=out)


@functools.lru_cache(maxsize=None)
def _rect_reference(H: int, C: int, p: float):
    ei = ref.make_graph()
    ei = np.ascontiguousarray(ei[:, ei[1] < N_DST])
    P = dict(_inputs(H, C))
    P["G"] = np.array(P["G"])
    P["G"][N_DST:] = 0  # the layer has N_DST output rows
    return P, ref.formulas(P, ei, H, SLOPE, _mask(ei.shape[1], H, p))


@pytest.mark.parametrize("H,C", [(4, 256), (2, 256)])
def test_rectangular_view(hip_ops, rect, cuda, monkeypatch, H, C):
    """n_dst = 1000 < n_src = 1400: the forward in two phases equals the one-phase forward bit for
    bit (out, agg, m, inv_l, xbits); the backward with a halo hook equals the unsplit backward bit
    for bit in every formulation, and the hook receives dx[n_dst:], finished; both against float64."""
    monkeypatch.setenv("PPGAT_XGAT_AGG", "keep")
    record = {}
    for p in (0.0, 0.2):
        P, want = _rect_reference(H, C, p)
        x, W, a_s, a_d, bias = (_dev(P[k], cuda) for k in LEAVES)
        G = _dev(P["G"][:N_DST], cuda)
        for T, r in rect.by_max.items():
            fwd = lambda phases: hip_ops.xgat_forward(x, W, a_s, a_d, bias, r.v, H, C, SLOPE, p, SEED, phases=phases,
                                                      keep_agg=True)
            out1, s1 = fwd(None)
            out2, s2 = fwd(r.phases)
            assert torch.equal(out1, out2)
            for k in ("agg", "m", "inv_l", "xbits", "s_src", "s_dst"):
                assert torch.equal(s1[k], s2[k]), k
            srcs = np.unique(rect.ei[0])
            assert torch.equal(s1["xbits"].cpu(), torch.from_numpy(np.abs(P["x"][srcs]).max(0)).view(torch.int32))
            for mode in ("gd", "g", "gt"):
                monkeypatch.setenv("PPGAT_XGAT_GATHER", mode)
                assert hip_ops._xgat_gather_mode(C, H, N, N_DST, rect.E, K) == mode
                whole = hip_ops.xgat_backward(s1, G, True)
                seen = []
                split = hip_ops.xgat_backward(s2, G, True, halo_hook=lambda t: seen.append((t, t.clone())))
                assert all(torch.equal(a, b) for a, b in zip(whole, split)), mode
                (t, snap), = seen
                dx = split[0]
                assert t.data_ptr() == dx[N_DST:].data_ptr() and t.shape == (N - N_DST, K)
                assert torch.equal(snap, dx[N_DST:]) and bool(snap.any())
                fig = _check(_figures((out1,) + tuple(split), want))
                record[f"p{p}_max_edges{T}_{mode}"] = fig
    write_report(f"xgat_rect_h{H}_c{C}", record)
