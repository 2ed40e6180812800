"""Full-size parity on the BASELINE configurations (GPU only, -m gpu).

The HIP path through the C ABI against the fp64 CPU oracle (oracle/gat_oracle.py) at the
sizes the bench runs:

* config 2 -- the whole statistics-matched U-I graph (192,403 users + 63,001 items,
  2,608,620 edge_index columns, max in-degree in the thousands, so every row class of the
  kernels runs: hub pieces, long rows, four-per-wave short rows).  PyGGAT (heads=1, C=128,
  L=2, train_gat_pyg.py:68-88) eval forward: final embeddings <= 1e-5 and serving top-20
  exact for 1,000 probe users; one training step (attention dropout 0.1 through the shared
  counter-hash mask, BPR over 200k triples, train_gat_pyg.py:307-323): Z and loss
  <= 1e-5, every parameter gradient <= 1e-5 (attention vectors and bias <= 1e-4).
* config 3 -- config 2 plus the I-I kNN relation (k=20) appended to edge_index: the same
  training-step checks.
* config 5 -- one GPU's share of the 200M-edge synthetic (1.25M users x 625k items, 25M
  columns, d=256, heads=4, scale 1/8): one GATConv(256, 256, heads=4) layer (lin 256->1024,
  train_gat_pyg.py:77) in train mode.  The fp64 oracle cannot hold [E, H, C] at this size
  in one piece, so ``oracle.pyg_gat_conv_chunked`` runs it by destination blocks (exact:
  softmax and aggregation are per destination) on the device in fp64: the output of every
  row, dx of every row, dW, datt_src, datt_dst and dbias; plus a bitwise repeat.

Tolerances: max-abs error / max-abs oracle value per tensor (as tests/test_gpu_parity.py),
and per row (``row_rel``: |a_i - b_i| / |b_i|) for the exported embeddings; the figures of
each run go to gpurun_out/parity/*.json.
"""
import importlib

import numpy as np
import pytest
import torch

from conftest import assert_kink_ties, check_att_dst, dx_rows, kink_report, kink_sides, row_rel, write_report

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(170)]


def rel(a, b):
    a = a.detach().double().cpu() if torch.is_tensor(a) else torch.from_numpy(np.asarray(a, np.float64))
    b = b.detach().double().cpu() if torch.is_tensor(b) else torch.from_numpy(np.asarray(b, np.float64))
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _conv_mod():
    return importlib.import_module("plotpointe-gat-recommendation_amd.conv")


def _ops():
    return importlib.import_module("plotpointe-gat-recommendation_amd.hip_ops")


def _graph():  # where KINK_TAP lives (module state is not re-exported by hip_ops)
    return importlib.import_module("plotpointe-gat-recommendation_amd.ops_graph")


@pytest.fixture(scope="module")
def cfg2(pkg):
    d = pkg.data
    g = d.synthetic_ui_graph(seed=42)
    feats = d.synthetic_item_features(g.n_items, 128, seed=42)
    u, i, j = d.sample_bpr_numpy(g.user_ptr, g.user_items, g.n_items, 200_000, seed=42)
    return g, g.edge_index_numpy(), feats, (u, i, j)


def _model(pkg, g, heads=1, p=0.1):
    torch.manual_seed(42)
    m = pkg.PyGGAT(g.n_users, g.n_items, item_feat_dim=128, hidden=128, layers=2, heads=heads, attn_dropout=p)
    with torch.no_grad():
        for c in m.convs:  # a non-zero bias so its gradient and the "out = bias" rows are checked
            c.bias.uniform_(-0.1, 0.1)
    return m


def _train_step_check(pkg, oracle, cuda, g, ei_np, feats_np, triples, name):
    m = _model(pkg, g).to(cuda).train()
    ei = torch.from_numpy(ei_np)
    feats = torch.from_numpy(feats_np)
    tu, ti, tj = (torch.from_numpy(a) for a in triples)
    # device step: the two layers' dropout seeds are drawn from torch's CPU generator
    torch.manual_seed(777)
    _graph().KINK_TAP = []  # the LeakyReLU side of every logit in this forward (for the oracle)
    try:
        Z = m(feats.to(cuda), ei.to(cuda))
        sides = kink_sides(_graph().KINK_TAP, ei_np.shape[1], 1, 2)
    finally:
        _graph().KINK_TAP = None
    loss = pkg.bpr_loss(Z, g.n_users, tu.to(cuda), ti.to(cuda), tj.to(cuda))
    loss.backward()
    torch.cuda.synchronize()
    torch.manual_seed(777)
    seeds = [_conv_mod()._dropout_seed() for _ in range(2)]
    P = {k: v.detach().double().to(cuda).requires_grad_(True) for k, v in m.named_parameters()}
    kst = []
    Zr = oracle.pyg_gat_model(P, feats.double().to(cuda), ei.to(cuda), 2, 1, dropout_p=0.1, seeds=seeds,
                              kink_pos=sides, kink_stats=kst)
    lr_t = oracle.bpr_loss(Zr, g.n_users, *(torch.from_numpy(a).to(cuda) for a in triples))
    lr_t.backward()
    lr, Zr = float(lr_t), Zr.detach().cpu()
    grads = {k: v.grad.cpu() for k, v in P.items()}
    r_items, worst, zmax = row_rel(Z[g.n_users:], Zr[g.n_users:])
    r_users = row_rel(Z[:g.n_users], Zr[:g.n_users])[0]
    write_report(name, {"Z_rel": rel(Z, Zr), "item_row_rel_max": r_items, "item_worst_row": worst,
                        "item_zero_rows_max_abs": zmax, "user_row_rel_max": r_users,
                        "loss_rel": abs(loss.item() - lr) / abs(lr),
                        "kink_ties_per_layer": kink_report(kst),
                        "grad_rel": {k: rel(v.grad, grads[k]) for k, v in m.named_parameters()},
                        "oracle": "fp64 torch ops on the device, LeakyReLU sides as the kernels took them"})
    assert_kink_ties(kst)  # the kernels' side differs from the fp64 sign only at fp32 ties of the logit
    assert rel(Z, Zr) <= 1e-5
    assert r_items <= 1e-5 and r_users <= 1e-5, (r_items, worst, r_users)
    assert abs(loss.item() - lr) <= 1e-5 * abs(lr)
    for k, v in m.named_parameters():
        tol = 1e-5 if v.dim() == 2 else 1e-4
        ref = grads[k]
        if k.endswith("att_dst"):
            err = float((v.grad.detach().double().cpu() - ref).abs().max())
            check_att_dst(err, ref, grads[k.replace("att_dst", "att_src")], tol)
            continue
        assert rel(v.grad, ref) <= tol, (k, rel(v.grad, ref))




def test_cfg2_full_eval_embeddings_and_top20(pkg, oracle, cuda, cfg2):
    g, ei_np, feats_np, _ = cfg2
    assert ei_np.shape[1] > 2_500_000
    deg = np.bincount(ei_np[1], minlength=g.n_nodes)
    assert deg.max() > 256  # hub rows (split into pieces) are on the path
    m = _model(pkg, g).to(cuda).eval()
    ei = torch.from_numpy(ei_np)
    with torch.no_grad():
        Z = m(torch.from_numpy(feats_np).to(cuda), ei.to(cuda)).cpu()
        P = {k: v.detach().double().cpu() for k, v in m.named_parameters()}
        Zr = oracle.pyg_gat_model(P, torch.from_numpy(feats_np).double(), ei, 2, 1)
    assert rel(Z, Zr) <= 1e-5
    assert rel(Z[g.n_users:], Zr[g.n_users:]) <= 1e-5  # the exported item embeddings
    # per exported item row (a small row is held to its own norm, not the largest row's)
    r_items, worst, zmax = row_rel(Z[g.n_users:], Zr[g.n_users:])
    # top-20 items for 1,000 probe users: argsort(I @ U[u]), fp64 scores of
    # each side's fp32 rows, ties by item index; a differing position is a near-tie only if
    # the oracle's two scores there differ by < 1e-6 * max|score|
    Za = Z.double().numpy()
    Zb = Zr.float().double().numpy()
    nu = g.n_users
    probes = np.random.default_rng(5).choice(nu, 1000, replace=False)
    Sa = Za[nu:] @ Za[probes].T
    Sb = Zb[nu:] @ Zb[probes].T
    mismatched = near = 0
    for t in range(len(probes)):
        a_idx, b_idx = oracle.topk_stable(Sa[:, t], 20), oracle.topk_stable(Sb[:, t], 20)
        if np.array_equal(a_idx, b_idx):
            continue
        diff = a_idx != b_idx
        if np.all(np.abs(Sb[a_idx[diff], t] - Sb[b_idx[diff], t]) < 1e-6 * np.abs(Sb[:, t]).max()):
            near += 1
        else:
            mismatched += 1
    write_report("cfg2_eval_forward", {
        "Z_rel": rel(Z, Zr), "item_row_rel_max": r_items, "item_worst_row": worst, "item_zero_rows_max_abs": zmax,
        "user_row_rel_max": row_rel(Z[:nu], Zr[:nu])[0],
        "top20": {"probe_users": 1000, "exact": 1000 - near - mismatched, "near_tie": near,
                  "mismatched": mismatched, "near_tie_rule": "oracle score gap < 1e-6 * max|score|"}})
    assert r_items <= 1e-5, (r_items, worst)
    assert mismatched == 0 and near == 0


def test_cfg2_full_train_step(pkg, oracle, cuda, cfg2):
    g, ei_np, feats_np, triples = cfg2
    _train_step_check(pkg, oracle, cuda, g, ei_np, feats_np, triples, "cfg2_train_step")


def test_cfg3_full_train_step(pkg, oracle, cuda, cfg2):
    g, ei_np, feats_np, triples = cfg2
    rows, cols, _ = pkg.data.synthetic_ii_edges(g, k=20, seed=42)
    ei3 = np.concatenate([ei_np, pkg.data.ii_edge_columns(g.n_users, rows, cols)], 1)
    assert ei3.shape[1] - ei_np.shape[1] > 1_000_000
    _train_step_check(pkg, oracle, cuda, g, ei3, feats_np, triples, "cfg3_train_step")


DX_ROW_TOL = 1e-5  # per row, relative to |message term| + |attention term| (conftest.dx_rows)


# ---------------------------------------------------------------------------
# config 5: one GPU's share, d=256, heads=4, the whole layer against a chunked fp64 oracle
# ---------------------------------------------------------------------------
@pytest.mark.timeout(400)
def test_cfg5_share_layer_full_gradients(pkg, oracle, cuda):
    """GATConv(256, 256, heads=4) (train_gat_pyg.py:77, lin 256 -> 1024) in train mode on one
    GPU's share of the 200M-edge synthetic (25M edges): output, dx of every row, dW, datt_src,
    datt_dst and dbias against the exact chunked fp64 oracle; plus a bitwise repeat."""
    d = pkg.data
    H, C = 4, 256
    g = d.synthetic_scaling_graph(1 / 8, seed=42)
    ei_np = g.edge_index_numpy()
    N, E = g.n_nodes, ei_np.shape[1]
    assert E == 25_000_000 and N == 1_875_000
    rng = np.random.default_rng(0)
    x = torch.from_numpy(rng.standard_normal((N, C), dtype=np.float32))
    Gup = torch.from_numpy(rng.standard_normal((N, C), dtype=np.float32))
    torch.manual_seed(9)
    conv = pkg.GATConv(C, C, heads=H, dropout=0.1, add_self_loops=False, concat=False)
    with torch.no_grad():
        conv.bias.uniform_(-0.1, 0.1)
    conv = conv.to(cuda).train()
    cm = _conv_mod()
    orig = cm._dropout_seed
    cm._dropout_seed = lambda: 424242
    names = ("out", "dx", "lin.weight", "att_src", "att_dst", "bias")
    try:
        ei = torch.from_numpy(ei_np).to(cuda)
        xd = x.to(cuda).requires_grad_(True)
        Gd = Gup.to(cuda)
        _graph().KINK_TAP = []
        try:
            out = conv(xd, ei)
            sides = kink_sides(_graph().KINK_TAP, E, H, 1)
        finally:
            _graph().KINK_TAP = None
        (out * Gd).sum().backward()
        torch.cuda.synchronize()
        res1 = (out.detach().clone(), xd.grad.clone(), conv.lin.weight.grad.clone(), conv.att_src.grad.clone(),
                conv.att_dst.grad.clone(), conv.bias.grad.clone())
        # bitwise repeat (same mask seed)
        xd.grad = None
        conv.zero_grad(set_to_none=True)
        out2 = conv(xd, ei)
        (out2 * Gd).sum().backward()
        res2 = (out2.detach(), xd.grad, conv.lin.weight.grad, conv.att_src.grad, conv.att_dst.grad, conv.bias.grad)
        for n, a, b in zip(names, res1, res2):
            assert torch.equal(a, b), n
    finally:
        cm._dropout_seed = orig
    del out, out2, res2, xd
    torch.cuda.empty_cache()
    P = {k: v.detach() for k, v in conv.named_parameters()}
    kst = []
    out_r, dx_r, grads, dxm_r = oracle.pyg_gat_conv_chunked(P, x.to(cuda), ei, Gd, H, 0.1, 424242,
                                                            kink_pos=sides[0].to(cuda), kink_stats=kst, dx_message=True)
    refs = (out_r, dx_r, grads["lin.weight"], grads["att_src"], grads["att_dst"], grads["bias"])
    errs = {n: rel(a, b) for n, a, b in zip(names, res1, refs)}
    U = oracle.pyg_dx_attention_scale(P, x.to(cuda), ei, Gd, H, 0.1, 424242)
    cond_dx, dx_rep = dx_rows(res1[1], dx_r, dxm_r, U, ei)
    del U
    rows = {"out": row_rel(res1[0], refs[0])[0], "dx": dx_rep["plain_row_rel_max"], "dx_cond": cond_dx}
    ties = sum(n for n, _, _ in kst)
    worst_tie = max((r for _, r, _ in kst), default=0.0)
    worst_bound = max((rb for _, _, rb in kst), default=0.0)
    write_report("cfg5_share_layer", {"edges": E, "nodes": N, "heads": H, "channels": C, "rel": errs,
                                      "row_rel_max": rows, "dx_rows": dx_rep, "kink_ties": ties,
                                      "kink_tie_max_abs_z_rel": worst_tie,
                                      "kink_tie_max_abs_z_over_fp32_bound": worst_bound,
                                      "oracle": "chunked fp64 pyg_gat_conv on the device, LeakyReLU sides as the "
                                                "kernels took them"})
    assert_kink_ties(kst)
    tol = {"out": 1e-5, "dx": 1e-5, "lin.weight": 1e-5, "att_src": 1e-4, "att_dst": 1e-4, "bias": 1e-5}
    for n in names:
        assert errs[n] <= tol[n], (n, errs[n])
    # every row of dx within 1e-5 of the scale of its terms (conftest.dx_rows: a row whose
    # message and attention terms cancel is judged on the terms, not on their small sum)
    assert rows["out"] <= 1e-5 and cond_dx <= DX_ROW_TOL, dx_rep
