"""Row-sparse lazy Adam on the GPU (csrc/ppgat_gemm.hip k_adam_rows, include/ppgat.h ppgat_adam_rows,
optim.Adam with sparse gradients, hip_ops.embedding_rows, model.forward_subgraph(sparse_grad=True),
train.py --sparse-adam): the row step equals the dense kernel on compact copies bit for bit, rows it
does not name and the guards around the tables keep their bits, the trajectory follows the fp64
reference, contract violations raise a flag and never leave the tables, the model-level step equals
the dense optimiser's after step one, the trainer runs."""
import copy
import ctypes
import importlib
import json
import math

import numpy as np
import pytest
import torch

import _rowadam_ref as ref
import _subgraph_ref as sref

pytestmark = pytest.mark.gpu

N_ROWS = 1000
GUARD, SENT = 64, -7.5
LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8
DIMS = [1, 3, 4, 32, 100, 128, 260]


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _rel(a, b):
    a = a.detach().double().cpu()
    b = torch.as_tensor(b).double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


class Guarded:
    """A [n, d] table inside its own allocation: GUARD sentinel floats in front, GUARD behind
    (``shift`` floats more in front: shift = 1 starts the table 4 bytes off a 16-byte boundary)."""

    def __init__(self, values: torch.Tensor, cuda, shift: int = 0):
        n, d = values.shape
        self.flat = torch.full((GUARD + shift + n * d + GUARD,), SENT, dtype=torch.float32, device=cuda)
        self.lo = GUARD + shift
        self.t = self.flat[self.lo:self.lo + n * d].view(n, d)
        self.t.copy_(values)
        assert self.t.data_ptr() % 16 == (4 * shift) % 16

    def guards_intact(self) -> bool:
        return bool((self.flat[:self.lo] == SENT).all() and (self.flat[self.lo + self.t.numel():] == SENT).all())


def _row_sets():
    rng = np.random.default_rng(7)
    return {"empty": np.zeros(0, np.int64), "first": np.array([0]), "last": np.array([N_ROWS - 1]),
            "all": np.arange(N_ROWS), "random37": np.sort(rng.choice(N_ROWS, 37, replace=False)),
            "first16": np.arange(16)}


def _step_consts(t: int):
    return LR / (1.0 - B1 ** t), math.sqrt(1.0 - B2 ** t)


def _rows_launch(pkg, P, M, V, G, rows, wd, flag=None, t=3):
    """ppgat_adam_rows through ctypes; an empty row set still hands over valid pointers."""
    lib = pkg._lib.load()
    ss, bc = _step_consts(t)
    k = rows.numel()
    G = G if k else G.new_zeros((1, P.size(1)))
    rows_p = rows if k else rows.new_zeros(1)
    pkg._lib.check(lib.ppgat_adam_rows(P.data_ptr(), M.data_ptr(), V.data_ptr(), G.data_ptr(), rows_p.data_ptr(), k,
                                       P.size(0), P.size(1), ss, bc, B1, B2, EPS, wd,
                                       None if flag is None else flag.data_ptr(),
                                       pkg._lib.stream_handle(P.device)), "adam_rows")


def _dense_launch(pkg, p, g, m, v, wd, t=3):
    """The existing dense ppgat_adam_step on one tensor, in place."""
    lib = pkg._lib.load()
    ss, bc = _step_consts(t)
    arr = lambda x: (ctypes.c_void_p * 1)(x.data_ptr())  # noqa: E731
    pkg._lib.check(lib.ppgat_adam_step(1, arr(p), arr(g), arr(m), arr(v), (ctypes.c_int64 * 1)(p.numel()),
                                       (ctypes.c_float * 1)(ss), (ctypes.c_float * 1)(bc), B1, B2, EPS, wd,
                                       pkg._lib.stream_handle(p.device)), "adam_step")


def _initial(d: int, seed: int = 0):
    g = torch.Generator().manual_seed(100 + d + seed)
    p0 = torch.randn(N_ROWS, d, generator=g)
    m0 = 0.1 * torch.randn(N_ROWS, d, generator=g)
    v0 = 0.01 * torch.rand(N_ROWS, d, generator=g)
    grad = torch.randn(N_ROWS, d, generator=g)
    return p0, m0, v0, grad


# ---- the kernel against the dense kernel ---------------------------------------------------------
@pytest.mark.parametrize("d", DIMS)
def test_row_step_equals_the_dense_kernel_on_compact_copies(pkg, cuda, d):
    """Reference: the dense ppgat_adam_step on compact copies p[R], g, m[R], v[R].  The dense kernel
    itself rounds in two ways: the compiler contracts adam_elem's multiply-adds differently in
    k_adam's float4 path (m = fma(b1, m, (1-b1) g)) and in its scalar tail (m = b1 m + (1-b1) g,
    no fma), so no single arithmetic equals it bit for bit on a compact copy whose element count
    is not a multiple of four (one row of d = 1 or 3), and the dense kernel's bits stay as they
    are.  Hence: bit for bit on every element the dense kernel took through its float4 path
    (all of them when d % 4 == 0), and test_adam_matches_torch's 1e-6 relative on the whole."""
    p0, m0, v0, grad = _initial(d)
    for wd in (0.0, 1e-4):
        for name, rows_np in _row_sets().items():
            rows = torch.from_numpy(rows_np).to(cuda)
            G = grad[:rows.numel()].to(cuda).contiguous()
            runs = []
            for _ in range(2):  # twice from the same state: the same bits
                P, M, V = (Guarded(x, cuda) for x in (p0, m0, v0))
                flag = torch.zeros(1, dtype=torch.int32, device=cuda)
                _rows_launch(pkg, P.t, M.t, V.t, G, rows, wd, flag)
                torch.cuda.synchronize()
                assert int(flag) == 0, (name, wd)
                assert P.guards_intact() and M.guards_intact() and V.guards_intact(), (name, wd)
                runs.append((P.t.clone(), M.t.clone(), V.t.clone()))
            for a, b in zip(*runs):
                assert _same_bits(a, b), (name, wd)
            rest = torch.ones(N_ROWS, dtype=torch.bool, device=cuda)
            rest[rows] = False
            want = [x.to(cuda).index_select(0, rows).contiguous() for x in (p0, m0, v0)]
            if rows.numel():
                _dense_launch(pkg, want[0], G, want[1], want[2], wd)
            for got, w, x0, what in zip(runs[0], want, (p0, m0, v0), "pmv"):
                a, b = got.index_select(0, rows).reshape(-1), w.reshape(-1)
                nv = a.numel() // 4 * 4  # what k_adam ran through its float4 path on the compact copy
                assert _same_bits(a[:nv], b[:nv]), (name, wd, what)
                if a.numel():
                    assert _rel(a, b.cpu()) <= 1e-6, (name, wd, what)
                assert _same_bits(got[rest], x0.to(cuda)[rest]), (name, wd, what)
            if rows.numel():
                assert not _same_bits(runs[0][0].index_select(0, rows), p0.to(cuda).index_select(0, rows))


def test_misaligned_table_takes_the_scalar_path_and_gives_the_same_values(pkg, cuda):
    d = 128
    p0, m0, v0, grad = _initial(d)
    rows = torch.from_numpy(_row_sets()["random37"]).to(cuda)
    G = grad[:37].to(cuda).contiguous()
    out = []
    for shift in (0, 1):
        P, M, V = Guarded(p0, cuda, shift), Guarded(m0, cuda), Guarded(v0, cuda)
        _rows_launch(pkg, P.t, M.t, V.t, G, rows, 1e-4)
        torch.cuda.synchronize()
        assert P.guards_intact() and M.guards_intact() and V.guards_intact()
        out.append((P.t.clone(), M.t.clone(), V.t.clone()))
    for a, b in zip(*out):
        assert _same_bits(a, b)
    assert not _same_bits(out[0][0], p0.to(cuda))


# ---- the optimiser ------------------------------------------------------------------------------
def _sparse(rows, vals, shape):
    return torch.sparse_coo_tensor(rows[None], vals, shape)


@pytest.mark.parametrize("d", [3, 32])
def test_trajectory_follows_the_reference(pkg, cuda, d):
    """Five steps, a different row set each, real sparse gradients, rows="ascending"."""
    rng = np.random.default_rng(11)
    p0 = torch.randn(N_ROWS, d, generator=torch.Generator().manual_seed(2))
    p = p0.to(cuda).requires_grad_(True)
    opt = pkg.optim.Adam([p], lr=LR, weight_decay=1e-4, rows="ascending")
    want = ref.LazyAdam(p0.numpy(), lr=LR, betas=(B1, B2), eps=EPS, weight_decay=1e-4)
    sizes = [37, N_ROWS, 1, 400, 16]
    for k in sizes:
        rows = np.sort(rng.choice(N_ROWS, k, replace=False))
        g = rng.standard_normal((k, d)).astype(np.float32)
        p.grad = _sparse(torch.from_numpy(rows).to(cuda), torch.from_numpy(g).to(cuda), p.shape)
        assert k < 2 or not p.grad.is_coalesced()  # as autograd hands them over: not flagged
        opt.step()
        want.step(rows, g)
    opt.check_rows()
    st = opt.state[p]
    e_p, e_v = _rel(p, want.p), _rel(st["exp_avg_sq"], want.v)
    print(f"d={d}: p {e_p:.3e}, exp_avg_sq {e_v:.3e}, exp_avg {_rel(st['exp_avg'], want.m):.3e} (bound 1e-6)")
    assert e_p <= 1e-6 and e_v <= 1e-6
    assert float(st["step"]) == 5.0 and set(st) == {"step", "exp_avg", "exp_avg_sq"}
    o2 = torch.optim.Adam([p], lr=LR, weight_decay=1e-4)
    o2.load_state_dict(opt.state_dict())
    assert float(o2.state[p]["step"]) == 5.0 and torch.equal(o2.state[p]["exp_avg"], st["exp_avg"])


def test_coalesce_mode_equals_ascending_on_the_coalesced_form(pkg, cuda, monkeypatch):
    d = 32
    g = torch.Generator().manual_seed(4)
    p0 = torch.randn(N_ROWS, d, generator=g)
    idx = torch.randint(0, 200, (300,), generator=g)  # shuffled, with repeats
    assert idx.unique().numel() < idx.numel()
    vals = torch.randn(300, d, generator=g)
    grad = _sparse(idx.to(cuda), vals.to(cuda), p0.shape)
    co = grad.coalesce()
    calls = []
    coalesce = torch.Tensor.coalesce
    monkeypatch.setattr(torch.Tensor, "coalesce", lambda self: calls.append(1) or coalesce(self))
    a = p0.to(cuda).requires_grad_(True)
    b = p0.to(cuda).requires_grad_(True)
    oa = pkg.optim.Adam([a], lr=LR, weight_decay=1e-4)  # rows="coalesce"
    ob = pkg.optim.Adam([b], lr=LR, weight_decay=1e-4, rows="ascending")
    a.grad = grad
    oa.step()
    assert len(calls) == 1
    b.grad = _sparse(co._indices()[0], co._values(), p0.shape)  # the coalesced form, not flagged
    assert not b.grad.is_coalesced()
    ob.step()
    assert len(calls) == 1
    a.grad = co  # flagged coalesced: taken as it is
    assert co.is_coalesced()
    oa.step()
    assert len(calls) == 1
    b.grad = _sparse(co._indices()[0], co._values(), p0.shape)
    ob.step()
    oa.check_rows()
    ob.check_rows()
    assert _same_bits(a, b)
    for k in ("exp_avg", "exp_avg_sq"):
        assert _same_bits(oa.state[a][k], ob.state[b][k])
    assert float(oa.state[a]["step"]) == 2.0
    assert not _same_bits(a, p0.to(cuda))


def _guarded_optimizer(pkg, cuda, d=32):
    p0, m0, v0, grad = _initial(d)
    P, M, V = (Guarded(x, cuda) for x in (p0, m0, v0))
    p = P.t.requires_grad_(True)
    opt = pkg.optim.Adam([p], lr=LR, weight_decay=1e-4, rows="ascending")
    opt.state[p] = {"step": torch.tensor(2.0), "exp_avg": M.t, "exp_avg_sq": V.t}
    return p, opt, (P, M, V), p0.to(cuda), grad.to(cuda)


@pytest.mark.parametrize("rows,word,other", [([5, 17, N_ROWS], "range", "order"), ([-1, 3, 9], "range", "order"),
                                            ([3, 7, 7, 20], "order", "range"), ([3, 9, 8, 20], "order", "range")],
                         ids=["past-the-end", "negative", "repeated", "descending"])
def test_contract_violations_raise_the_flag_and_stay_in_bounds(pkg, cuda, rows, word, other):
    p, opt, tables, p0, grad = _guarded_optimizer(pkg, cuda)
    rows_t = torch.tensor(rows, device=cuda)
    p.grad = _sparse(rows_t, grad[:len(rows)].contiguous(), p.shape)
    opt.step()
    torch.cuda.synchronize()
    assert all(t.guards_intact() for t in tables)
    rest = torch.ones(N_ROWS, dtype=torch.bool, device=cuda)
    rest[rows_t[(rows_t >= 0) & (rows_t < N_ROWS)]] = False
    assert _same_bits(p.detach()[rest], p0[rest])  # only named rows were written
    with pytest.raises(RuntimeError, match=word) as exc:
        opt.check_rows()
    assert other not in str(exc.value)
    opt.check_rows()  # the flag is clear again
    ok = torch.tensor([2, 4, 900], device=cuda)
    p.grad = _sparse(ok, grad[:3].contiguous(), p.shape)
    opt.step()
    opt.check_rows()
    assert all(t.guards_intact() for t in tables) and float(opt.state[p]["step"]) == 4.0


def test_capturable_refuses_sparse_and_dense_gradients_are_untouched(pkg, cuda):
    g = torch.Generator().manual_seed(9)
    w0, e0 = torch.randn(50, 8, generator=g), torch.randn(N_ROWS, 8, generator=g)
    gw, ge = torch.randn(50, 8, generator=g).to(cuda), torch.randn(5, 8, generator=g).to(cuda)
    rows = torch.tensor([1, 2, 30, 500, 999], device=cuda)
    w, e = w0.to(cuda).requires_grad_(True), e0.to(cuda).requires_grad_(True)
    w2 = w0.to(cuda).requires_grad_(True)
    both, dense = pkg.optim.Adam([w, e], lr=LR), pkg.optim.Adam([w2], lr=LR)
    w.grad, w2.grad, e.grad = gw.clone(), gw.clone(), _sparse(rows, ge, e.shape)
    both.step()
    dense.step()
    both.check_rows()
    assert _same_bits(w, w2) and not _same_bits(w, w0.to(cuda))  # the dense tensor of a mixed step: the dense launch
    changed = (_bits(e) != _bits(e0.to(cuda))).any(dim=1)
    assert changed.nonzero().flatten().tolist() == rows.tolist()
    cap = pkg.optim.Adam([e], lr=LR, capturable=True)
    with pytest.raises(NotImplementedError, match="capturable"):
        cap.step()


# ---- model level --------------------------------------------------------------------------------
FEAT, HIDDEN = 32, 32


def _batch(rng, s):
    u = rng.integers(0, 2900, s)
    i, j = rng.integers(0, 1400, s), rng.integers(0, 1400, s)
    return u, i, j


def _bpr_step(pkg, model, opt, feats, ei, g, batch, seed, sparse_grad, cuda):
    u, i, j = batch
    s = len(u)
    seeds = torch.from_numpy(np.concatenate([u, sref.N_USERS + i, sref.N_USERS + j])).to(cuda)
    sub = pkg.sample_subgraph(ei, sref.N, seeds, 2, 7, seed, n_users=sref.N_USERS, graph=g)
    nus = sub.n_users_s
    ul, il = sub.seed_local[:s].contiguous(), sub.seed_local[s:] - nus
    Z = model.forward_subgraph(feats, sub, sparse_grad=sparse_grad)
    lo = pkg.bpr_loss(Z, nus, ul, il[:s].contiguous(), il[s:].contiguous(), "bpr")
    opt.zero_grad()
    lo.backward()
    assert model.user_emb.weight.grad.is_sparse == sparse_grad
    opt.step()
    return sub.n_id[:nus]


def test_model_step_equals_the_dense_optimiser_after_step_one(pkg, cuda):
    ei = torch.from_numpy(sref.graph(7)).to(cuda)
    cache = pkg.hip_ops.graph_cache
    cache.clear()
    g = pkg.hip_ops.csr_build(ei, sref.N)
    torch.manual_seed(5)
    ma = pkg.PyGGAT(sref.N_USERS, sref.N_ITEMS, FEAT, HIDDEN, 2, 2, 0.0).to(cuda).train()
    mb = copy.deepcopy(ma)
    init = ma.user_emb.weight.detach().clone()
    feats = torch.randn(sref.N_ITEMS, FEAT, device=cuda)
    oa = pkg.optim.Adam(ma.parameters(), lr=LR, weight_decay=0.0, rows="ascending")
    ob = pkg.optim.Adam(mb.parameters(), lr=LR, weight_decay=0.0)
    rng = np.random.default_rng(21)
    b1, b2 = _batch(rng, 64), _batch(rng, 64)
    ua = _bpr_step(pkg, ma, oa, feats, ei, g, b1, 42, True, cuda)
    ub = _bpr_step(pkg, mb, ob, feats, ei, g, b1, 42, False, cuda)
    oa.check_rows()
    assert torch.equal(ua, ub) and 0 < ua.numel() < sref.N_USERS
    for (ka, pa), (kb, pb) in zip(ma.named_parameters(), mb.named_parameters()):
        assert ka == kb and _same_bits(pa, pb), ka
        assert pa.grad is not None and pb.grad is not None, ka
        sa, sb = oa.state[pa], ob.state[pb]
        assert float(sa["step"]) == float(sb["step"]) == 1.0
        for k in ("exp_avg", "exp_avg_sq"):
            assert _same_bits(sa[k], sb[k]), (ka, k)
    touched1 = torch.zeros(sref.N_USERS, dtype=torch.bool, device=cuda)
    touched1[ua] = True
    assert not _same_bits(ma.user_emb.weight[touched1], init[touched1])
    # step two on another batch: the two optimisers part ways on purpose (the dense one coasts rows
    # of batch one on their momentum); the lazy one has not touched what neither batch named
    u2 = _bpr_step(pkg, ma, oa, feats, ei, g, b2, 43, True, cuda)
    _bpr_step(pkg, mb, ob, feats, ei, g, b2, 43, False, cuda)
    oa.check_rows()
    touched = touched1.clone()
    touched[u2] = True
    assert 0 < int((~touched).sum()) and int((touched & ~touched1).sum()) > 0
    wa, wb = ma.user_emb.weight.detach(), mb.user_emb.weight.detach()
    assert torch.isfinite(wa[touched]).all() and torch.isfinite(wb[touched]).all()
    assert _same_bits(wa[~touched], init[~touched])
    for k in ("exp_avg", "exp_avg_sq"):
        assert not oa.state[ma.user_emb.weight][k][~touched].any()
    cache.clear()


# ---- trainer ------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [[], ["--loss", "softmax"]], ids=["bpr", "softmax"])
def test_trainer(pkg, cuda, tmp_path, capsys, monkeypatch, extra):
    train = importlib.import_module(pkg.__name__ + ".train")
    seen, checks = [], []
    evaluate = train.evaluate
    monkeypatch.setattr(train, "evaluate", lambda args, model, cfg, feats, edge_index, *a, **k:
                        seen.append(int(edge_index.size(1))) or evaluate(args, model, cfg, feats, edge_index, *a, **k))
    check_rows = pkg.optim.Adam.check_rows
    monkeypatch.setattr(pkg.optim.Adam, "check_rows", lambda self: checks.append(1) or check_rows(self))
    capsys.readouterr()
    out = train.main(["--synthetic", "cfg1", "--epochs", "2", "--fanout", "5", "--subgraph-batch", "4096",
                      "--sparse-adam", "--eval-neg-k", "100", "--device-eval", "--fast-sampler", "--structured-logs",
                      "--models-prefix", str(tmp_path)] + extra)
    log = capsys.readouterr().out
    ends = [e for e in (json.loads(ln) for ln in log.splitlines() if ln.startswith("{")) if e["event"] == "epoch_end"]
    assert len(ends) == 2 and all(e["batches"] > 1 for e in ends)
    assert len(checks) == 2  # once per epoch, and it did not raise
    assert len(seen) == 3 and seen == [seen[0]] * 3  # two validations and the test, all on the whole graph
    assert list((tmp_path / "checkpoints").glob("*.pt"))
    vals = list(out["test"].values()) + list(out["val"].values()) + [e["loss"] for e in ends]
    assert vals and all(np.isfinite(v) for v in vals), out
    assert "--sparse-adam" in out["notes"] and "weight decay" in out["notes"] and "momentum" in out["notes"]
