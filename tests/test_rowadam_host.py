"""Row-sparse lazy Adam, the parts that need no GPU: the numpy reference against torch.optim.Adam,
the untouched rows, hip_ops.embedding_rows' gradient, the ABI's refusals (nothing launched), the
trainer's refusal and defaults -- CPU."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import _rowadam_ref as ref


def test_reference_with_every_row_touched_is_torch_adam():
    rng = np.random.default_rng(0)
    n, d = 40, 7
    p0 = rng.standard_normal((n, d))
    for wd in (0.0, 1e-4):
        mine = ref.LazyAdam(p0, lr=1e-3, weight_decay=wd)
        q = torch.tensor(p0, dtype=torch.float64, requires_grad=True)
        opt = torch.optim.Adam([q], lr=1e-3, weight_decay=wd)
        for _ in range(5):
            g = rng.standard_normal((n, d))
            q.grad = torch.tensor(g)
            opt.step()
            mine.step(np.arange(n), g)
        st = opt.state[q]
        for got, want in ((mine.p, q), (mine.m, st["exp_avg"]), (mine.v, st["exp_avg_sq"])):
            want = want.detach().numpy()
            assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
        assert mine.t == 5 == int(st["step"])


def test_reference_leaves_untouched_rows_bit_identical():
    rng = np.random.default_rng(1)
    n, d = 50, 5
    a = ref.LazyAdam(rng.standard_normal((n, d)), weight_decay=1e-4)
    a.step(np.arange(n), rng.standard_normal((n, d)))  # nonzero moments everywhere
    rows = np.sort(rng.choice(n, 17, replace=False))
    before = [x.copy() for x in (a.p, a.m, a.v)]
    a.step(rows, rng.standard_normal((17, d)))
    rest = np.setdiff1d(np.arange(n), rows)
    for b, x in zip(before, (a.p, a.m, a.v)):
        assert np.array_equal(b[rest].view(np.uint64), x[rest].view(np.uint64))
        assert (b[rows] != x[rows]).all()
    assert a.t == 2


def test_embedding_rows_gradient_is_row_sparse(pkg):
    g = torch.Generator().manual_seed(3)
    n, d = 30, 6
    w = torch.randn(n, d, generator=g, requires_grad=True)
    w2 = w.detach().clone().requires_grad_(True)
    up = torch.randn(9, d, generator=g)
    for idx in (torch.tensor([0, 3, 4, 9, 11, 17, 20, 28, 29]), torch.tensor([5, 2, 5, 29, 0, 2, 5, 7, 8])):
        w.grad = w2.grad = None
        out = pkg.hip_ops.embedding_rows(w, idx)
        assert torch.equal(out, w.detach().index_select(0, idx))
        (out * up).sum().backward()
        (w2.index_select(0, idx) * up).sum().backward()
        assert w.grad.is_sparse and w.grad.sparse_dim() == 1 and w.grad.shape == w.shape
        assert w.grad._values().shape == (9, d) and torch.equal(w.grad._indices()[0], idx)
        assert torch.equal(w.grad.to_dense(), w2.grad)
    with pytest.raises(RuntimeError, match="embedding_rows"):
        pkg.hip_ops.embedding_rows(w, torch.tensor([0, 1], dtype=torch.int32))


def test_abi_refusals_launch_nothing(pkg):
    lib = pkg._lib.load()
    assert "ppgat_adam_rows" in pkg._lib.SIGNATURES and len(pkg._lib.SIGNATURES["ppgat_adam_rows"][1]) == 16
    p = ctypes.c_void_p(256)  # never dereferenced: every call below is refused on the host or launches nothing
    #     param m  v  grad rows n_rows n_table dim  ss    bc2s b1   b2     eps   wd   flag  stream
    ok = [p, p, p, p, p, 10, 1000, 128, 1e-3, 1.0, 0.9, 0.999, 1e-8, 0.0, None, None]
    for pos in (0, 1, 2, 3, 4):
        a = list(ok)
        a[pos] = None
        assert lib.ppgat_adam_rows(*a) == 1 and b"null" in lib.ppgat_last_error(), pos
    for pos, val, rc in ((7, 0, 1), (7, -4, 1), (5, -1, 1), (6, -1, 1), (5, 1 << 31, 2), (6, 1 << 31, 2),
                         (5, 1 << 40, 2)):
        a = list(ok)
        a[pos] = val
        assert lib.ppgat_adam_rows(*a) == rc, (pos, val)
    for flag in (None, p):  # no row: OK, nothing launched (the pointers are not device memory)
        a = list(ok)
        a[5], a[14] = 0, flag
        assert lib.ppgat_adam_rows(*a) == 0
    with pytest.raises(NotImplementedError):
        a = list(ok)
        a[6] = 1 << 31
        pkg._lib.check(lib.ppgat_adam_rows(*a), "adam_rows")
    assert lib.ppgat_version() == 3


def test_optimizer_arguments(pkg):
    w = torch.nn.Parameter(torch.zeros(4, 4))
    with pytest.raises(ValueError, match="rows"):
        pkg.optim.Adam([w], rows="sorted")
    for mode in ("coalesce", "ascending"):
        opt = pkg.optim.Adam([w], rows=mode)
        assert opt.rows == mode
        opt.check_rows()  # no sparse step yet: nothing to read, nothing raised
    assert pkg.optim.Adam([w]).rows == "coalesce"


def test_trainer_refusal_and_defaults(pkg):
    train = importlib.import_module(pkg.__name__ + ".train")
    with pytest.raises(ValueError, match="sparse-adam"):
        train.main(["--synthetic", "cfg1", "--sparse-adam"])
    with pytest.raises(ValueError, match="sparse-adam"):
        train.main(["--synthetic", "cfg1", "--fanout", "5", "--sparse-adam"])
    base = ["--synthetic", "cfg1", "--fanout", "5", "--subgraph-batch", "4096", "--sparse-adam"]
    with pytest.raises(NotImplementedError, match="subgraph-batch"):  # what --subgraph-batch refuses stays refused
        train.main(base + ["--model-family", "lightgcn"])
    with pytest.raises(NotImplementedError, match="subgraph-batch"):
        train.main(base + ["--world-size", "2"])
    with pytest.raises(ValueError, match="resample-every"):
        train.main(base + ["--resample-every", "2"])
    args = train.build_parser().parse_args([])
    assert args.sparse_adam is False and args.subgraph_batch == 0
    assert train.build_parser().parse_args(["--sparse-adam"]).sparse_adam is True
    assert callable(train.check_sparse_adam)


def test_forward_subgraph_takes_the_flag(pkg):
    import inspect
    for fn in (pkg.forward_subgraph, pkg.PyGGAT.forward_subgraph, pkg.PyGGATv2.forward_subgraph,
               pkg.CustomGAT.forward_subgraph):
        assert inspect.signature(fn).parameters["sparse_grad"].default is False
