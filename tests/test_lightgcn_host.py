"""LightGCN host-side pieces against the reference's recorded outputs
(tests/golden/lightgcn_small.npz, written by tests/golden/make_golden_lightgcn.py from
scripts/train_lightgcn.py) -- CPU, no GPU call."""
import ctypes
import random

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from _lightgcn_ref import sample_positives_numpy


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(GOLDEN / "lightgcn_small.npz"))


def _train_pos(fx):
    ptr, items = fx["user_ptr"], fx["user_items"]
    return {u: items[ptr[u]:ptr[u + 1]] for u in range(len(ptr) - 1) if ptr[u + 1] > ptr[u]}


def test_build_adj_bitwise(pkg, fx):
    tr = _train_pos(fx)
    assert len(tr) == 295 and len(np.unique(tr[3])) < len(tr[3])  # isolated users; a repeated interaction
    idx, val = pkg.lightgcn.build_adj(int(fx["n_users"]), int(fx["n_items"]), tr)
    assert idx.dtype == torch.int64 and val.dtype == torch.float32
    assert np.array_equal(idx.numpy(), fx["adj_indices"])
    assert np.array_equal(val.numpy().view(np.uint32), fx["adj_values"].view(np.uint32))


def test_build_adj_empty(pkg):
    idx, val = pkg.lightgcn.build_adj(3, 2, {})
    assert tuple(idx.shape) == (2, 0) and val.numel() == 0


def test_host_sampler_replays_the_reference_batches(pkg, fx):
    tr = _train_pos(fx)
    random.seed(42)
    gen = pkg.data.sample_lightgcn_batches(tr, int(fx["n_items"]), int(fx["neg_per_pos"]), int(fx["batch_size"]))
    for b in range(3):
        u, i, j = next(gen)
        assert np.array_equal(u, fx[f"b{b}_u"]) and np.array_equal(i, fx[f"b{b}_i"]), b
        assert np.array_equal(j, fx[f"b{b}_j"]), b


def test_host_sampler_last_batch_is_partial(pkg, fx):
    tr = _train_pos(fx)
    total = len(fx["user_items"]) * 2
    sizes = [len(u) for u, _, _ in pkg.data.sample_lightgcn_batches(tr, int(fx["n_items"]), 2, 1000)]
    assert sum(sizes) == total and all(s == 1000 for s in sizes[:-1]) and sizes[-1] == total % 1000


def test_sample_positives_restatement_columns(pkg, fx):
    """The device sampler's rule (numpy restatement): (u, i) equal the reference's batches; no j
    is a positive of its user."""
    tr = _train_pos(fx)
    n_items, npp, bs = int(fx["n_items"]), int(fx["neg_per_pos"]), int(fx["batch_size"])
    random.seed(7)
    host = list(pkg.data.sample_lightgcn_batches(tr, n_items, npp, bs))
    n_batches = -(-len(fx["user_items"]) * npp // bs)
    assert len(host) == n_batches
    pos_sets = {u: set(v.tolist()) for u, v in tr.items()}
    for b in (0, 1, 2, n_batches - 1):
        u, i, j, bad = sample_positives_numpy(fx["user_ptr"], fx["user_items"], n_items, npp, bs, b, seed=42)
        assert bad == 0
        assert np.array_equal(u, host[b][0]) and np.array_equal(i, host[b][1]), b
        assert all(int(jj) not in pos_sets[int(uu)] for uu, jj in zip(u, j))
        assert j.min() >= 0 and j.max() < n_items
    for b in range(3):
        u, i, _, _ = sample_positives_numpy(fx["user_ptr"], fx["user_items"], n_items, npp, bs, b, seed=1)
        assert np.array_equal(u, fx[f"b{b}_u"]) and np.array_equal(i, fx[f"b{b}_i"])


def test_abi_symbols_and_invalid_arguments(pkg):
    lib = pkg._lib.load()
    for name in ("ppgat_lgcn_supported", "ppgat_lgcn_hop_workspace_bytes", "ppgat_lgcn_hop",
                 "ppgat_bpr_sample_positives"):
        assert hasattr(lib, name) and name in pkg._lib.SIGNATURES
    assert lib.ppgat_version() == 3
    assert [c for c in range(1, 600) if lib.ppgat_lgcn_supported(c)] == [64, 128, 256]
    nb = ctypes.c_size_t(0)
    assert lib.ppgat_lgcn_hop_workspace_bytes(3, 64, ctypes.byref(nb)) == 0 and nb.value >= 3 * 64 * 4
    assert lib.ppgat_lgcn_hop_workspace_bytes(3, 32, ctypes.byref(nb)) == 2
    p = ctypes.c_void_p(256)  # never dereferenced: every call below fails validation first

    o = ctypes.c_void_p(1 << 20)

    def hop(sched, C=64, split=0, src1=None, div=1.0, ws=None, ws_bytes=0, out=o, accw=None, acc0=None):
        return lib.ppgat_lgcn_hop(sched, p, p, 10, 10, 5, C, p, src1, split, acc0, None, 0, div, out, accw, ws,
                                  ws_bytes, None)

    ok = pkg._lib.Schedule(p, p, p, 10, 0, None, None, 0, -1)
    assert hop(ctypes.byref(ok), C=32) == 2 and b"channels" in lib.ppgat_last_error()
    assert hop(ctypes.byref(ok), C=96) == 2
    assert hop(None) == 1 and b"schedule" in lib.ppgat_last_error()
    bad = pkg._lib.Schedule(None, None, None, 3, 5, None, None, 0, -1)
    assert hop(ctypes.byref(bad)) == 1 and b"inconsistent" in lib.ppgat_last_error()
    assert hop(ctypes.byref(ok), split=11, src1=ctypes.c_void_p(512)) == 1 and b"split" in lib.ppgat_last_error()
    assert hop(ctypes.byref(ok), split=-1, src1=ctypes.c_void_p(512)) == 1
    assert hop(ctypes.byref(ok), div=0.0) == 1 and b"div" in lib.ppgat_last_error()
    assert hop(ctypes.byref(ok), div=-2.0) == 1
    assert hop(ctypes.byref(ok), div=float("nan")) == 1
    assert hop(ctypes.byref(ok), out=None) == 1 and b"output" in lib.ppgat_last_error()
    assert hop(ctypes.byref(ok), out=p) == 1 and b"gathered" in lib.ppgat_last_error()
    hubs = pkg._lib.Schedule(p, p, p, 12, 3, p, p, 1, 4)
    assert hop(ctypes.byref(hubs)) == 1 and b"workspace" in lib.ppgat_last_error()
    assert hop(ctypes.byref(hubs), ws=p, ws_bytes=64) == 1 and b"workspace" in lib.ppgat_last_error()
    # the sampler: a range past nnz * neg_per_pos, neg_per_pos < 1
    sp = lib.ppgat_bpr_sample_positives
    assert sp(p, p, p, 4, 10, 7, 5, 51, 0, 0, p, p, p, p, None) == 1 and b"exceeds" in lib.ppgat_last_error()
    assert sp(p, p, p, 4, 10, 7, 5, 10, 0, 45, p, p, p, p, None) == 1
    assert sp(p, p, p, 4, 10, 7, 0, 10, 0, 0, p, p, p, p, None) == 1
    assert sp(p, p, p, 4, 10, 7, 5, 10, 0, 0, p, p, p, None, None) == 1 and b"null" in lib.ppgat_last_error()


def test_lightgcn_refuses_cpu_tensors(pkg, fx):
    m = pkg.LightGCN(int(fx["n_users"]), int(fx["n_items"]), 64, torch.from_numpy(fx["adj_indices"]),
                     torch.from_numpy(fx["adj_values"]))
    with pytest.raises(RuntimeError, match="ROCm"):
        m.propagate(3)
    with pytest.raises(RuntimeError, match="ROCm"):
        m(None, None)
    with pytest.raises(RuntimeError, match="ROCm"):
        pkg.lightgcn.LGCNGraph(m.adj_indices, m.adj_values, 420)


def test_state_dict_keys_and_seeded_weights(pkg, fx):
    torch.manual_seed(42)
    m = pkg.LightGCN(int(fx["n_users"]), int(fx["n_items"]), int(fx["embed_dim"]),
                     torch.from_numpy(fx["adj_indices"]), torch.from_numpy(fx["adj_values"]))
    assert sorted(m.state_dict().keys()) == ["E_item.weight", "E_user.weight", "adj_indices", "adj_values"]
    # the reference's construction order under set_seed(42): the same initial weights
    assert np.array_equal(m.E_user.weight.detach().numpy(), fx["b0_E_user"])
    assert np.array_equal(m.E_item.weight.detach().numpy(), fx["b0_E_item"])
    # a reference-layout checkpoint loads, and ours loads back
    sd = {"E_user.weight": torch.from_numpy(fx["b1_E_user"]), "E_item.weight": torch.from_numpy(fx["b1_E_item"]),
          "adj_indices": torch.from_numpy(fx["adj_indices"]), "adj_values": torch.from_numpy(fx["adj_values"])}
    m.load_state_dict(sd)
    assert np.array_equal(m.E_item.weight.detach().numpy(), fx["b1_E_item"])
    assert m.score(torch.ones(2, 3), torch.full((2, 3), 2.0)).tolist() == [6.0, 6.0]


def test_train_cli_has_the_reference_defaults(pkg):
    import importlib
    train = importlib.import_module(pkg.__name__ + ".train")
    c = train.LGCNConfig("p", "r", "s", "g", "m")
    assert (c.embed_dim, c.n_layers, c.lr, c.l2, c.epochs, c.batch_size, c.neg_per_pos, c.seed, c.eval_neg_k) == \
        (64, 3, 1e-3, 1e-4, 50, 8192, 5, 42, 1000)
