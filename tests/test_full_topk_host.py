"""Host side of the full-catalogue top-K: the numpy reference against a brute-force loop,
topk_metrics against hand-computed values and against metrics_from_ranks, and the argument
validation of ppgat_full_topk through ctypes (every refusal returns before any device work, so no
GPU is needed and the pointers are never read)."""
import importlib
import math

import numpy as np
import pytest
import torch

import _fullrank_ref as rr
import _fulltopk_ref as ref


def test_reference_against_a_brute_force_loop():
    rng = np.random.default_rng(11)
    U = rng.integers(-2, 3, (5, 4)).astype(np.float32)
    I = rng.integers(-2, 3, (9, 4)).astype(np.float32)
    I[7] = I[2]  # a sure tie
    users = np.array([0, 1, 2, 3, 4, 0, 3])
    hist = {0: [1, 4], 1: [5, 6, 0], 2: [], 3: [8, 8, 2], 4: [0, 1, 2, 3, 4, 5, 6]}  # user 4: two items left
    ptr, items = rr.csr_from_lists(hist, 5)
    for k in (1, 3, 9, 12):
        idx, sc = ref.full_topk_ref(U, I, users, k, ptr, items)
        assert idx.shape == (7, k) and idx.dtype == np.int32
        for b, u in enumerate(users):
            cand = []
            for i in range(9):
                if i in hist[u]:
                    continue
                cand.append((sum(float(U[u, c]) * float(I[i, c]) for c in range(4)), i))
            # total order: score descending, index ascending (insertion sort, no library ordering)
            best = []
            for s, i in cand:
                pos = 0
                while pos < len(best) and (best[pos][0] > s or (best[pos][0] == s and best[pos][1] < i)):
                    pos += 1
                best.insert(pos, (s, i))
            best = best[:k]
            want_i = [i for _, i in best] + [-1] * (k - len(best))
            want_s = [s for s, _ in best] + [-np.inf] * (k - len(best))
            assert idx[b].tolist() == want_i and sc[b].tolist() == want_s, (k, b)
    idx, _ = ref.full_topk_ref(U, I, users, 9, ptr, items)
    assert (idx[4] >= 0).sum() == 2 and sorted(idx[4][:2].tolist()) == [7, 8]
    # users = None: query b is user b; no history: nothing is excluded
    idx0, sc0 = ref.full_topk_ref(U, I, None, 9)
    assert idx0.shape == (5, 9) and (np.sort(idx0, 1) == np.arange(9)).all() and (np.diff(sc0, axis=1) <= 0).all()
    two, seven = np.flatnonzero(idx0[0] == 2)[0], np.flatnonzero(idx0[0] == 7)[0]
    assert seven > two and sc0[0, two] == sc0[0, seven]  # the tied pair: the smaller index first


def test_topk_metrics_hand_computed(pkg):
    tm = pkg.evaluation.topk_metrics
    idx = np.array([[5, 3, 9, 1],    # held {3, 1, 7}: hits at positions 1 and 3
                    [2, 0, 4, 6],    # held {8}: no hit
                    [7, 8, -1, -1],  # held {7}: hit at 0; a padded list
                    [1, 2, 3, 4]])   # no held-out item: outside the means
    held = [[3, 1, 7], 8, [7], []]
    m = tm(idx, held, n_items=12, Ks=(2, 4))
    assert list(m) == ["recall@2", "recall@4", "ndcg@2", "ndcg@4", "precision@2", "precision@4", "hit@2", "hit@4",
                       "coverage@2", "coverage@4"]
    d = [1.0 / math.log2(q + 2) for q in range(4)]
    assert m["recall@2"] == pytest.approx((1 / 3 + 0 + 1) / 3) and m["recall@4"] == pytest.approx((2 / 3 + 0 + 1) / 3)
    assert m["ndcg@2"] == pytest.approx((d[1] / (d[0] + d[1]) + 0 + 1) / 3)
    assert m["ndcg@4"] == pytest.approx(((d[1] + d[3]) / (d[0] + d[1] + d[2]) + 0 + 1) / 3)
    assert m["precision@2"] == pytest.approx((0.5 + 0 + 0.5) / 3) and m["precision@4"] == pytest.approx((0.5 + 0 + 0.25) / 3)
    assert m["hit@2"] == pytest.approx(2 / 3) and m["hit@4"] == pytest.approx(2 / 3)
    assert m["coverage@2"] == 7 / 12 and m["coverage@4"] == 10 / 12  # {5,3,2,0,7,8,1}, then + {9,4,6}; pads never count
    # the CSR form of the same held-out sets, and a torch tensor of lists
    csr = (np.array([0, 3, 4, 5, 5]), np.array([3, 1, 7, 8, 7]))
    assert tm(torch.from_numpy(idx), csr, 12, Ks=(2, 4)) == m
    with pytest.raises(ValueError):
        tm(idx, held, 10, Ks=(5,))
    with pytest.raises(ValueError):
        tm(idx, held[:3], 10, Ks=(2,))
    empty = tm(np.zeros((0, 4), np.int64), [], 10, Ks=(2, 4))
    assert set(empty.values()) == {0.0} and list(empty) == list(m)


def test_topk_metrics_equal_metrics_from_ranks_for_single_positives(pkg):
    rng = np.random.default_rng(3)
    n, n_items, k = 200, 50, 20
    idx = np.stack([rng.permutation(n_items)[:k] for _ in range(n)])
    held = rng.integers(0, n_items, n)
    ranks = np.array([(np.flatnonzero(idx[b] == held[b])[0] + 1) if held[b] in idx[b] else k + 7 for b in range(n)])
    assert (ranks <= 10).any() and (ranks > 20).any()
    got = pkg.evaluation.topk_metrics(idx, held.tolist(), n_items, Ks=(10, 20))
    want = pkg.evaluation.metrics_from_ranks(ranks, Ks=(10, 20))
    for key, v in want.items():
        assert got[key] == v, key  # exactly: the same terms in the same order
    assert got["hit@10"] == got["recall@10"] and got["precision@20"] == pytest.approx(got["recall@20"] / 20)


def _call(lib, *, C=64, k=20, ldu=64, ldi=64, n_users=8, n_items=100, users=0x2000, n_query=4, uptr=0x3000, hist=0x4000,
          out_idx=0x5000, out_score=0x6000, ws=0x7000, ws_bytes=1 << 30):
    return lib.ppgat_full_topk(0x1000, ldu, n_users, 0x10000, ldi, n_items, C, users, n_query, uptr, hist, k, out_idx,
                               out_score, ws, ws_bytes, None)


def test_argument_validation_returns_before_any_device_work(pkg):
    lib = pkg._lib.load()
    max_k = lib.ppgat_full_topk_max_k()
    assert max_k >= 100
    assert [lib.ppgat_full_topk_supported(c) for c in (32, 64, 128, 256, 16, 48, 512)] == [1, 1, 1, 1, 0, 0, 0]
    err = lambda: lib.ppgat_last_error().decode()  # noqa: E731
    assert _call(lib, C=48, ldu=48, ldi=48) == 2 and "channels" in err()
    for k in (0, -3, max_k + 1):
        assert _call(lib, k=k) == 1 and "k" in err(), k
    assert _call(lib, ldu=66) == 1 and "ld_user" in err()   # not a multiple of 4
    assert _call(lib, ldi=32) == 1 and "ld_item" in err()   # below channels
    assert _call(lib, uptr=None) == 1 and "go together" in err()
    assert _call(lib, hist=None) == 1 and "go together" in err()
    assert _call(lib, ws=None) == 1 and "workspace" in err()
    assert _call(lib, ws_bytes=64) == 1 and "workspace" in err()
    assert _call(lib, out_idx=None) == 1
    assert _call(lib, users=None, n_query=9) == 1 and "n_query" in err()  # query b is user b: at most n_users
    assert _call(lib, n_query=-1) == 1
    # nothing to do: success without a launch (and without a workspace)
    assert _call(lib, n_query=0, users=None, out_idx=None, out_score=None, ws=None, ws_bytes=0) == 0
    import ctypes
    nbytes = ctypes.c_size_t(7)
    assert lib.ppgat_full_topk_workspace_bytes(0, 100, 64, 20, ctypes.byref(nbytes)) == 0 and nbytes.value == 0
    assert lib.ppgat_full_topk_workspace_bytes(4, 100, 48, 20, ctypes.byref(nbytes)) == 2
    assert lib.ppgat_full_topk_workspace_bytes(4, 100, 64, max_k + 1, ctypes.byref(nbytes)) == 1


def test_recommend_topk_refuses_cpu_tensors(pkg):
    Z = torch.zeros(12, 64)
    with pytest.raises(RuntimeError, match="ROCm"):
        pkg.evaluation.recommend_topk(Z[:4], Z[4:], k=3)
    for name in ("recommend_topk", "topk_metrics", "eval_topk"):
        assert getattr(pkg, name) is getattr(pkg.evaluation, name) and name in pkg.__all__


def test_trainer_recommend_flags(pkg):
    train = importlib.import_module(pkg.__name__ + ".train")
    ap = train.build_parser()
    a = ap.parse_args([])
    assert a.recommend_out is None and a.recommend_k == 20
    a = ap.parse_args(["--recommend-out", "r.npz", "--recommend-k", "10"])
    assert a.recommend_out == "r.npz" and a.recommend_k == 10
    with pytest.raises(NotImplementedError, match="one GPU"):
        train.main(["--recommend-out", "r.npz", "--world-size", "2"])
