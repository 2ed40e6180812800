"""Host side of the selection and InfoNCE tests: each numpy/torch reference of _select_ref.py and
_infonce_ref.py against a brute-force loop on a handful of rows, the exactness claim the integer
cases rest on, and the refusals of ppgat_knn_topk / ppgat_infonce through ctypes (each returns
before any device work, so no GPU is needed and the pointers are never read)."""
import ctypes
import math

import numpy as np
import torch

import _infonce_ref as iref
import _select_ref as sref


def _insertion_topk(pairs, k):
    """(value, index) pairs -> the k first under (value descending, index ascending), no library sort."""
    best = []
    for v, i in pairs:
        pos = 0
        while pos < len(best) and (best[pos][0] > v or (best[pos][0] == v and best[pos][1] < i)):
            pos += 1
        best.insert(pos, (v, i))
    return best[:k]


def test_knn_reference_against_a_brute_force_loop():
    rng = np.random.default_rng(5)
    n_cols, ld = 11, 14
    S = np.full((4, ld), np.inf, np.float32)
    S[:, :n_cols] = rng.integers(-4, 5, (4, n_cols)).astype(np.float32) / 4
    S[0, 3], S[0, 6], S[1, 0] = -np.inf, np.nan, np.nan
    S[2, :n_cols] = 0.5                                   # all equal
    S[3, :n_cols] = -np.inf                               # nothing to select
    for q0 in (0, 2, 9, n_cols):
        for k in (1, 3, 10, 12):
            for min_sim in (-np.inf, 0.25, 0.5, np.nextafter(np.float32(1), np.float32(2)), np.inf):
                idx, sim, cnt = sref.knn_topk_ref(S, n_cols, q0, k, min_sim)
                assert idx.shape == sim.shape == (4, k) and idx.dtype == np.int32 and sim.dtype == np.float32
                for r in range(4):
                    pairs = [(float(S[r, j]), j) for j in range(n_cols)
                             if j != q0 + r and not math.isnan(S[r, j]) and S[r, j] != -np.inf]
                    best = _insertion_topk(pairs, k)
                    assert idx[r].tolist() == [j for _, j in best] + [-1] * (k - len(best)), (q0, k, r)
                    assert sim[r].tolist() == [v for v, _ in best] + [-np.inf] * (k - len(best))
                    assert cnt[r] == sum(1 for v, _ in best if v >= min_sim), (q0, k, r, min_sim)
    idx, sim, cnt = sref.knn_topk_ref(S, n_cols, 0, 12, -np.inf)
    assert cnt.tolist() == [8, 9, 10, 0]                  # pads are not counted, even at min_sim = -inf
    assert idx[2, :3].tolist() == [0, 1, 3] and (idx[3] == -1).all()   # row 2: self (column 2) skipped, index order
    assert not np.isin(idx, [11, 12, 13]).any()           # the +inf padding columns


def test_knn_case_rows_are_what_they_claim():
    S = sref.knn_case(6, 1000, 8, q0=7, ld=1037, seed=0)
    assert np.isinf(S[:, 1000:]).all() and (S[:, :1000] * 16 == np.round(S[:, :1000] * 16))[5].all()
    body = lambda r: np.delete(S[r, :1000], 7 + r)  # noqa: E731
    assert (body(0) == 0.25).all() and (np.diff(body(1)) > 0).all() and (np.diff(body(2)) < 0).all()
    idx, sim, _ = sref.knn_topk_ref(S, 1000, 7, 8, -np.inf)
    assert len(set(idx[3] % 64)) == 1 and (sim[3, 0::2] == sim[3, 1::2]).all()     # one lane's stride, tied pairs
    assert (idx[4] >= 768).all()                                                     # the last partial group of 256
    assert all(S[r, 7 + r] == 2.0 and 7 + r not in idx[r] for r in range(6))         # self holds the maximum
    _, sim5, _ = sref.knn_topk_ref(S, 1000, 7, 64, -np.inf)
    assert (sim5[5, 1:] == sim5[5, :-1]).mean() > 0.5                                # ordinary rows: ties everywhere


def test_serve_reference_against_a_brute_force_loop():
    V, hists = sref.serve_case(8, 6, 23, seed=2, max_len=8)
    hists[0] = [4, 4, 9, 11]                              # a repeated item: twice in the mean, masked once
    V[7] = V[3]
    for k in (1, 5, 23):
        idx, sc = sref.serve_topk_ref(V, hists, k)
        for b, h in enumerate(hists):
            u = [sum(float(V[i, c]) for i in h) / len(h) for c in range(8)]
            pairs = [(-1e9 if i in h else sum(float(V[i, c]) * u[c] for c in range(8)), i) for i in range(23)]
            best = _insertion_topk(pairs, k)
            assert idx[b].tolist() == [i for _, i in best] and sc[b].tolist() == [s for s, _ in best], (k, b)
    idx, sc = sref.serve_topk_ref(V, hists, 23)
    assert idx[0, -3:].tolist() == [4, 9, 11] and (sc[0, -3:] == -1e9).all()   # the masked items close the list, by index


def test_serve_case_scores_are_exact_in_fp32():
    """The claim the exact comparison rests on: with integer items and power-of-two history lengths
    the fp32 mean and the fp32 scores equal the fp64 ones, in more than one summation order."""
    V, hists = sref.serve_case(256, 40, 8197, seed=1)
    hists[0] = hists[0][:1] * 16                          # one item sixteen times
    S64 = np.stack([V.astype(np.float64) @ V[np.asarray(h)].astype(np.float64).mean(0) for h in hists])
    u32 = np.stack([V[np.asarray(h)].mean(0, dtype=np.float32) for h in hists])
    assert np.array_equal((V @ u32.T).T.astype(np.float64), S64)
    assert np.array_equal((V[:, ::-1] @ u32[:, ::-1].T).T.astype(np.float64), S64)
    rev = np.cumsum((V[:, None, :] * u32[None, :3, :])[:, :, ::-1], axis=2, dtype=np.float32)[:, :, -1]
    assert np.array_equal(rev.T.astype(np.float64), S64[:3])
    assert len(np.unique(S64)) < 5000                     # few distinct values over 328k scores: ties everywhere


def test_sampled_rank_reference_against_a_brute_force_loop():
    Z, users, cands = sref.rank_case(8, 7, 10, seed=3)
    ref = sref.sampled_rank_ref(Z, 40, users, cands)
    assert ref.dtype == np.int64
    for b in range(7):
        s = [sum(float(Z[40 + c, d]) * float(Z[users[b], d]) for d in range(8)) for c in cands[b]]
        assert ref[b] == 1 + sum(1 for v in s[1:] if v > s[0]), b
    assert (cands[:, 3] == cands[:, 0]).all() and (Z[40 + cands[::2, 2]] == Z[40 + cands[::2, 0]]).all()
    Z1, u1, c1 = sref.rank_case(8, 3, 1, seed=4)
    assert sref.sampled_rank_ref(Z1, 40, u1, c1).tolist() == [1, 1, 1]


def test_infonce_reference_against_loops():
    g = torch.Generator().manual_seed(0)
    F, T, I = (torch.randn(5, 6, generator=g, dtype=torch.float64) for _ in range(3))
    F = F * torch.logspace(-2, 2, 5, dtype=torch.float64)[:, None]
    F[1] = 0.0                                            # the |x| <= eps branch, in fused and in txt_p
    T[3] = 0.0
    for tau in (0.07, 0.5):
        loss, dF, dT, dI, rowmax = iref.infonce(F, T, I, tau)
        l2, dF2, dT2, dI2 = iref.infonce_loops(F.tolist(), T.tolist(), I.tolist(), tau)
        assert np.allclose(loss.numpy(), l2, rtol=1e-12, atol=0)
        for a, b in ((dF, dF2), (dT, dT2), (dI, dI2)):
            b = np.asarray(b)
            assert np.isfinite(a.numpy()).all()
            assert (np.linalg.norm(a.numpy() - b, axis=1) <= 1e-11 * np.linalg.norm(b, axis=1)).all(), tau
        assert dF[1].abs().max() > 1e6 and dT[3].abs().max() > 1e6     # dy / 1e-12
        assert rowmax.shape == (5,)
    one = iref.infonce(F[:1], T[:1], I[:1], 0.07)
    assert (one[0] == 0).all() and all((g == 0).all() for g in one[1:4])   # B = 1: nothing to contrast


def test_relu_dropout_restatement_against_a_loop(oracle):
    z = np.array([0.0, -0.0, 1e-40, -1e-40, -2.5, 3.0, 1.0, 7.0, np.float32(1.5)], np.float32)
    g = np.array([1.0, 2.0, -3.0, 4.0, 5.0, -6.0, 7.0, 1e-41, -0.0], np.float32)
    for p in (0.0, 0.3, 0.999):
        m = oracle.mlp_dropout_scale(99, z.size, p)
        assert set(np.unique(m)) <= ({np.float32(1.0)} if p == 0 else {np.float32(0), np.float32(1) / (np.float32(1) - np.float32(p))})
        a = iref.relu_dropout(z, p, 99, oracle.mlp_dropout_scale)
        dz = iref.relu_dropout(z, p, 99, oracle.mlp_dropout_scale, grad=g)
        for t in range(z.size):
            fa = np.float32(z[t] if z[t] > 0 else 0.0) * m[t]
            fd = g[t] * m[t] if z[t] > 0 else np.float32(0.0)
            assert a[t].tobytes() == np.float32(fa).tobytes() and dz[t].tobytes() == np.float32(fd).tobytes(), (p, t)
        assert a[:2].view(np.uint32).tolist() == [0, 0] and a[3] == 0 and a[4] == 0   # +0, -0, negatives -> +0
    assert iref.relu_dropout(z, 0.0, 99, oracle.mlp_dropout_scale)[2] == np.float32(1e-40)   # a denormal passes


def test_knn_topk_and_infonce_refusals_return_before_any_device_work(pkg):
    lib = pkg._lib.load()
    err = lambda: lib.ppgat_last_error().decode()  # noqa: E731

    def knn(k=8, ld=100, n_cols=100, q0=0):
        return lib.ppgat_knn_topk(0x1000, ld, 4, n_cols, q0, k, 0.0, 0x2000, 0x3000, 0x4000, None)

    assert lib.ppgat_knn_max_k() == 64
    assert knn(k=0) == 2 and "k must be" in err()
    assert knn(k=65) == 2 and "k must be" in err()
    assert knn(ld=99) == 1 and "bad sizes" in err()
    assert knn(n_cols=0, ld=0) == 1 and knn(q0=-1) == 1
    nbytes = ctypes.c_size_t(7)
    for B, D in ((4097, 128), (0, 128), (64, 64)):
        assert lib.ppgat_infonce_workspace_bytes(B, D, ctypes.byref(nbytes)) == 2 and "4096" in err(), (B, D)
        assert lib.ppgat_infonce(0x1000, 0x2000, 0x3000, B, D, 0.07, 0x4000, 0x5000, 0x6000, 0x7000, 0x8000, 1 << 40,
                                 None) == 2 and "dim 128" in err(), (B, D)
    assert nbytes.value == 7
    assert lib.ppgat_infonce_workspace_bytes(4096, 128, ctypes.byref(nbytes)) == 0 and nbytes.value > 2 * 4096 * 4096 * 4
