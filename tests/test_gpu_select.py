"""The older selection kernels on the GPU, called directly and compared element by element with the
exact references of tests/_select_ref.py: ppgat_knn_topk (through _lib), ppgat_serve_topk (through
evaluation.top_k_batch), ppgat_sampled_rank, and build_ii_knn at its edges against
oracle/knn_oracle.py.

No tolerance anywhere in the first three: the selection is handed its values (multiples of 1/16,
exact ties everywhere), the serving and ranking scores are integers over a power of two, exact in
fp32 whatever the summation order.  Indices, values (bitwise) and counts must all be equal."""
import numpy as np
import pytest
import torch

import _select_ref as ref
from test_knn import _compare

pytestmark = pytest.mark.gpu

IDX_GUARD, SIM_GUARD, CNT_GUARD = -7, 12345.0, -9


def _knn_call(pkg, cuda, S, n_cols, q0, k, min_sim, rows=None):
    """ppgat_knn_topk on S [rows, ld] with sentinel-filled outputs one row longer than needed ->
    (return code, idx, sim, cnt) as numpy, guard row included."""
    lib = pkg._lib.load()
    rows = S.shape[0] if rows is None else rows
    Sd = torch.from_numpy(S).to(cuda)
    idx = torch.full((rows + 1, max(k, 1)), IDX_GUARD, dtype=torch.int32, device=cuda)
    sim = torch.full((rows + 1, max(k, 1)), SIM_GUARD, dtype=torch.float32, device=cuda)
    cnt = torch.full((rows + 1,), CNT_GUARD, dtype=torch.int32, device=cuda)
    rc = lib.ppgat_knn_topk(Sd.data_ptr(), S.shape[1], rows, n_cols, q0, k, float(min_sim), idx.data_ptr(),
                            sim.data_ptr(), cnt.data_ptr(), pkg._lib.stream_handle(cuda))
    torch.cuda.synchronize()
    return rc, idx.cpu().numpy(), sim.cpu().numpy(), cnt.cpu().numpy()


def _knn_check(pkg, cuda, S, n_cols, q0, k, min_sim, tag):
    rc, idx, sim, cnt = _knn_call(pkg, cuda, S, n_cols, q0, k, min_sim)
    assert rc == 0, (tag, pkg._lib.load().ppgat_last_error().decode())
    rows = S.shape[0]
    assert (idx[rows] == IDX_GUARD).all() and (sim[rows] == SIM_GUARD).all() and cnt[rows] == CNT_GUARD, tag
    widx, wsim, wcnt = ref.knn_topk_ref(S, n_cols, q0, k, min_sim)
    assert np.array_equal(idx[:rows], widx), (tag, np.argwhere(idx[:rows] != widx)[:8])
    assert np.array_equal(sim[:rows].view(np.uint32), wsim.view(np.uint32)), tag
    assert np.array_equal(cnt[:rows], wcnt), (tag, cnt[:rows][:8], wcnt[:8])
    assert idx[:rows].max(initial=-1) < n_cols   # never a padding column (those hold +inf)
    return widx, wsim, wcnt


# (rows, n_cols, k, q0 kind, ld - n_cols, min_sim kind): every n_cols, k, rows, q0, ld and min_sim of
# the ladder at least once, the template boundaries 8|9, 16|17, 32|33, 64 at the small and the large
# widths, k > n_cols - 1 at every width below 65.
KNN_CASES = [
    (1, 1, 1, "zero", 0, "-inf"), (1, 1, 8, "none", 37, "-inf"), (3, 2, 1, "zero", 0, "present"),
    (4, 2, 9, "none", 37, "-inf"), (5, 2, 64, "zero", 0, "-inf"), (5, 63, 8, "zero", 0, "-inf"),
    (5, 63, 64, "seven", 37, "present"), (4, 63, 17, "end", 0, "above"), (5, 64, 9, "zero", 37, "-inf"),
    (3, 64, 64, "end", 0, "present"), (1, 64, 32, "none", 0, "+inf"), (5, 64, 1, "none", 0, "present"),
    (5, 65, 16, "seven", 0, "present"), (130, 65, 33, "zero", 37, "-inf"), (5, 255, 17, "end", 37, "present"),
    (4, 255, 1, "zero", 0, "-inf"), (5, 256, 8, "zero", 0, "present"), (5, 256, 32, "none", 37, "-inf"),
    (3, 256, 64, "seven", 0, "above"), (5, 257, 33, "end", 0, "-inf"), (5, 257, 9, "zero", 37, "present"),
    (1, 257, 16, "none", 0, "present"), (130, 257, 8, "end", 37, "present"), (130, 1000, 16, "zero", 0, "present"),
    (5, 1000, 1, "seven", 37, "-inf"), (5, 1000, 8, "end", 0, "+inf"), (5, 1000, 9, "none", 37, "present"),
    (5, 1000, 17, "zero", 0, "-inf"), (5, 1000, 32, "seven", 0, "present"), (5, 1000, 33, "end", 37, "above"),
    (130, 1000, 64, "none", 37, "present"), (4, 1000, 64, "zero", 0, "-inf"), (3, 1000, 16, "end", 37, "present"),
    (1, 1000, 64, "seven", 0, "present"),
]


def _q0(kind, n_cols, rows):
    return {"zero": 0, "seven": 7, "end": max(n_cols - rows, 0), "none": n_cols}[kind]


@pytest.mark.parametrize("case", KNN_CASES, ids=lambda c: "r{}_n{}_k{}_{}_pad{}_{}".format(*c))
def test_knn_topk_exact(pkg, cuda, case):
    rows, n_cols, k, q0_kind, pad, min_kind = case
    q0 = _q0(q0_kind, n_cols, rows)
    S = ref.knn_case(rows, n_cols, k, q0, n_cols + pad, seed=KNN_CASES.index(case))
    # thresholds from the values that can be selected: the middle one of the last row's list (an
    # ordinary row where rows > 5) is the >= edge; the next float above the best of any row keeps nothing
    sel = ref.knn_topk_ref(S, n_cols, q0, k, -np.inf)[1]
    last = sel[-1][np.isfinite(sel[-1])]
    assert min_kind == "-inf" or len(last)
    min_sim = {"-inf": lambda: -np.inf, "present": lambda: float(last[len(last) // 2]), "+inf": lambda: np.inf,
               "above": lambda: float(np.nextafter(sel.max(), np.float32(3.0)))}[min_kind]()
    widx, wsim, wcnt = _knn_check(pkg, cuda, S, n_cols, q0, k, min_sim, case)
    if min_kind == "present":
        assert (wsim == np.float32(min_sim)).any() and 0 < wcnt[-1] <= k
    if min_kind in ("+inf", "above"):
        assert (wcnt == 0).all() and np.isfinite(sel).any()
    if k > n_cols - 1:
        assert (widx == -1).any()          # the pads are part of what was compared


def test_knn_topk_treats_minus_inf_and_nan_as_absent(pkg, cuda):
    """-inf and NaN entries are never selected and never counted, whatever k and min_sim; a row of
    nothing else comes out as k pads with a count of 0."""
    rows, n_cols, ld = 9, 300, 337
    S = ref.knn_case(rows, n_cols, 16, 0, ld, seed=3, n_special=0)
    rng = np.random.default_rng(8)
    S[:, :n_cols][rng.random((rows, n_cols)) < 0.3] = -np.inf
    S[:, :n_cols][rng.random((rows, n_cols)) < 0.3] = np.nan
    S[4, :n_cols] = np.nan
    S[5, :n_cols] = -np.inf
    S[6, :n_cols] = np.nan
    S[6, 250] = -0.5                        # one real entry, in the second group of 256
    S[7, :n_cols:2] = np.nan                # NaN before every real value a lane sees
    for k, min_sim in ((1, -np.inf), (16, -np.inf), (17, -0.5), (64, -np.inf), (64, 0.25)):
        widx, _, wcnt = _knn_check(pkg, cuda, S, n_cols, 0, k, min_sim, (k, min_sim))
        assert (widx[4] == -1).all() and (widx[5] == -1).all() and wcnt[4] == wcnt[5] == 0
        assert widx[6].tolist() == [250] + [-1] * (k - 1) and wcnt[6] == (1 if -0.5 >= min_sim else 0)
    # all 300 columns real would give 64 items; here fewer than 64 survive in some row
    assert (ref.knn_topk_ref(S, n_cols, 0, 64, -np.inf)[2] < 64).any()


def test_knn_topk_refusals_write_nothing(pkg, cuda):
    S = ref.knn_case(4, 100, 8, 0, 100, seed=1)
    for k, ld_cols, code in ((0, 100, 2), (65, 100, 2), (8, 101, 1)):   # the last: ld (100) < n_cols (101)
        rc, idx, sim, cnt = _knn_call(pkg, cuda, S, ld_cols, 0, k, 0.0)
        assert rc == code, (k, ld_cols, rc)
        assert (idx == IDX_GUARD).all() and (sim == SIM_GUARD).all() and (cnt == CNT_GUARD).all()


# (C, B, n_items or None for k, k): C = 256 with B = 65 crosses the 64-user LDS batch, B = 257 the
# wrapper's 256-user chunk, n_items = 2048 * (1024 / C) + 5 the 2048-block grid-stride loop
SERVE_CASES = [
    (64, 1, 257, 1), (64, 65, 2048 * 16 + 5, 20), (64, 257, 257, 20), (64, 64, None, 64), (64, 256, 257, 64),
    (128, 65, 257, 20), (128, 256, 2048 * 8 + 5, 64), (128, 1, None, 20), (128, 257, 257, 1),
    (256, 65, 2048 * 4 + 5, 20), (256, 257, 257, 64), (256, 64, 257, 1), (256, 1, None, 64), (256, 65, None, 20),
]


def _serve_check(pkg, cuda, V, hists, k):
    idx, sc = pkg.evaluation.top_k_batch(torch.from_numpy(V).to(cuda), hists, k)
    assert idx.dtype == torch.int64 and sc.dtype == torch.float32 and tuple(idx.shape) == (len(hists), k)
    widx, wsc = ref.serve_topk_ref(V, hists, k)
    idx, sc = idx.cpu().numpy(), sc.cpu().numpy()
    assert np.array_equal(idx, widx), np.argwhere(idx != widx)[:8]
    assert np.array_equal(sc.astype(np.float64), wsc)
    return widx, wsc


@pytest.mark.parametrize("C,B,n_items,k", SERVE_CASES)
def test_serve_topk_exact(pkg, cuda, C, B, n_items, k):
    n = k if n_items is None else n_items
    V, hists = ref.serve_case(C, B, n, seed=C + B + n + k)
    widx, wsc = _serve_check(pkg, cuda, V, hists, k)
    if n_items is None:
        # k = n_items: every item is listed, the masked history last, in index order
        for b, h in enumerate(hists):
            assert widx[b, k - len(h):].tolist() == sorted(h) and (wsc[b, k - len(h):] == -1e9).all()
    elif k > 1 and n >= 257:
        assert (wsc[:, 1:] == wsc[:, :-1]).mean() > 0.05   # exact ties between neighbours: the index rule is exercised


def test_serve_topk_repeated_history_item(pkg, cuda):
    """An item twice in a history: counted twice in the mean, masked once."""
    V, hists = ref.serve_case(128, 3, 300, seed=9)
    hists[0] = [5, 5, 9, 12]
    hists[1] = [7] * 8
    widx, wsc = _serve_check(pkg, cuda, V, hists, 64)
    assert not np.isin(widx[0], [5, 9, 12]).any() and 7 not in widx[1]
    single = ref.serve_topk_ref(V, [[5, 9, 12, 12]], 64)[0]
    assert not np.array_equal(single[0], widx[0])          # the weight of the repeat changes the list
    widx, wsc = _serve_check(pkg, cuda, V[:64], [[5, 5, 9, 12], [7] * 8], 64)
    assert widx[0, -3:].tolist() == [5, 9, 12] and widx[1, -1] == 7 and (wsc[1, :-1] > -1e9).all()


def _rank(pkg, cuda, Z, n_users, users, cands, row_map=None):
    r = pkg.evaluation.sampled_rank(torch.from_numpy(Z).to(cuda), n_users, users, cands, row_map=row_map)
    assert r.dtype == np.int32 and r.shape == (len(users),)
    return r.astype(np.int64)


# every C, B and K1 of the ladder: K1 = 9 fills one block of EPW * U = 8 candidates exactly, 10 starts a second
RANK_CASES = [(32, 1, 1), (32, 5, 9), (32, 257, 101), (32, 3, 2), (64, 4, 8), (64, 257, 10), (64, 1, 130), (64, 5, 1),
              (128, 3, 9), (128, 5, 10), (128, 257, 2), (128, 4, 130), (256, 1, 8), (256, 4, 9), (256, 257, 130),
              (256, 5, 101), (256, 3, 1), (256, 5, 10)]


@pytest.mark.parametrize("C,B,K1", RANK_CASES)
def test_sampled_rank_exact(pkg, cuda, C, B, K1):
    n_users, n_items = 40, 60
    Z, users, cands = ref.rank_case(C, B, K1, seed=C * 1000 + B + K1, n_users=n_users, n_items=n_items)
    want = ref.sampled_rank_ref(Z, n_users, users, cands)
    got = _rank(pkg, cuda, Z, n_users, users, cands)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    if K1 == 1:
        assert (want == 1).all()
    if K1 >= 101 and B >= 5:
        assert len(np.unique(want)) > 3
    # the same rows behind a row_map: a permutation into a taller table whose other rows are NaN
    rng = np.random.default_rng(K1)
    tall = n_users + n_items + 53
    rows = rng.permutation(tall)[:n_users + n_items]
    T = np.full((tall, C), np.nan, np.float32)
    T[rows] = Z
    rm = torch.from_numpy(rows.astype(np.int32)).to(cuda)
    mapped = _rank(pkg, cuda, T, n_users, users, cands, row_map=rm)
    assert np.array_equal(mapped, want), np.flatnonzero(mapped != want)[:8]


def test_sampled_rank_positive_and_twins_do_not_count(pkg, cuda):
    """Every candidate is the positive itself or a row equal to it under another index: rank 1."""
    n_users, n_items, C = 40, 60, 64
    Z, users, _ = ref.rank_case(C, 6, 10, seed=5)
    pos = np.arange(6)                                      # items 0..5 have twins at 10..15
    cands = np.stack([pos, pos + 10, pos, pos + 10, pos, pos, pos + 10, pos, pos + 10, pos], 1).astype(np.int64)
    assert np.array_equal(ref.sampled_rank_ref(Z, n_users, users, cands), np.ones(6, np.int64))
    assert np.array_equal(_rank(pkg, cuda, Z, n_users, users, cands), np.ones(6, np.int64))


def _knn_inputs(n, d, seed):
    rng = np.random.default_rng(seed)
    centers = rng.standard_normal((max(n // 20, 2), d)).astype(np.float32)
    return (centers[rng.integers(0, len(centers), n)] + 0.7 * rng.standard_normal((n, d))).astype(np.float32)


@pytest.mark.parametrize("n,d,k,block", [(2, 1, 5, 1), (2, 33, 1, 50), (129, 1, 8, 50), (129, 33, 20, 1),
                                         (129, 33, 64, 50), (129, 33, 9, 128), (129, 1, 17, 128)])
def test_build_ii_knn_edges_vs_oracle(pkg, cuda, n, d, k, block):
    """Two items, one column, one query row per block, a block that does not divide n (50, 128 at
    n = 129), with a zero row and an identical pair among the embeddings: the reference script's
    lists under test_knn's near-tie rule, no bad row."""
    from oracle import knn_oracle
    emb = _knn_inputs(n, d, n * 100 + d)
    if n == 2:
        emb[1] = 2 * emb[0]                 # the same direction: each is the other's only neighbour
    else:
        emb[5] = 0.0                        # a zero row: no similarity reaches 0.3, for it or with it
        emb[17] = emb[40]                   # an identical pair
    want = knn_oracle.ii_knn(emb, min(k, n - 1), 0.3, batch_size=1000)
    rows, cols, sims = pkg.knn.build_ii_knn(torch.from_numpy(emb).to(cuda), k=k, min_similarity=0.3, block_rows=block)
    got = (rows.cpu().numpy(), cols.cpu().numpy(), sims.cpu().numpy())
    assert _compare(got, want, n, 0.3) == 0
    assert (got[1] >= 0).all() and (got[1] < n).all() and np.isfinite(got[2]).all()   # k > n - 1: no pad in the COO
    assert (got[0] != got[1]).all()
    if n == 2:
        assert got[0].tolist() == [0, 1] and got[1].tolist() == [1, 0]
    else:
        assert 5 not in got[0] and 5 not in got[1] and 5 not in want[0]
        if d > 1:
            first = {r: got[1][np.flatnonzero(got[0] == r)[0]] for r in (17, 40)}
            assert first == {17: 40, 40: 17}
            assert got[2][np.flatnonzero(got[0] == 17)[0]] == pytest.approx(1.0, abs=1e-5)
