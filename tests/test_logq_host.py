"""Popularity-weighted negative sampling and the logQ correction, host side: the quantisation, the
distribution of the restated draw, the two correction formulas and the unbiasedness they buy, the
pool rule, the trainer's options and the ABI return codes of every new entry -- CPU."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import _wsample_ref as wref


@pytest.fixture(scope="module")
def sampler(pkg):
    return importlib.import_module(pkg.__name__ + ".sampler")


# ---- quantisation ----
def test_quantisation(sampler):
    x = np.array([0.0, 1e-30, 1.0, 0.5, 0.0, 0.25])
    w, cdf, total, log_q = sampler.quantise_item_weights(x, 6)
    assert w.dtype == np.uint64 and cdf.dtype == np.uint64 and log_q.dtype == np.float32
    assert w.tolist() == [0, 1, 2 ** 32, 2 ** 31, 0, 2 ** 30]  # a tiny positive weight is 1, never 0
    assert cdf.tolist() == [0, 1, 2 ** 32 + 1, 2 ** 32 + 2 ** 31 + 1, 2 ** 32 + 2 ** 31 + 1, total]
    assert total == 2 ** 32 + 2 ** 31 + 2 ** 30 + 1
    assert np.isneginf(log_q[[0, 4]]).all() and np.isfinite(log_q[[1, 2, 3, 5]]).all()
    assert np.array_equal(log_q[[1, 2, 3, 5]], np.log(w[[1, 2, 3, 5]].astype(np.float64) / total).astype(np.float32))
    # the restatement is the same quantisation, and a tensor is taken as an array is
    rw, rcdf, rtotal, rq = wref.quantise(x)
    assert np.array_equal(rw, w) and np.array_equal(rcdf, cdf) and rtotal == total
    w2, cdf2, total2, _ = sampler.quantise_item_weights(torch.from_numpy(x).float(), 6)
    assert total2 > 0 and w2[2] == 2 ** 32 and w2[0] == 0
    # Zipf over 63k items: the prefix sum is exact integer arithmetic
    z = 1.0 / np.arange(1, 63_002) ** 0.75
    w, cdf, total, _ = sampler.quantise_item_weights(z, 63_001)
    assert total == sum(int(v) for v in w) and int(cdf[-1]) == total and bool((np.diff(cdf.astype(object)) >= 0).all())


@pytest.mark.parametrize("bad", [[1.0, -0.5, 2.0], [1.0, float("nan"), 2.0], [1.0, float("inf"), 2.0], [0.0, 0.0, 0.0],
                                 [1.0, 2.0], [1.0, 2.0, 3.0, 4.0]], ids=["negative", "nan", "inf", "zero", "short", "long"])
def test_constructor_refuses_bad_weights(sampler, bad):
    """The weights are checked on the host before anything touches a device."""
    with pytest.raises(ValueError, match="item_weights"):
        sampler.BPRSampler(np.array([0, 1, 2]), np.array([0, 1]), 3, item_weights=np.array(bad))
    with pytest.raises(ValueError, match="item_weights"):
        sampler.quantise_item_weights(bad, 3)


def test_popularity_weights(sampler):
    ptr, items = np.array([0, 3, 3, 5]), np.array([4, 1, 1, 0, 4])
    w = sampler.BPRSampler.popularity_weights(ptr, items, 6)
    assert w.dtype == np.float64 and np.allclose(w, np.array([1, 2, 0, 0, 2, 0]) ** 0.75) and w[2] == 0.0
    assert np.array_equal(sampler.BPRSampler.popularity_weights(ptr, torch.from_numpy(items), 6, power=1.0),
                          [1, 2, 0, 0, 2, 0])
    with pytest.raises(ValueError):
        sampler.BPRSampler.popularity_weights(ptr, items, 4)


# ---- the distribution of the restated draw ----
def test_draw_distribution():
    """200,000 draws over 50 Zipf items (seed 7, checked on the CPU): every frequency within 5
    standard deviations sqrt(q (1 - q) / n) of q_i; an item of weight 0 never appears."""
    n = 200_000
    x = 1.0 / np.arange(1, 51)
    w, cdf, total, q = wref.quantise(x)
    d = wref.raw_draws(cdf, n, seed=7)
    freq = np.bincount(d, minlength=50) / n
    sd = np.sqrt(q * (1 - q) / n)
    z = np.abs(freq - q) / sd
    print("worst z", float(z.max()))
    assert d.min() >= 0 and d.max() < 50 and float(z.max()) <= 5.0, z
    x[[3, 17]] = 0.0
    _, cdf0, _, _ = wref.quantise(x)
    assert not np.isin(wref.raw_draws(cdf0, 50_000, seed=7), [3, 17]).any()


# ---- the correction formulas ----
def _ulp_close(got, want64):
    want = want64.astype(np.float32)
    fin = np.isfinite(want)
    assert np.array_equal(np.isneginf(got), np.isneginf(want)) and not np.isnan(got).any()
    return bool((np.abs(got[fin].astype(np.float64) - want64[fin]) <= 2.0 ** -23 * np.maximum(np.abs(want64[fin]), 1e-30)
                 + 1e-45).all())


def test_correction_formulas(sampler):
    x = 1.0 / np.arange(1, 2001) ** 1.1
    x[[5, 1999]] = 0.0
    w, cdf, total, _ = sampler.quantise_item_weights(x, 2000)
    _, _, _, q = wref.quantise(x)
    for M in (1, 16, 64):
        got = sampler.logq_correction(w, total, M)
        assert got.dtype == np.float32 and _ulp_close(got, wref.correction64(q, M))
    for T in (1, 40, 1024, 70_000):
        got = sampler.logq_pool_correction(w, total, T)
        assert got.dtype == np.float32 and _ulp_close(got, wref.pool_correction64(q, T))
        assert bool((got[np.isfinite(got)] <= 0).all())  # the log of a probability
    # the stable form keeps small q T where the naive one would lose it: log(q T) to first order
    tiny = wref.pool_correction64(np.array([1e-12]), 10)
    assert abs(float(tiny[0]) - np.log(1e-11)) <= 1e-9
    # one item holding all the mass is in every pool: log 1
    assert float(sampler.logq_pool_correction(np.array([0, 7], np.uint64), 7, 3)[1]) == 0.0


UNBIASED_SEEDS = 2000


def test_corrected_estimator_is_unbiased():
    """One user without history, 200 items, weights ~ rank^-1.2, scores that rise with popularity.
    Over 2,000 seeds the mean of exp(s0) + sum_m exp(s_m - log(M q_m)) (M = 16 weighted draws) lies
    within 4 standard errors of sum_all exp(s); the uncorrected mean scaled by n_items / M lies more
    than 4 away.  (The positive is the least popular item: the sampler never returns it as a
    negative, which renormalises q by 1 - q_pos = 1 - 4.5e-4, far inside the standard error.)  Float64
    throughout; figures on the CPU: corrected |z| = 0.65, uncorrected |z| = 137."""
    n_items, M = 200, 16
    x = 1.0 / np.arange(1, n_items + 1) ** 1.2
    w, cdf, total, q = wref.quantise(x)
    rng = np.random.default_rng(3)
    s = 0.8 * (np.log(q) - np.log(q).mean()) / np.log(q).std() + 0.3 * rng.standard_normal(n_items)
    pos = n_items - 1
    full = float(np.exp(s).sum())
    corr = wref.correction64(q, M)
    ptr, items = np.array([0, 0]), np.zeros(0, np.int64)
    est, raw = np.empty(UNBIASED_SEEDS), np.empty(UNBIASED_SEEDS)
    for seed in range(UNBIASED_SEEDS):
        cand, bad = wref.weighted_eval_sample(ptr, items, [0], [pos], n_items, M, seed, cdf)
        neg = cand[0, 1:]
        assert bad == 0 and pos not in neg
        est[seed] = np.exp(s[pos]) + np.exp(s[neg] - corr[neg]).sum()
        raw[seed] = np.exp(s[pos]) + n_items / M * np.exp(s[neg]).sum()
    z_corr = (est.mean() - full) / (est.std(ddof=1) / np.sqrt(UNBIASED_SEEDS))
    z_raw = (raw.mean() - full) / (raw.std(ddof=1) / np.sqrt(UNBIASED_SEEDS))
    print("z corrected", z_corr, "z uncorrected", z_raw, "q_pos", q[pos])
    assert abs(z_corr) <= 4.0, (z_corr, est.mean(), full)
    assert abs(z_raw) > 4.0, (z_raw, raw.mean(), full)


# ---- the pool rule ----
@pytest.mark.parametrize("n_pool", [1, 33, 150])
def test_pool_rule(n_pool):
    x = 1.0 / np.arange(1, 301) ** 0.9
    x[:40:4] = 0.0
    w, cdf, total, q = wref.quantise(x)
    items, T = wref.pool(w, cdf, n_pool, seed=11)
    assert items.shape == (n_pool,) and bool((np.diff(items) > 0).all()) and bool((w[items] > 0).all())
    d = wref.raw_draws(cdf, T, seed=11)
    assert len(np.unique(d)) == n_pool and len(np.unique(d[:T - 1])) == n_pool - 1  # T is minimal
    assert np.array_equal(items, np.unique(d))


def test_pool_rule_raises():
    x = np.zeros(100)
    x[:5] = 1.0
    w, cdf, _, _ = wref.quantise(x)
    assert len(wref.pool(w, cdf, 5, seed=0)[0]) == 5
    with pytest.raises(ValueError, match="positive weight"):
        wref.pool(w, cdf, 6, seed=0)
    x = np.full(100, 1e-12)
    x[0] = 1.0  # 99 items share 1e-10 of the mass: 64 * 50 draws do not find 50 of them
    w, cdf, _, _ = wref.quantise(x)
    with pytest.raises(ValueError, match="64 n_pool"):
        wref.pool(w, cdf, 50, seed=0)


# ---- trainer options ----
def test_trainer_options(pkg):
    train = importlib.import_module(pkg.__name__ + ".train")
    parse = train.build_parser().parse_args
    a = parse([])
    assert (a.negative_sampling, a.popularity_power, a.logq) == ("uniform", 0.75, "auto")
    assert train.check_negative_sampling(a) is False
    cfg = train.Config("p", "r", "s", "g", "e", "m")
    assert (cfg.negative_sampling, cfg.popularity_power, cfg.logq) == ("uniform", 0.75, "auto")
    pop = ["--negative-sampling", "popularity"]
    # --logq auto is on exactly when sampling is by popularity (and the loss has a correction)
    assert train.check_negative_sampling(parse(["--loss", "softmax"])) is False
    assert train.check_negative_sampling(parse(["--loss", "softmax", "--logq", "off"])) is False
    assert train.check_negative_sampling(parse(["--loss", "softmax"] + pop)) is True
    assert train.check_negative_sampling(parse(["--loss", "softmax", "--shared-negatives", "64"] + pop)) is True
    assert train.check_negative_sampling(parse(["--loss", "softmax", "--logq", "on"] + pop)) is True
    assert train.check_negative_sampling(parse(["--loss", "softmax", "--logq", "off"] + pop)) is False
    assert train.check_negative_sampling(parse(["--fast-sampler"] + pop)) is False
    assert train.check_negative_sampling(parse(["--loss", "bce", "--fast-sampler"] + pop)) is False
    for loss in ("bpr", "bce"):
        with pytest.raises(ValueError, match="logq on"):
            train.check_negative_sampling(parse(["--loss", loss, "--fast-sampler", "--logq", "on"] + pop))
        with pytest.raises(ValueError, match="fast-sampler"):
            train.check_negative_sampling(parse(["--loss", loss] + pop))
    with pytest.raises(ValueError, match="popularity"):
        train.check_negative_sampling(parse(["--loss", "softmax", "--logq", "on"]))
    with pytest.raises(ValueError, match="popularity-power"):
        train.check_negative_sampling(parse(["--loss", "softmax", "--popularity-power", "-1"] + pop))
    for extra in (pop, ["--logq", "on"]):
        with pytest.raises(NotImplementedError, match="lightgcn"):
            train.check_negative_sampling(parse(["--model-family", "lightgcn"] + extra))
        with pytest.raises(NotImplementedError, match="world-size"):
            train.check_negative_sampling(parse(["--loss", "softmax", "--world-size", "2"] + extra))
        with pytest.raises(NotImplementedError):  # main refuses before anything is loaded
            train.main(["--model-family", "lightgcn"] + extra)
    with pytest.raises(SystemExit):
        parse(["--negative-sampling", "alias"])


# ---- ABI return codes ----
def test_abi_return_codes(pkg):
    """Every new entry refuses invalid and unsupported arguments before any device work."""
    lib = pkg._lib.load()
    p = ctypes.c_void_p(256)
    nb = ctypes.c_size_t(0)
    for name in ("ppgat_weighted_draws", "ppgat_weighted_bpr_sample", "ppgat_weighted_eval_sample",
                 "ppgat_ssm_fwd_corrected", "ppgat_shs_corrected_workspace_bytes", "ppgat_shs_fwd_corrected",
                 "ppgat_shs_bwd_corrected"):
        assert hasattr(lib, name) and name in pkg._lib.SIGNATURES

    def draws(cdf=p, n_items=10, n=5, t0=0, out=p):
        return lib.ppgat_weighted_draws(cdf, n_items, n, 1, t0, out, None)

    assert draws(cdf=None) == 1 and b"null" in lib.ppgat_last_error()
    assert draws(out=None) == 1 and draws(n_items=0) == 1 and draws(n_items=2 ** 31) == 1
    assert draws(n=-1) == 1 and draws(t0=-1) == 1 and b"sizes" in lib.ppgat_last_error()

    def wbpr(ptr=p, items=p, el=p, ne=p, n_items=10, cdf=p, S=5, t0=0, u=p, i=p, j=p, bad=p):
        return lib.ppgat_weighted_bpr_sample(ptr, items, el, ne, n_items, cdf, S, 1, t0, u, i, j, bad, None)

    assert wbpr(n_items=0) == 1 and wbpr(n_items=2 ** 31) == 1 and wbpr(S=-1) == 1 and wbpr(t0=-1) == 1
    for k in ("ptr", "el", "ne", "cdf", "u", "i", "j", "bad"):
        assert wbpr(**{k: None}) == 1 and b"null" in lib.ppgat_last_error(), k

    def weval(ptr=p, items=p, users=p, pos=p, B=5, M=4, n_items=10, cdf=p, cands=p, bad=p):
        return lib.ppgat_weighted_eval_sample(ptr, items, users, pos, B, M, n_items, cdf, 1, cands, bad, None)

    assert weval(B=-1) == 1 and weval(M=-1) == 1 and weval(n_items=0) == 1 and weval(n_items=2 ** 31) == 1
    for k in ("ptr", "users", "pos", "cdf", "cands", "bad"):
        assert weval(**{k: None}) == 1 and b"null" in lib.ppgat_last_error(), k

    def ssm(C=64, S=10, K1=5, tau=1.0, Z=p, u=p, cand=p, corr=p, loss=p, coef=p, wsp=p, wsb=1 << 40, n_rows=30):
        return lib.ppgat_ssm_fwd_corrected(Z, n_rows, 10, 20, C, u, cand, corr, S, K1, tau, loss, coef, p, wsp, wsb, None)

    assert ssm(C=96) == 2 and b"channels" in lib.ppgat_last_error()
    assert ssm(K1=1) == 1 and ssm(n_rows=31) == 1 and ssm(S=-1) == 1
    for tau in (0.0, -1.0, float("inf"), float("nan")):
        assert ssm(tau=tau) == 1 and b"temperature" in lib.ppgat_last_error()
    for k in ("Z", "u", "cand", "corr", "loss", "coef", "wsp"):
        assert ssm(**{k: None}) == 1, k
    assert ssm(corr=None) == 1 and b"null" in lib.ppgat_last_error()
    assert ssm(wsb=16) == 1 and b"workspace" in lib.ppgat_last_error()

    ws, ws0 = lib.ppgat_shs_corrected_workspace_bytes, lib.ppgat_shs_workspace_bytes
    assert ws0(90_000, 200_000, 1024, 128, ctypes.byref(nb)) == 0
    plain = nb.value
    assert ws(90_000, 200_000, 1024, 128, ctypes.byref(nb)) == 0 and plain + 4096 <= nb.value <= plain + 4096 + 256
    assert ws(500, 2000, 1000, 96, ctypes.byref(nb)) == 2 and b"channels" in lib.ppgat_last_error()
    assert ws(500, 2000, 0, 128, ctypes.byref(nb)) == 1 and ws(500, 2000, 1000, 128, None) == 1
    assert ws(500, 2000, 1000, 64, ctypes.byref(nb)) == 0
    need = nb.value
    assert ws0(500, 2000, 1000, 64, ctypes.byref(nb)) == 0 and nb.value < need
    uncorrected = nb.value

    def fwd(C=64, S=2000, P=1000, tau=1.0, Z=p, u=p, pos=p, pool=p, hp=None, hi=None, corr=p, loss=p, lse=p, c0=p, bad=p,
            wsp=p, wsb=1 << 40):
        return lib.ppgat_shs_fwd_corrected(Z, 500, 100, 400, C, u, pos, S, pool, P, hp, hi, corr, tau, loss, lse, c0, bad,
                                           wsp, wsb, None)

    def bwd(C=64, S=2000, P=1000, tau=1.0, Z=p, u=p, pos=p, pool=p, lse=p, c0=p, gl=p, dZ=p, wsp=p, wsb=1 << 40):
        return lib.ppgat_shs_bwd_corrected(Z, 500, 100, 400, C, u, pos, S, pool, P, tau, lse, c0, gl, dZ, wsp, wsb, None)

    for f in (fwd, bwd):
        for C in (16, 32, 96, 256):
            assert f(C=C) == 2 and b"channels" in lib.ppgat_last_error()
        assert f(P=0) == 1 and b"n_pool" in lib.ppgat_last_error()
        for tau in (0.0, -1.0, float("inf"), float("nan")):
            assert f(tau=tau) == 1 and b"temperature" in lib.ppgat_last_error()
        assert f(Z=None) == 1 and b"null" in lib.ppgat_last_error()
        assert f(u=None) == 1 and f(pos=None) == 1 and f(pool=None) == 1 and f(lse=None) == 1 and f(c0=None) == 1
        assert f(wsp=None) == 1
        # the uncorrected workspace is too small: the gathered corrections sit behind it
        assert f(wsb=uncorrected) == 1 and b"workspace" in lib.ppgat_last_error()
    assert fwd(corr=None) == 1 and b"null" in lib.ppgat_last_error()
    assert fwd(loss=None) == 1 and fwd(bad=None) == 1 and bwd(gl=None) == 1 and bwd(dZ=None) == 1
    assert fwd(hp=p, hi=None) == 1 and b"together" in lib.ppgat_last_error()
    assert lib.ppgat_version() == 3


def test_python_argument_checks(pkg):
    """A CPU tensor is refused as before, whatever the correction."""
    hip_ops = importlib.import_module(pkg.__name__ + ".hip_ops")
    Z = torch.zeros(30, 64)
    u = torch.zeros(10, dtype=torch.int64)
    corr = torch.zeros(20)
    with pytest.raises(RuntimeError, match="ROCm.*no CPU path"):
        hip_ops.softmax_loss(Z, 10, u, torch.zeros(10, 3, dtype=torch.int64), correction=corr)
    with pytest.raises(RuntimeError, match="ROCm.*no CPU path"):
        pkg.shared_softmax_loss(Z, 10, u, u, torch.arange(5), correction=corr)
    with pytest.raises(RuntimeError, match="ROCm.*no CPU path"):
        hip_ops.shared_softmax_loss_corrected(Z, 10, u, u, torch.arange(5), 1.0, history=None, correction=corr)
    with pytest.raises(ValueError, match="pool"):
        hip_ops.shared_softmax_loss_corrected(Z, 10, u, u, torch.arange(5)[:0], correction=corr)
