"""Popularity-weighted negative sampling and the logQ-corrected softmax losses on the GPU: the three
weighted samplers and the pool against the numpy restatement (tests/_wsample_ref.py) bit for bit,
both losses with a correction against float64 autograd on the same fp32 inputs (the bounds of
tests/test_gpu_softmax_loss.py and tests/test_gpu_shared_softmax.py), the zero correction against
the uncorrected entries bit for bit, repeatability (debug library included), the refusal of -inf /
NaN corrections, and the trainer end to end.  The tests print their figures and record them through
conftest.write_report; DESIGN.md section 19 has the table."""
import functools
import importlib
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import _shs_ref
import _ssm_ref
import _wsample_ref as wref
from conftest import ROOT, write_report

pytestmark = pytest.mark.gpu

TOL = 1e-5
UP = 3.0  # the upstream gradient
NU, NI = _shs_ref.N_USERS, _shs_ref.N_ITEMS


@pytest.fixture(scope="module")
def hip_ops(pkg):
    return importlib.import_module(pkg.__name__ + ".hip_ops")


# ---------------------------------------------------------------------------
# samplers
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _graph():
    """The _shs_ref graph (300 users, 1,500 items, a hot user, a user without history) and Zipf
    weights with 100 items at weight 0 and one item holding a third of the mass."""
    _, u, pos, _, ptr, items = _shs_ref.make_case(33, 64)
    rng = np.random.default_rng(12)
    x = 1.0 / (1.0 + rng.permutation(NI))
    zero = rng.choice(NI, 100, replace=False)
    x[zero] = 0.0
    heavy = int(np.flatnonzero(x > 0)[5])
    x[heavy] = 0.0
    x[heavy] = x.sum() / 2.0
    w, cdf, total, q = wref.quantise(x)
    assert abs(q[heavy] - 1 / 3) < 1e-6 and int((w == 0).sum()) == 100
    return ptr.numpy(), items.numpy().astype(np.int64), u.numpy(), pos.numpy(), x, w, cdf, zero


@pytest.fixture(scope="module")
def smp(pkg, cuda):
    ptr, items, _, _, x, *_ = _graph()
    return pkg.sampler.BPRSampler(ptr, items, NI, device=cuda, item_weights=x)


@pytest.fixture(scope="module")
def plain(pkg, cuda):
    ptr, items, *_ = _graph()
    return pkg.sampler.BPRSampler(ptr, items, NI, device=cuda)


def test_quantised_tables_on_the_device(smp):
    _, _, _, _, x, w, cdf, _ = _graph()
    assert np.array_equal(smp.cdf.cpu().numpy().view(np.uint64), cdf) and smp.total == int(cdf[-1])
    lq = smp.log_q.cpu().numpy()
    assert lq.dtype == np.float32 and np.array_equal(np.isneginf(lq), w == 0)
    q = w.astype(np.float64) / float(smp.total)
    for got, want in ((smp.correction(16), wref.correction64(q, 16)), (smp.pool_correction(4000), wref.pool_correction64(q, 4000))):
        g = got.cpu().numpy()
        fin = np.isfinite(want)
        assert got.dtype == torch.float32 and np.array_equal(np.isneginf(g), ~fin)
        assert float(np.abs(g[fin] - want[fin]).max()) <= 2.0 ** -23 * float(np.abs(want[fin]).max())


def test_raw_draws(smp):
    _, _, _, _, _, w, cdf, zero = _graph()
    d = smp.weighted_draws(20_000, seed=5, offset=3).cpu().numpy()
    assert np.array_equal(d, wref.raw_draws(cdf, 20_000, seed=5, t0=3))
    assert not np.isin(d, zero).any() and bool((w[d] > 0).all())
    big = 2 ** 64 - 5  # the seed is the ABI's uint64
    assert np.array_equal(smp.weighted_draws(1000, seed=big).cpu().numpy(), wref.raw_draws(cdf, 1000, seed=big))


@pytest.mark.parametrize("M", [1, 16])
def test_candidates(smp, M):
    ptr, items, u, pos, _, w, cdf, zero = _graph()
    cand = smp.train_candidates(u, pos, M, seed=9).cpu().numpy()
    want, bad = wref.weighted_eval_sample(ptr, items, u, pos, NI, M, 9, cdf)
    assert bad == 0 and cand.shape == (2000, M + 1) and np.array_equal(cand, want)
    assert np.array_equal(cand[:, 0], pos) and not np.isin(cand[:, 1:], zero).any()
    hist = [set(items[ptr[a]:ptr[a + 1]].tolist()) for a in range(NU)]
    for t in range(2000):
        assert pos[t] not in cand[t, 1:] and not (set(cand[t, 1:].tolist()) & hist[u[t]])


def test_candidates_without_an_eligible_item(pkg, cuda):
    """A user whose items outside the history all have weight 0: 1,024 draws, then 0 and bad & 2."""
    ptr, items = np.array([0, 10, 12]), np.array(list(range(10)) + [3, 20])
    x = np.zeros(50)
    x[:10] = 1.0 + np.arange(10)
    s = pkg.sampler.BPRSampler(ptr, items, 50, device=cuda, item_weights=x)
    users, pos = np.array([1, 0, 1]), np.array([20, 4, 3])
    cand = s.train_candidates(users, pos, 3, seed=1, check=False)
    bad = int(s._bad.item())
    _, cdf, _, _ = wref.quantise(x)
    want, wbad = wref.weighted_eval_sample(ptr, items, users, pos, 50, 3, 1, cdf)
    assert bad & 2 and wbad == 2 and np.array_equal(cand.cpu().numpy(), want)
    assert cand[1].tolist() == [4, 0, 0, 0] and bool((cand[[0, 2], 1:] != 0).any())
    with pytest.raises(ValueError, match="no negative"):
        s.train_candidates(users, pos, 3, seed=1)


def test_triples(smp, plain):
    ptr, items, _, _, _, w, cdf, zero = _graph()
    u, i, j = (t.cpu().numpy() for t in smp.sample(5000, seed=21, offset=40))
    pu, pi, _ = (t.cpu().numpy() for t in plain.sample(5000, seed=21, offset=40))
    assert np.array_equal(u, pu) and np.array_equal(i, pi)  # the uniform sampler's bits
    wu, wi, wj, bad = wref.weighted_bpr_sample(ptr, items, NI, 5000, 21, cdf, t0=40)
    assert bad == 0 and np.array_equal(u, wu) and np.array_equal(i, wi) and np.array_equal(j, wj)
    assert not np.isin(j, zero).any()
    a = [t.cpu().numpy() for t in smp.sample(1700, seed=21, offset=40)]
    b = [t.cpu().numpy() for t in smp.sample(3300, seed=21, offset=1740)]
    for k, full in enumerate((u, i, j)):
        assert np.array_equal(np.concatenate([a[k], b[k]]), full)
    cu, cand = smp.sample_candidates(500, 6, seed=21, offset=40)
    assert np.array_equal(cu.cpu().numpy(), u[:500]) and np.array_equal(cand[:, 0].cpu().numpy(), i[:500])
    want, _ = wref.weighted_eval_sample(ptr, items, u[:500], i[:500], NI, 6, 21, cdf)
    assert np.array_equal(cand.cpu().numpy(), want)


@pytest.mark.parametrize("P", [1, 33, 1000])
def test_pool(smp, P):
    _, _, _, _, _, w, cdf, _ = _graph()
    got = smp.sample_pool(P, seed=4)
    want, T = wref.pool(w, cdf, P, seed=4)
    print("[pool]", P, "tries", T)
    assert got.dtype == torch.int64 and got.device.type == "cuda" and np.array_equal(got.cpu().numpy(), want)
    assert smp.pool_tries == T and bool((got[1:] > got[:-1]).all())


def test_pool_refusals(pkg, cuda, smp):
    with pytest.raises(ValueError, match="positive weight"):
        smp.sample_pool(1401)
    x = np.full(100, 1e-12)
    x[0] = 1.0
    s = pkg.sampler.BPRSampler(np.array([0, 1]), np.array([0]), 100, device=cuda, item_weights=x)
    with pytest.raises(ValueError, match="concentrated"):
        s.sample_pool(50)
    with pytest.raises(ValueError):
        smp.pool_correction(0)


def test_without_weights_nothing_changes(pkg, cuda, plain):
    ptr, items, u, pos, *_ = _graph()
    other = pkg.sampler.BPRSampler(ptr, items, NI, device=cuda, item_weights=None)
    assert not other.weighted and not plain.weighted
    assert torch.equal(plain.sample_pool(256, seed=3), other.sample_pool(256, seed=3))
    assert all(torch.equal(a, b) for a, b in zip(plain.sample(3000, seed=8, offset=5), other.sample(3000, seed=8, offset=5)))
    assert torch.equal(plain.eval_candidates(u, pos, 9, seed=2), other.eval_candidates(u, pos, 9, seed=2))
    assert torch.equal(plain.train_candidates(u, pos, 9, seed=2), other.eval_candidates(u, pos, 9, seed=2))
    with pytest.raises(ValueError, match="item_weights"):
        plain.correction(16)


def test_evaluation_stays_uniform(smp, plain):
    _, _, u, pos, *_ = _graph()
    assert torch.equal(smp.eval_candidates(u, pos, 20, seed=6), plain.eval_candidates(u, pos, 20, seed=6))
    a = smp.sample_positives(2, 512, 1, seed=6)
    b = plain.sample_positives(2, 512, 1, seed=6)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------------------
# sampled softmax with a correction
# ---------------------------------------------------------------------------
SSM_CASES = [(1, 32, 1.0), (7, 64, 1.0), (16, 128, 0.1), (16, 256, 0.1)]
assert all(c in _ssm_ref.CASES for c in SSM_CASES)
SNU = _ssm_ref.N_USERS


@functools.lru_cache(maxsize=None)
def _ssm_case(M, C, tau, seed=0, z_std=0.1):
    Z, u, cand = _ssm_ref.make_case(M, C, seed=seed, z_std=z_std)
    corr = wref.make_correction(_ssm_ref.N_ITEMS, seed=M + C)
    loss, dZ = wref.ssm_loss_autograd(Z, SNU, u, cand, tau, corr, upstream=UP)
    return Z, u, cand, corr, loss, dZ, wref.ssm_term_scale(Z, SNU, u, cand, tau, corr, upstream=UP)


def _ssm_run(hip_ops, Z, u, cand, tau, dev, corr=None):
    Zg = Z.to(dev).requires_grad_(True)
    loss = hip_ops.softmax_loss(Zg, SNU, u.to(dev), cand.to(dev), tau, correction=None if corr is None else corr.to(dev))
    (dZ,) = torch.autograd.grad(loss, Zg, torch.tensor(UP, device=dev))
    return loss.detach(), dZ


@pytest.mark.parametrize("M,C,tau", SSM_CASES)
def test_ssm_parity(hip_ops, cuda, M, C, tau):
    Z, u, cand, corr, loss64, dZ64, scale = _ssm_case(M, C, tau)
    assert float(corr.max()) == 80.0 and float(corr.min()) == -80.0
    loss, dZ = _ssm_run(hip_ops, Z, u, cand, tau, cuda, corr)
    hip_ops.check_bpr_indices()
    lrel = abs(float(loss.double().cpu() - loss64)) / abs(float(loss64))
    drow, zmax = _ssm_ref.scaled_rows(dZ, dZ64, scale)
    fig = {"M": M, "C": C, "tau": tau, "loss_rel": lrel, "dZ_row_over_scale": drow, "zero_rows_max": zmax}
    write_report(f"logq_ssm_parity_M{M}_C{C}_tau{tau}", fig)
    assert bool(torch.isfinite(dZ).all())
    assert lrel <= TOL, fig
    assert drow <= TOL and zmax == 0.0, fig


def test_ssm_extreme_logits(hip_ops, cuda):
    """tau = 0.01 with Z ~ 0.5 N(0, 1), logits of about +-900, and the correction on top: the term
    enters the online maximum, nothing overflows.  The bound is that of the uncorrected test: 4 x the
    fp32 CPU restatement's own figure on these inputs, never the kernel's."""
    M, C, tau = _ssm_ref.EXTREME
    Z, u, cand, corr, loss64, dZ64, scale = _ssm_case(M, C, tau, seed=_ssm_ref.EXTREME_SEED, z_std=0.5)
    _, r32 = wref.ssm_restatement_error(Z, SNU, u, cand, tau, corr, upstream=UP, abs_floor=_ssm_ref.UNDERFLOW_ABS)
    bound = max(TOL, 4.0 * r32)
    loss, dZ = _ssm_run(hip_ops, Z, u, cand, tau, cuda, corr)
    lrel = abs(float(loss.double().cpu() - loss64)) / abs(float(loss64))
    drow, zmax = _ssm_ref.scaled_rows(dZ, dZ64, scale, abs_floor=_ssm_ref.UNDERFLOW_ABS)
    fig = {"loss_rel": lrel, "dZ_row_over_scale": drow, "restatement": r32, "bound": bound, "zero_rows_max": zmax}
    write_report("logq_ssm_extreme", fig)
    assert bool(torch.isfinite(dZ).all()) and bool(torch.isfinite(loss))
    assert lrel <= TOL, fig
    assert drow <= bound and zmax == 0.0, fig


def test_ssm_zero_correction_and_repeat(hip_ops, cuda):
    for M, C, tau in ((7, 64, 1.0), (16, 256, 0.1)):
        Z, u, cand, corr, *_ = _ssm_case(M, C, tau)
        plain_ = _ssm_run(hip_ops, Z, u, cand, tau, cuda)
        zero = _ssm_run(hip_ops, Z, u, cand, tau, cuda, torch.zeros_like(corr))
        assert all(torch.equal(a, b) for a, b in zip(plain_, zero))
        a = _ssm_run(hip_ops, Z, u, cand, tau, cuda, corr)
        b = _ssm_run(hip_ops, Z, u, cand, tau, cuda, corr)
        assert all(torch.equal(x, y) for x, y in zip(a, b)) and not torch.equal(a[0], plain_[0])


def test_ssm_positive_is_not_corrected(hip_ops, cuda):
    """A table that differs only at items that are never a negative gives the same bits."""
    Z, u, cand, corr, *_ = _ssm_case(7, 64, 1.0)
    cand = cand.clone()
    cand[:, 0] = _ssm_ref.N_ITEMS - 1 - (torch.arange(cand.size(0)) % 3)  # the reserved items as positives ...
    cand[:, 1:] = cand[:, 1:].clamp(max=_ssm_ref.N_ITEMS - 4)            # ... and never as negatives
    other = corr.clone()
    other[-3:] += 5.0
    a = _ssm_run(hip_ops, Z, u, cand, 1.0, cuda, corr)
    b = _ssm_run(hip_ops, Z, u, cand, 1.0, cuda, other)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------------------
# shared negatives with a correction
# ---------------------------------------------------------------------------
SHS_CASES = [(1, 64, 1.0), (33, 64, 1.0), (129, 128, 1.0), (1000, 128, 0.1)]
assert all(c in _shs_ref.CASES for c in SHS_CASES)


@functools.lru_cache(maxsize=None)
def _shs_case(P, C, tau, history=True):
    return wref.ShsReference(P, C, tau, history=history)


def _shs_run(hip_ops, r, dev, corr="own", pool=None, u=None, pos=None):
    Zg = r.Z.to(dev).requires_grad_(True)
    hist = None if r.ptr is None else (r.ptr.to(dev), r.items.to(dev))
    corr = r.corr if isinstance(corr, str) else corr
    args = (Zg, NU, (r.u if u is None else u).to(dev), (r.pos if pos is None else pos).to(dev),
            (r.pool if pool is None else pool).to(dev), r.tau)
    if corr is None:  # the uncorrected public call
        loss = hip_ops.shared_softmax_loss(*args, history=hist)
    else:
        loss = hip_ops.shared_softmax_loss_corrected(*args, history=hist, correction=corr.to(dev))
    (dZ,) = torch.autograd.grad(loss, Zg, torch.tensor(UP, device=dev))
    return loss.detach(), dZ


@pytest.mark.parametrize("history", [True, False], ids=["hist", "nohist"])
@pytest.mark.parametrize("P,C,tau", SHS_CASES)
def test_shs_parity(hip_ops, cuda, P, C, tau, history):
    r = _shs_case(P, C, tau, history)
    loss, dZ = _shs_run(hip_ops, r, cuda)
    hip_ops.check_bpr_indices()
    lrel = abs(float(loss.double().cpu() - r.loss)) / max(abs(float(r.loss)), 1e-300)
    drow, zmax = _shs_ref.scaled_rows(dZ, r.dZ, r.scale)
    fig = {"P": P, "C": C, "tau": tau, "history": history, "loss_rel": lrel, "dZ_row_over_scale": drow,
           "zero_rows_max": zmax}
    print("[logq shs parity]", fig)
    write_report(f"logq_shs_parity_P{P}_C{C}_tau{tau}_{'hist' if history else 'nohist'}", fig)
    assert bool(torch.isfinite(dZ).all())
    assert lrel <= TOL, fig
    assert drow <= TOL and zmax == 0.0, fig


def test_shs_zero_correction_and_repeat(hip_ops, cuda):
    for P, C, tau in ((33, 64, 1.0), (1000, 128, 0.1)):
        r = _shs_case(P, C, tau)
        plain_ = _shs_run(hip_ops, r, cuda, corr=None)
        zero = _shs_run(hip_ops, r, cuda, corr=torch.zeros_like(r.corr))
        assert all(torch.equal(a, b) for a, b in zip(plain_, zero))
        a, b = _shs_run(hip_ops, r, cuda), _shs_run(hip_ops, r, cuda)
        assert all(torch.equal(x, y) for x, y in zip(a, b)) and not torch.equal(a[0], plain_[0])


def test_shs_whole_pool_masked(hip_ops, cuda):
    """P = 1 and every sample's positive is the pool's item: each loss term is 0 and c0 = 0, so the
    loss and every gradient row are exactly 0, whatever the correction (-80 here)."""
    r = _shs_case(1, 64, 1.0)
    pos = torch.full_like(r.pos, int(r.pool[0]))
    corr = r.corr.clone()
    corr[int(r.pool[0])] = -80.0
    loss, dZ = _shs_run(hip_ops, r, cuda, corr=corr, pos=pos)
    assert float(loss) == 0.0 and float(dZ.abs().max()) == 0.0


DEBUG_SNIPPET = r"""
import sys, importlib
import numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import _shs_ref, _ssm_ref, _wsample_ref as wref
pkg = importlib.import_module("plotpointe-gat-recommendation_amd")
hip_ops = importlib.import_module(pkg.__name__ + ".hip_ops")
assert pkg._lib.debug_build()
r = wref.ShsReference(1000, 128, 0.1)
Zg = r.Z.cuda().requires_grad_(True)
loss = hip_ops.shared_softmax_loss_corrected(Zg, _shs_ref.N_USERS, r.u.cuda(), r.pos.cuda(), r.pool.cuda(), r.tau,
                                             history=(r.ptr.cuda(), r.items.cuda()), correction=r.corr.cuda())
(dZ,) = torch.autograd.grad(loss, Zg, torch.tensor(3.0, device="cuda"))
Z, u, cand = _ssm_ref.make_case(16, 128)
corr = wref.make_correction(_ssm_ref.N_ITEMS, seed=16 + 128)
Zs = Z.cuda().requires_grad_(True)
l2 = hip_ops.softmax_loss(Zs, _ssm_ref.N_USERS, u.cuda(), cand.cuda(), 0.1, correction=corr.cuda())
(dZ2,) = torch.autograd.grad(l2, Zs, torch.tensor(3.0, device="cuda"))
np.savez(sys.argv[2], loss.detach().cpu().numpy(), dZ.cpu().numpy(), l2.detach().cpu().numpy(), dZ2.cpu().numpy())
print("DEBUG-OK")
"""


def test_debug_library_gives_the_same_bits(hip_ops, cuda, tmp_path):
    dbg = ROOT / "plotpointe-gat-recommendation_amd" / "libppgat_debug.so"
    if not dbg.exists():
        pytest.fail("libppgat_debug.so missing: build() makes it")
    env = dict(os.environ, PPGAT_LIB=str(dbg), HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, "-c", DEBUG_SNIPPET, str(ROOT), str(tmp_path / "d.npz")], env=env,
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "DEBUG-OK" in p.stdout, p.stdout[-2000:] + p.stderr[-3000:]
    Z, u, cand, corr, *_ = _ssm_case(16, 128, 0.1)
    got = _shs_run(hip_ops, _shs_case(1000, 128, 0.1), cuda) + _ssm_run(hip_ops, Z, u, cand, 0.1, cuda, corr)
    with np.load(tmp_path / "d.npz") as z:
        for k, t in enumerate(got):
            assert np.array_equal(z[f"arr_{k}"], t.cpu().numpy()), k


# ---------------------------------------------------------------------------
# validation of the correction
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("value", [float("-inf"), float("nan")], ids=["neginf", "nan"])
def test_bad_correction_terms_raise(hip_ops, cuda, value):
    hip_ops.check_bpr_indices()
    Z, u, cand, corr, *_ = _ssm_case(7, 64, 1.0)
    bad = corr.clone()
    bad[_ssm_ref.HOT_ITEM] = value  # a third of the candidates
    _ssm_run(hip_ops, Z, u, cand, 1.0, cuda, bad)
    with pytest.raises(ValueError, match="correction"):
        hip_ops.check_bpr_indices()
    hip_ops.check_bpr_indices()  # the pending count was consumed
    r = _shs_case(33, 64, 1.0)
    bad = r.corr.clone()
    bad[_shs_ref.HOT_ITEM] = value  # in the pool by construction
    _shs_run(hip_ops, r, cuda, corr=bad)
    with pytest.raises(ValueError, match="correction"):
        hip_ops.check_bpr_indices()
    _shs_run(hip_ops, r, cuda)
    _ssm_run(hip_ops, Z, u, cand, 1.0, cuda, corr)
    hip_ops.check_bpr_indices()


def test_bad_correction_tensors_raise_before_any_launch(hip_ops, cuda):
    Z, u, cand, corr, *_ = _ssm_case(7, 64, 1.0)
    r = _shs_case(33, 64, 1.0)
    for wrong in (corr[:-1], corr.double(), corr.view(1, -1), corr.tolist()):
        with pytest.raises(ValueError, match="correction"):
            hip_ops.softmax_loss(Z.to(cuda), SNU, u.to(cuda), cand.to(cuda), 1.0,
                                 correction=wrong.to(cuda) if torch.is_tensor(wrong) else wrong)
    with pytest.raises(ValueError, match="device"):  # a CPU table with a device Z
        hip_ops.softmax_loss(Z.to(cuda), SNU, u.to(cuda), cand.to(cuda), 1.0, correction=corr)
    for wrong in (r.corr[:-1].to(cuda), r.corr.double().to(cuda), r.corr):
        with pytest.raises(ValueError, match="correction"):
            hip_ops.shared_softmax_loss_corrected(r.Z.to(cuda), NU, r.u.to(cuda), r.pos.to(cuda), r.pool.to(cuda), 1.0,
                                                  correction=wrong)
    hip_ops.check_bpr_indices()
    # no gradient flows to the table
    c = corr.to(cuda).requires_grad_(True)
    Zg = Z.to(cuda).requires_grad_(True)
    hip_ops.softmax_loss(Zg, SNU, u.to(cuda), cand.to(cuda), 1.0, correction=c).backward()
    assert c.grad is None and Zg.grad is not None


# ---------------------------------------------------------------------------
# the trainer, end to end (child processes)
# ---------------------------------------------------------------------------
def _train(tmp_path, *flags):
    cmd = [sys.executable, str(ROOT / "plotpointe-gat-recommendation_amd" / "train.py"), "--synthetic", "cfg1",
           "--epochs", "2", "--eval-neg-k", "100", "--device-eval", "--models-prefix", str(tmp_path), *flags]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    files = list(tmp_path.glob("metrics_gat_pyg_d128_*.json"))
    ckpts = list((tmp_path / "checkpoints").glob("gat_pyg_d128_*.pt"))
    assert len(files) == 1 and len(ckpts) == 1
    return p.stdout, json.loads(files[0].read_text()), torch.load(ckpts[0], map_location="cpu", weights_only=True)


@pytest.mark.parametrize("flags", [["--negatives", "16"], ["--shared-negatives", "256"]], ids=["private", "shared"])
def test_trainer_softmax_popularity(tmp_path, flags):
    out, rec, ck = _train(tmp_path, "--loss", "softmax", "--negative-sampling", "popularity", *flags)
    losses = [float(v) for v in re.findall(r"\] loss=(\S+) \(softmax\)", out)]
    print("losses", flags, losses)
    write_report("logq_trainer_" + flags[0].strip("-").replace("-", "_"), {"losses": losses})
    assert len(losses) == 2 and all(np.isfinite(losses)) and all(v > 0 for v in losses), losses
    for cfg in (rec["config"], ck["config"]):
        assert (cfg["negative_sampling"], cfg["popularity_power"], cfg["logq"]) == ("popularity", 0.75, "auto")
    assert "logQ correction on" in rec["notes"]


def test_trainer_bpr_popularity(tmp_path):
    out, rec, ck = _train(tmp_path, "--loss", "bpr", "--fast-sampler", "--negative-sampling", "popularity",
                          "--popularity-power", "0.5")
    losses = [float(v) for v in re.findall(r"\] loss=(\S+) \(bpr\)", out)]
    print("losses bpr", losses)
    write_report("logq_trainer_bpr", {"losses": losses})
    assert len(losses) == 2 and all(np.isfinite(losses)), losses
    assert rec["config"]["negative_sampling"] == "popularity" and ck["config"]["popularity_power"] == 0.5
    assert "logQ correction off" in rec["notes"]
