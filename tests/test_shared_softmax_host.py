"""Shared-negatives softmax loss, host side: the references agree with autograd, the case builder's
facts, the condition behind the GPU bounds (from the references alone), ABI return codes, the
CPU-tensor refusal, the trainer's flag and the sampler's entry -- CPU."""
import ctypes
import functools
import importlib
import inspect
import math

import pytest
import torch

import _shs_ref as ref

# fp32 CPU restatement against float64, dZ per row over the term scale (upstream gradient 3.0),
# measured with this builder: the figures are in test_fp32_restatement_is_close_to_float64
RESTATEMENT_BOUND = 2.5e-6


@functools.lru_cache(maxsize=None)
def _case(P, C, tau):
    return ref.Reference(P, C, tau)


@pytest.mark.parametrize("P,C,tau,history", [(5, 8, 1.0, True), (40, 16, 0.1, True), (40, 16, 0.1, False)])
def test_formulas_equal_autograd(P, C, tau, history):
    r = ref.Reference(P, C, tau, seed=2, S=200, history=history)
    f = ref.formulas(r.Z, ref.N_USERS, r.u, r.pos, r.pool, r.mask, tau, upstream=3.0)
    assert abs(float(f["loss"] - r.loss)) <= 1e-12 * abs(float(r.loss))
    assert float((f["dZ"] - r.dZ).abs().max()) <= 1e-12 * float(r.dZ.abs().max())
    # every row's gradient is inside its term scale
    assert bool((r.dZ.abs().max(dim=1).values <= r.scale * (1 + 1e-12) + 1e-300).all())


def test_empty_batch_reference():
    r = ref.Reference(5, 8, 1.0, S=0)
    f = ref.formulas(r.Z, ref.N_USERS, r.u, r.pos, r.pool, r.mask, 1.0)
    assert float(f["loss"]) == 0.0 and float(f["dZ"].abs().max()) == 0.0 and float(r.loss) == 0.0


def test_case_builder_facts():
    for P, C, tau in ref.CASES:
        r = _case(P, C, tau)
        assert r.Z.shape == (ref.N_USERS + ref.N_ITEMS, C) and r.Z.dtype == torch.float32
        assert r.u.shape == r.pos.shape == (ref.N_SAMPLES,) and r.u.dtype == r.pos.dtype == torch.int64
        assert r.pool.shape == (P,) and r.pool.dtype == torch.int64 and r.items.dtype == torch.int32
        assert bool((r.pool[1:] > r.pool[:-1]).all()) and int(r.pool[0]) >= 0 and int(r.pool[-1]) == ref.N_ITEMS - 1
        n = r.ptr[1:] - r.ptr[:-1]
        assert int(n[ref.HOT_USER]) == ref.HOT_HIST and int(n[ref.EMPTY_USER]) == 0
        assert int((n == ref.HIST).sum()) == ref.N_USERS - 2
        for usr in (0, ref.HOT_USER, ref.N_USERS - 1):  # sorted and distinct per user
            h = r.items[int(r.ptr[usr]):int(r.ptr[usr + 1])]
            assert bool((h[1:] > h[:-1]).all())
        assert int((r.u == ref.EMPTY_USER).sum()) == 0
        assert 0.30 <= float((r.u == ref.HOT_USER).float().mean()) <= 0.37
        hot = r.pos == ref.HOT_ITEM
        assert 0.30 <= float(hot.float().mean()) <= 0.37
        if P >= 2:  # the hot positive is in the pool: a third of the samples have a masked pool column
            assert int((r.pool == ref.HOT_ITEM).sum()) == 1
            assert bool(r.mask[hot].any(dim=1).all())
        # rows nothing reaches (the GPU test wants them exactly 0)
        assert int((r.scale == 0).sum()) >= 1
    # P = 1: the pool is the last item, and the samples of the users who hold it lose their whole pool
    assert int(_case(1, 64, 1.0).mask.all(dim=1).sum()) >= 1


def test_fp32_restatement_is_close_to_float64():
    """The condition behind the GPU test's 1e-5: on every parity case the plain fp32 restatement
    of the formulas is within 2.5e-6 of float64, per row over the term scale.  Measured with this
    builder (P, C, tau -> dZ figure, loss relative error):
      (1, 64, 1) 1.6e-6, 5.0e-8      (33, 64, 1) 1.5e-6, 1.9e-8     (129, 128, 1) 1.9e-6, 7.6e-9
      (1000, 128, 0.1) 1.9e-6, 5.6e-9   (1000, 64, 0.1) 1.5e-6, 4.5e-8
    (and 5.1e-6 / 4.9e-5 on the two sharp cases, test_sharp_cases_bound_something)."""
    for P, C, tau in ref.CASES:
        lrel, drow = _case(P, C, tau).restatement()
        print(f"[shs restatement] P={P} C={C} tau={tau}: dZ/scale {drow:.3e}  loss rel {lrel:.3e}")
        assert drow <= RESTATEMENT_BOUND, ((P, C, tau), drow)
        assert lrel <= 2.5e-6, ((P, C, tau), lrel)


def test_sharp_cases_bound_something():
    """The two cases whose GPU bound is 4 x the restatement's own figure: the figure must lie in
    [1e-6, 5e-5] for that bound to check something (seeds: _shs_ref.SHARP_SEED / EXTREME_SEED)."""
    P, C, tau = ref.SHARP
    r = ref.Reference(P, C, tau, seed=ref.SHARP_SEED)
    _, fig = r.restatement(ref.UNDERFLOW_ABS)
    print(f"[shs restatement] sharp: dZ/scale {fig:.3e}")
    assert 1e-6 <= fig <= 5e-5, fig
    f = ref.formulas(r.Z, ref.N_USERS, r.u, r.pos, r.pool, r.mask, tau, upstream=3.0)
    assert ref.scaled_rows(r.dZ, f["dZ"], r.scale, ref.UNDERFLOW_ABS)[0] <= 1e-9
    P, C, tau = ref.EXTREME
    r = ref.Reference(P, C, tau, seed=ref.EXTREME_SEED, z_std=0.5)
    s = (r.Z.double()[r.u] @ r.Z.double()[ref.N_USERS + r.pool].T) / tau
    assert float(s.abs().max()) > 600.0
    _, fig = r.restatement(ref.UNDERFLOW_ABS)
    print(f"[shs restatement] extreme: dZ/scale {fig:.3e}")
    assert 1e-6 <= fig <= 5e-5, fig
    # the float64 autograd reference itself: p0 - 1 by subtraction must not have cancelled on any row
    f = ref.formulas(r.Z, ref.N_USERS, r.u, r.pos, r.pool, r.mask, tau, upstream=3.0)
    own = ref.scaled_rows(r.dZ, f["dZ"], r.scale, ref.UNDERFLOW_ABS)[0]
    print(f"[shs reference] extreme: float64 autograd against the float64 formulas {own:.3e}")
    assert own <= 1e-9, own
    f = ref.formulas(r.Z, ref.N_USERS, r.u, r.pos, r.pool, r.mask, tau, dtype=torch.float32)
    assert bool(torch.isfinite(f["dZ"]).all()) and math.isfinite(float(f["loss"]))


def test_abi_return_codes(pkg):
    """Invalid and unsupported arguments are refused before any device work (null device pointers)."""
    lib = pkg._lib.load()
    p = ctypes.c_void_p(256)
    nb = ctypes.c_size_t(0)
    assert lib.ppgat_shs_supported(64) == 1 and lib.ppgat_shs_supported(128) == 1
    assert [lib.ppgat_shs_supported(c) for c in (32, 96, 256)] == [0, 0, 0]
    ws = lib.ppgat_shs_workspace_bytes
    assert ws(90_000, 200_000, 1024, 128, ctypes.byref(nb)) == 0
    # at least the per-sample gradients and the mask words, and far from an [S, P] float matrix
    assert 200_000 * 128 * 4 + 200_000 * 32 * 4 <= nb.value < 200_000 * 1024 * 4 // 4
    small = nb.value
    assert ws(90_000, 200_000, 4096, 128, ctypes.byref(nb)) == 0 and small < nb.value < 200_000 * 4096 * 4 // 8
    assert ws(500, 0, 16, 64, ctypes.byref(nb)) == 0 and nb.value > 0
    assert ws(500, 2000, 1000, 96, ctypes.byref(nb)) == 2 and b"channels" in lib.ppgat_last_error()
    assert ws(500, 2000, 0, 128, ctypes.byref(nb)) == 1
    assert ws(500, 2000, 1000, 128, None) == 1

    def fwd(C=128, S=10, P=5, tau=1.0, Z=p, u=p, pos=p, pool=p, hp=None, hi=None, loss=p, lse=p, c0=p, bad=p, wsp=p,
            wsb=1 << 40):
        return lib.ppgat_shs_fwd(Z, 30, 10, 20, C, u, pos, S, pool, P, hp, hi, tau, loss, lse, c0, bad, wsp, wsb, None)

    def bwd(C=128, S=10, P=5, tau=1.0, Z=p, u=p, pos=p, pool=p, lse=p, c0=p, gl=p, dZ=p, wsp=p, wsb=1 << 40):
        return lib.ppgat_shs_bwd(Z, 30, 10, 20, C, u, pos, S, pool, P, tau, lse, c0, gl, dZ, wsp, wsb, None)

    for f in (fwd, bwd):
        for C in (16, 32, 96, 256):
            assert f(C=C) == 2 and b"channels" in lib.ppgat_last_error()
        assert f(P=0) == 1 and b"n_pool" in lib.ppgat_last_error()
        for tau in (0.0, -1.0, float("inf"), float("nan")):
            assert f(tau=tau) == 1 and b"temperature" in lib.ppgat_last_error()
        assert f(Z=None) == 1 and b"null" in lib.ppgat_last_error()
        assert f(u=None) == 1 and f(pos=None) == 1 and f(pool=None) == 1 and f(lse=None) == 1 and f(c0=None) == 1
        assert f(wsp=None) == 1
        assert f(wsb=16) == 1 and b"workspace" in lib.ppgat_last_error()
    assert fwd(loss=None) == 1 and fwd(bad=None) == 1 and bwd(gl=None) == 1 and bwd(dZ=None) == 1
    assert fwd(hp=p, hi=None) == 1 and b"together" in lib.ppgat_last_error()
    # n_rows must be n_users + n_items
    assert lib.ppgat_shs_fwd(p, 31, 10, 20, 128, p, p, 10, p, 5, None, None, 1.0, p, p, p, p, p, 1 << 40, None) == 1
    assert lib.ppgat_version() == 3


def test_python_argument_checks(pkg):
    hip_ops = importlib.import_module(pkg.__name__ + ".hip_ops")
    Z = torch.zeros(30, 64)
    u = torch.zeros(10, dtype=torch.int64)
    pos = torch.zeros(10, dtype=torch.int64)
    pool = torch.arange(5, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="ROCm.*no CPU path"):
        hip_ops.shared_softmax_loss(Z, 10, u, pos, pool)
    with pytest.raises(RuntimeError, match="ROCm.*no CPU path"):
        pkg.shared_softmax_loss(Z, 10, u, pos, pool, temperature=0.5, history=None)
    assert pkg.model.shared_softmax_loss is pkg.shared_softmax_loss and "shared_softmax_loss" in pkg.__all__
    assert list(inspect.signature(hip_ops.shared_softmax_loss).parameters) == [
        "Z", "n_users", "u", "pos", "pool", "temperature", "history"]
    with pytest.raises(ValueError, match="pool"):
        hip_ops.shared_softmax_loss(Z, 10, u, pos, pool.to(torch.int32))
    with pytest.raises(ValueError, match="pool"):
        hip_ops.shared_softmax_loss(Z, 10, u, pos, pool[:0])
    with pytest.raises(ValueError, match="pos"):
        hip_ops.shared_softmax_loss(Z, 10, u, pos[:9], pool)
    with pytest.raises(ValueError, match="temperature"):
        hip_ops.shared_softmax_loss(Z, 10, u, pos, pool, temperature=0.0)


def test_trainer_flag(pkg):
    train = importlib.import_module(pkg.__name__ + ".train")
    a = train.build_parser().parse_args([])
    assert a.shared_negatives == 0
    a = train.build_parser().parse_args(["--loss", "softmax", "--shared-negatives", "256"])
    assert a.shared_negatives == 256 and a.negatives == 16
    helps = {x.dest: x.help for x in train.build_parser()._actions}
    assert "unused" in helps["negatives"] and "pool" in helps["shared_negatives"]
    assert "shared" in inspect.signature(train.epoch_step).parameters
    for loss in ("bpr", "bce"):
        with pytest.raises(ValueError, match="shared-negatives"):
            train.main(["--synthetic", "cfg1", "--shared-negatives", "64", "--loss", loss])
    with pytest.raises(ValueError, match="shared-negatives"):
        train.main(["--synthetic", "cfg1", "--shared-negatives", "64"])
    with pytest.raises(ValueError, match="shared-negatives"):
        train.main(["--synthetic", "cfg1", "--loss", "softmax", "--shared-negatives", "-1"])
    # what --loss softmax refuses it refuses with a pool too
    for extra, word in ((["--model-family", "lightgcn"], "lightgcn"), (["--world-size", "2"], "world-size")):
        with pytest.raises(NotImplementedError, match=word):
            train.main(["--loss", "softmax", "--shared-negatives", "64", "--synthetic", "cfg1"] + extra)


def test_sampler_has_sample_pool(pkg):
    sig = inspect.signature(pkg.sampler.BPRSampler.sample_pool)
    assert list(sig.parameters) == ["self", "n_pool", "seed"]
