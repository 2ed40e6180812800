"""Sampled-softmax loss, host side: the references agree with autograd, the case builder's facts,
the condition behind the GPU bounds (from the references alone), trainer options and refusals,
ABI return codes, the CPU-tensor refusal and the sampler's entry -- CPU."""
import ctypes
import importlib
import inspect
import math

import pytest
import torch

import _ssm_ref as ref

# fp32 CPU restatement against float64, dZ per row over the term scale (upstream gradient 3.0),
# measured with this builder: the figures are in test_fp32_restatement_is_close_to_float64
RESTATEMENT_BOUND = 2.5e-6


@pytest.mark.parametrize("M,C,tau", [(3, 8, 1.0), (5, 16, 0.1)])
def test_formulas_equal_autograd(M, C, tau):
    Z, u, cand = ref.make_case(M, C, seed=2, S=200)
    loss, dZ = ref.loss_autograd(Z, ref.N_USERS, u, cand, tau, upstream=3.0)
    f = ref.formulas(Z, ref.N_USERS, u, cand, tau, upstream=3.0)
    assert abs(float(f["loss"] - loss)) <= 1e-13 * abs(float(loss))
    assert float((f["dZ"] - dZ).abs().max()) <= 1e-13 * float(dZ.abs().max())
    # every row's gradient is inside its term scale
    sc = ref.term_scale(Z, ref.N_USERS, u, cand, tau, upstream=3.0)
    assert bool((dZ.abs().max(dim=1).values <= sc * (1 + 1e-12) + 1e-300).all())


def test_formulas_at_one_negative_are_softplus():
    """M = 1, tau = 1: loss = softplus(s_neg - s_pos), BPR without its 1e-8."""
    Z, u, cand = ref.make_case(1, 32)
    f = ref.formulas(Z, ref.N_USERS, u, cand, 1.0)
    Zd = Z.double()
    pos = (Zd[u] * Zd[ref.N_USERS + cand[:, 0]]).sum(-1)
    neg = (Zd[u] * Zd[ref.N_USERS + cand[:, 1]]).sum(-1)
    want = torch.nn.functional.softplus(neg - pos).mean()
    assert abs(float(f["loss"] - want)) <= 1e-13 * float(want)


def test_empty_batch_reference():
    Z, u, cand = ref.make_case(3, 8, S=0)
    f = ref.formulas(Z, ref.N_USERS, u, cand, 1.0)
    assert float(f["loss"]) == 0.0 and float(f["dZ"].abs().max()) == 0.0


def test_case_builder_facts():
    for M, C, _ in ref.CASES:
        Z, u, cand = ref.make_case(M, C)
        assert Z.shape == (ref.N_USERS + ref.N_ITEMS, C) and Z.dtype == torch.float32
        assert cand.shape == (ref.N_SAMPLES, M + 1) and cand.dtype == torch.int64 and u.dtype == torch.int64
        assert int(cand.min()) >= 0 and int(cand.max()) < ref.N_ITEMS and int(u.min()) >= 0 and int(u.max()) < ref.N_USERS
        assert int((cand == ref.ITEM_ONE).sum()) == 1
        assert int((cand == ref.ITEM_32).sum()) == 32
        assert int((cand == ref.ITEM_33).sum()) == 33
        hot = cand == ref.HOT_ITEM
        assert 0.30 <= float(hot.float().mean()) <= 0.37
        assert int(hot[:, 0].sum()) > ref.N_SAMPLES // 4 and int(hot[:, 1:].sum()) > 0   # positive and negative terms
        assert 0.30 <= float((u == ref.HOT_USER).float().mean()) <= 0.37
        assert int((hot.sum(1) >= 2).sum()) > 0 or M == 1                                # duplicates in a row
    _, _, cand = ref.make_case(64, 64)
    assert int((cand == ref.HOT_ITEM).sum()) > 40_000
    assert int(((cand == ref.HOT_ITEM).sum(1) >= 2).sum()) > 1000


def test_fp32_restatement_is_close_to_float64():
    """The condition behind the GPU test's 1e-5: on every parity case the plain fp32 restatement
    of the formulas is within 2.5e-6 of float64, per row over the term scale.  Measured with this
    builder (M, C, tau -> dZ figure, loss relative error):
      (1, 32, 1) 1.5e-7, 3.1e-8    (7, 64, 1) 2.0e-7, 2.7e-8      (64, 64, 1) 5.5e-7, 2.9e-8
      (16, 128, 0.1) 1.6e-6, 7.5e-8  (16, 256, 0.1) 1.9e-6, 8.7e-9  (16, 32, 0.02) 2.1e-6, 3.9e-8
    (and 1.6e-5 on the extreme-logit case, test_extreme_case_logits_are_large)."""
    seen = {}
    for M, C, tau in ref.CASES:
        Z, u, cand = ref.make_case(M, C)
        lrel, drow = ref.restatement_error(Z, ref.N_USERS, u, cand, tau, upstream=3.0)
        seen[(M, C, tau)] = (drow, lrel)
        print(f"[ssm restatement] M={M} C={C} tau={tau}: dZ/scale {drow:.3e}  loss rel {lrel:.3e}")
    for key, (drow, lrel) in seen.items():
        assert drow <= RESTATEMENT_BOUND, (key, drow)
        assert lrel <= 2.5e-6, (key, lrel)


def test_extreme_case_logits_are_large():
    M, C, tau = ref.EXTREME
    Z, u, cand = ref.make_case(M, C, seed=ref.EXTREME_SEED, z_std=0.5)
    s = (Z.double()[u].unsqueeze(1) * Z.double()[ref.N_USERS + cand]).sum(-1) / tau
    assert float(s.abs().max()) > 600.0
    # the restatement's own error here is what bounds the GPU test (x 4): it must bound something
    _, r32 = ref.restatement_error(Z, ref.N_USERS, u, cand, tau, upstream=3.0, abs_floor=ref.UNDERFLOW_ABS)
    print(f"[ssm restatement] extreme: dZ/scale {r32:.3e}")
    assert 1e-6 <= r32 <= 5e-5, r32
    f = ref.formulas(Z, ref.N_USERS, u, cand, tau, dtype=torch.float32)
    assert bool(torch.isfinite(f["dZ"]).all()) and math.isfinite(float(f["loss"]))


def test_trainer_options(pkg):
    train = importlib.import_module(pkg.__name__ + ".train")
    a = train.build_parser().parse_args([])
    assert a.loss == "bpr" and a.negatives == 16 and a.temperature == 1.0
    a = train.build_parser().parse_args(["--loss", "softmax", "--negatives", "8", "--temperature", "0.5"])
    assert a.loss == "softmax" and a.negatives == 8 and a.temperature == 0.5
    helps = {x.dest: x.help for x in train.build_parser()._actions}
    assert "convention" in helps["negatives"]
    cfg = train.Config("p", "r", "s", "g", "e", "m")
    assert cfg.negatives == 16 and cfg.temperature == 1.0 and list(cfg.__dict__)[-2:] == ["negatives", "temperature"]
    cfg = train.Config("p", "r", "s", "g", "e", "m", hidden_dim=64, layers=1, loss="softmax", negatives=4, temperature=0.2)
    assert cfg.__dict__["negatives"] == 4 and cfg.__dict__["temperature"] == 0.2
    for fam in ("gat_pyg", "gat_custom", "gatv2_pyg"):
        cfg.model_family = fam
        assert train.build_model(cfg, 7, 5, 12).n_users == 7
    assert "softmax" in inspect.signature(train.epoch_step).parameters
    assert list(inspect.signature(train.epoch_step).parameters)[:10] == [
        "model", "opt", "item_feats", "edge_index", "n_users", "u", "i", "j", "loss", "edge_attr"]


def test_trainer_refusals(pkg):
    train = importlib.import_module(pkg.__name__ + ".train")
    for extra, word in ((["--model-family", "lightgcn"], "lightgcn"), (["--world-size", "2"], "world-size")):
        with pytest.raises(NotImplementedError, match=word):
            train.main(["--loss", "softmax", "--synthetic", "cfg1"] + extra)
    with pytest.raises(ValueError, match="negatives"):
        train.main(["--loss", "softmax", "--synthetic", "cfg1", "--negatives", "0"])
    with pytest.raises(ValueError, match="temperature"):
        train.main(["--loss", "softmax", "--synthetic", "cfg1", "--temperature", "0"])


def test_abi_return_codes(pkg):
    """Invalid and unsupported arguments are refused before any device work (null device pointers)."""
    lib = pkg._lib.load()
    p = ctypes.c_void_p(256)
    nb = ctypes.c_size_t(0)
    ws = lib.ppgat_ssm_workspace_bytes
    assert ws(500, 2000, 17, 128, ctypes.byref(nb)) == 0 and nb.value >= 2000 * 17 * 16
    small = nb.value
    assert ws(500, 2000, 65, 128, ctypes.byref(nb)) == 0 and nb.value > small
    assert ws(500, 0, 2, 32, ctypes.byref(nb)) == 0 and nb.value > 0
    assert ws(500, 2000, 17, 96, ctypes.byref(nb)) == 2 and b"channels" in lib.ppgat_last_error()
    assert ws(500, 2000, 1, 128, ctypes.byref(nb)) == 1
    assert ws(500, 2000, 17, 128, None) == 1
    assert ws(500, 2 ** 31 // 18 + 1, 17, 128, ctypes.byref(nb)) == 1     # n_samples (n_cand + 1) >= 2^31

    def fwd(C=128, S=10, K1=5, tau=1.0, Z=p, u=p, cand=p, loss=p, coef=p, wsp=p, wsb=1 << 40):
        return lib.ppgat_ssm_fwd(Z, 30, 10, 20, C, u, cand, S, K1, tau, loss, coef, None, wsp, wsb, None)

    def bwd(C=128, S=10, K1=5, tau=1.0, Z=p, u=p, cand=p, coef=p, gl=p, dZ=p, wsp=p, wsb=1 << 40):
        return lib.ppgat_ssm_bwd(Z, 30, 10, 20, C, u, cand, S, K1, tau, coef, gl, dZ, wsp, wsb, None)

    for f in (fwd, bwd):
        for C in (16, 48, 96, 512):
            assert f(C=C) == 2 and b"channels" in lib.ppgat_last_error()
        assert f(K1=1) == 1 and b"n_cand" in lib.ppgat_last_error()
        for tau in (0.0, -1.0, float("inf"), float("nan")):
            assert f(tau=tau) == 1 and b"temperature" in lib.ppgat_last_error()
        assert f(S=2 ** 31 // 6 + 1) == 1 and b"2^31" in lib.ppgat_last_error()
        assert f(Z=None) == 1 and b"null" in lib.ppgat_last_error()
        assert f(u=None) == 1 and f(cand=None) == 1 and f(coef=None) == 1
        assert f(wsp=None) == 1
        assert f(wsb=16) == 1 and b"workspace" in lib.ppgat_last_error()
    assert fwd(loss=None) == 1 and bwd(gl=None) == 1 and bwd(dZ=None) == 1
    # n_rows must be n_users + n_items
    assert lib.ppgat_ssm_fwd(p, 31, 10, 20, 128, p, p, 10, 5, 1.0, p, p, None, p, 1 << 40, None) == 1
    assert lib.ppgat_version() == 3


def test_python_argument_checks(pkg):
    hip_ops = importlib.import_module(pkg.__name__ + ".hip_ops")
    Z = torch.zeros(30, 64)
    u = torch.zeros(10, dtype=torch.int64)
    cand = torch.zeros(10, 5, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="ROCm.*no CPU path"):
        hip_ops.softmax_loss(Z, 10, u, cand)
    with pytest.raises(RuntimeError, match="ROCm.*no CPU path"):
        pkg.softmax_loss(Z, 10, u, cand, temperature=0.5)
    assert pkg.model.softmax_loss is pkg.softmax_loss and "softmax_loss" in pkg.__all__ and "bpr_loss" in pkg.__all__
    with pytest.raises(ValueError, match="cand"):
        hip_ops.softmax_loss(Z, 10, u, cand[:, :1])
    with pytest.raises(ValueError, match="cand"):
        hip_ops.softmax_loss(Z, 10, u, cand.to(torch.int32))
    with pytest.raises(ValueError, match="cand"):
        hip_ops.softmax_loss(Z, 10, u, cand.reshape(-1))
    with pytest.raises(ValueError, match="u "):
        hip_ops.softmax_loss(Z, 10, u[:9], cand)
    with pytest.raises(ValueError, match="temperature"):
        hip_ops.softmax_loss(Z, 10, u, cand, temperature=0.0)


def test_sampler_has_sample_candidates(pkg):
    sig = inspect.signature(pkg.sampler.BPRSampler.sample_candidates)
    assert list(sig.parameters) == ["self", "samples", "n_neg", "seed", "offset"]
    assert sig.parameters["seed"].default == 42 and sig.parameters["offset"].default == 0
