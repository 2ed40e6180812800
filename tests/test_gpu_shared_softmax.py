"""Shared-negatives softmax loss on the GPU (hip_ops.shared_softmax_loss): parity against the
float64 reference (tests/_shs_ref.py) evaluated on the same fp32 Z, the two sharp cases, tile edges,
the cross-check with the per-positive kernel, the pool precondition, bad indices, bitwise
repeatability (debug library included), graph capture, the hand-off to the layer below and the
trainer.  The tests print their figures and record them through conftest.write_report; DESIGN.md
section 18 has the table."""
import functools
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import _shs_ref as ref
import _ssm_ref
from conftest import ROOT, write_report

pytestmark = pytest.mark.gpu

TOL = 1e-5
UP = ref.Reference.UPSTREAM  # the upstream gradient
NU = ref.N_USERS


@pytest.fixture(scope="module")
def hip_ops(pkg):
    return importlib.import_module(pkg.__name__ + ".hip_ops")


@functools.lru_cache(maxsize=None)
def _case(P, C, tau, seed=0, z_std=0.1, S=ref.N_SAMPLES, history=True):
    """Inputs and the float64 reference of one case, computed once and shared (never modified)."""
    return ref.Reference(P, C, tau, seed=seed, z_std=z_std, S=S, history=history)


def _run(hip_ops, r, dev, upstream=UP, pool=None, u=None, pos=None):
    Zg = r.Z.to(dev).requires_grad_(True)
    hist = None if r.ptr is None else (r.ptr.to(dev), r.items.to(dev))
    loss = hip_ops.shared_softmax_loss(Zg, NU, (r.u if u is None else u).to(dev), (r.pos if pos is None else pos).to(dev),
                                       (r.pool if pool is None else pool).to(dev), r.tau, history=hist)
    (dZ,) = torch.autograd.grad(loss, Zg, torch.tensor(upstream, device=dev))
    return loss.detach(), dZ


def _figures(r, loss, dZ, abs_floor=0.0):
    lrel = abs(float(loss.double().cpu() - r.loss)) / max(abs(float(r.loss)), 1e-300)
    drow, zmax = ref.scaled_rows(dZ, r.dZ, r.scale, abs_floor)
    return {"P": r.P, "C": r.C, "tau": r.tau, "S": int(r.u.numel()), "loss_rel": lrel, "dZ_row_over_scale": drow,
            "zero_rows_max": zmax}


@pytest.mark.parametrize("P,C,tau", ref.CASES)
def test_parity(hip_ops, cuda, P, C, tau):
    r = _case(P, C, tau)
    loss, dZ = _run(hip_ops, r, cuda)
    hip_ops.check_bpr_indices()
    fig = _figures(r, loss, dZ)
    print("[shs parity]", fig)
    write_report(f"shs_parity_P{P}_C{C}_tau{tau}", fig)
    assert bool(torch.isfinite(dZ).all())
    assert int((r.scale == 0).sum()) >= 1
    assert fig["loss_rel"] <= TOL, fig
    assert fig["dZ_row_over_scale"] <= TOL and fig["zero_rows_max"] == 0.0, fig


@pytest.mark.parametrize("which", ["sharp", "extreme"])
def test_sharp_cases(hip_ops, cuda, which):
    """(300, 128, tau = 0.02), and tau = 0.01 with Z ~ 0.5 N(0, 1) (logits of about +-900).  The bound
    on dZ is 4 x the fp32 CPU restatement's own figure on the same inputs, never the kernel's;
    ref.UNDERFLOW_ABS is the absolute allowance for softmax weights no fp32 number holds.  (The
    extreme case's seed is one where float64 autograd itself is sound: on most draws a positive
    wins by so much that its "p0 - 1" cancels to 0 in float64, _shs_ref.EXTREME_SEED.)"""
    (P, C, tau), seed, z_std = ((ref.SHARP, ref.SHARP_SEED, 0.1) if which == "sharp" else
                                (ref.EXTREME, ref.EXTREME_SEED, 0.5))
    r = _case(P, C, tau, seed=seed, z_std=z_std)
    _, r32 = r.restatement(ref.UNDERFLOW_ABS)
    bound = 4.0 * r32
    loss, dZ = _run(hip_ops, r, cuda)
    fig = dict(_figures(r, loss, dZ, ref.UNDERFLOW_ABS), restatement=r32, bound=bound)
    print("[shs sharp]", which, fig)
    write_report(f"shs_{which}", fig)
    assert bool(torch.isfinite(dZ).all()) and bool(torch.isfinite(loss))
    assert fig["loss_rel"] <= TOL, fig
    assert fig["dZ_row_over_scale"] <= bound and fig["zero_rows_max"] == 0.0, fig


EDGES = ([(S, 129, True) for S in (1, 255, 257)] + [(ref.N_SAMPLES, P, True) for P in (1, 31, 32, 33, 1500)] +
         [(40, 1000, True), (ref.N_SAMPLES, 129, False)])


@pytest.mark.parametrize("S,P,history", EDGES, ids=[f"S{S}_P{P}" + ("" if h else "_nohist") for S, P, h in EDGES])
def test_tile_edges(hip_ops, cuda, S, P, history):
    """C = 64 against float64: sample counts around the 128-sample tile and the 256-sample loss block,
    pools around the 32-item mask word, the whole catalogue as the pool (every positive is in it),
    few samples against many pool tiles (the pool range is split over blocks), no history."""
    r = _case(P, 64, 1.0, S=S, history=history)
    loss, dZ = _run(hip_ops, r, cuda)
    hip_ops.check_bpr_indices()
    fig = _figures(r, loss, dZ)
    print("[shs edge]", fig)
    assert fig["loss_rel"] <= TOL and fig["dZ_row_over_scale"] <= TOL and fig["zero_rows_max"] == 0.0, fig
    if P == 1500:
        assert bool(r.mask.any(dim=1).all())


def test_empty_batch(hip_ops, cuda):
    r = _case(129, 64, 1.0, S=0)
    loss, dZ = _run(hip_ops, r, cuda)
    assert float(loss) == 0.0 and dZ.shape == r.Z.shape and float(dZ.abs().max()) == 0.0


@pytest.mark.parametrize("C", [64, 128])
def test_agrees_with_the_per_positive_kernel(hip_ops, cuda, C):
    """A pool disjoint from every positive, no history: the same loss as softmax_loss on
    cand = [pos | pool repeated for every sample], within the parity bounds."""
    r0 = _case(129, C, 1.0, history=False)
    free = np.setdiff1d(np.arange(ref.N_ITEMS), r0.pos.numpy())
    pool = torch.from_numpy(np.sort(np.random.default_rng(4).choice(free, 16, replace=False)).astype(np.int64))
    loss, dZ = _run(hip_ops, r0, cuda, pool=pool)
    cand = torch.cat([r0.pos.unsqueeze(1), pool.unsqueeze(0).expand(r0.pos.numel(), 16)], 1).contiguous()
    Zg = r0.Z.to(cuda).requires_grad_(True)
    l2 = hip_ops.softmax_loss(Zg, NU, r0.u.to(cuda), cand.to(cuda), 1.0)
    (dZ2,) = torch.autograd.grad(l2, Zg, torch.tensor(UP, device=cuda))
    scale = _ssm_ref.term_scale(r0.Z, NU, r0.u, cand, 1.0, upstream=UP)
    lrel = abs(float(loss) - float(l2.detach())) / abs(float(l2.detach()))
    drow, zmax = ref.scaled_rows(dZ, dZ2, scale)
    print("[shs cross]", C, lrel, drow)
    assert lrel <= TOL and drow <= TOL and zmax == 0.0, (lrel, drow, zmax)


def test_pool_precondition_and_bad_indices(hip_ops, cuda):
    hip_ops.check_bpr_indices()
    r = _case(33, 64, 1.0)
    swapped = r.pool.clone()
    swapped[[3, 4]] = swapped[[4, 3]]
    dup = r.pool.clone()
    dup[10] = dup[9]
    for bad in (swapped, dup):
        loss, dZ = _run(hip_ops, r, cuda, pool=bad)
        assert bool(torch.isfinite(dZ).all())
        with pytest.raises(ValueError, match="ascending"):
            hip_ops.check_bpr_indices()
        hip_ops.check_bpr_indices()  # the pending counts were consumed
    past = torch.cat([r.pool[:-1], torch.tensor([ref.N_ITEMS])])  # still ascending
    loss, dZ = _run(hip_ops, r, cuda, pool=past)
    assert bool(torch.isfinite(dZ).all())  # clamped, not read out of range
    with pytest.raises(IndexError):
        hip_ops.check_bpr_indices()
    upast = r.u.clone()
    upast[7] = NU
    _run(hip_ops, r, cuda, u=upast)
    with pytest.raises(IndexError):
        hip_ops.check_bpr_indices()
    _run(hip_ops, r, cuda)
    hip_ops.check_bpr_indices()


def test_repeat_gives_the_same_bits(hip_ops, cuda):
    for P, C, tau in ((1000, 128, 0.1), (1000, 64, 0.1)):
        r = _case(P, C, tau)
        a = _run(hip_ops, r, cuda)
        b = _run(hip_ops, r, cuda)
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    r = _case(1000, 64, 1.0, S=40)  # the split pool range
    assert all(torch.equal(x, y) for x, y in zip(_run(hip_ops, r, cuda), _run(hip_ops, r, cuda)))


DEBUG_SNIPPET = r"""
import sys, importlib
import numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import _shs_ref as ref
pkg = importlib.import_module("plotpointe-gat-recommendation_amd")
hip_ops = importlib.import_module(pkg.__name__ + ".hip_ops")
assert pkg._lib.debug_build()
P, C, tau = 1000, 128, 0.1
Z, u, pos, pool, ptr, items = ref.make_case(P, C)
Zg = Z.cuda().requires_grad_(True)
loss = hip_ops.shared_softmax_loss(Zg, ref.N_USERS, u.cuda(), pos.cuda(), pool.cuda(), tau, history=(ptr.cuda(), items.cuda()))
(dZ,) = torch.autograd.grad(loss, Zg, torch.tensor(3.0, device="cuda"))
np.savez(sys.argv[2], loss.detach().cpu().numpy(), dZ.cpu().numpy())
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
    got = _run(hip_ops, _case(1000, 128, 0.1), cuda)
    with np.load(tmp_path / "d.npz") as z:
        for k, t in enumerate(got):
            assert np.array_equal(z[f"arr_{k}"], t.cpu().numpy()), k


def test_capture_replays_eager_bits(hip_ops, cuda):
    """A captured forward + backward replayed twice gives the eager bits."""
    r = _case(1000, 128, 0.1)
    u, pos, pool, hist = r.u.to(cuda), r.pos.to(cuda), r.pool.to(cuda), (r.ptr.to(cuda), r.items.to(cuda))
    Zs = r.Z.to(cuda).requires_grad_(True)
    up = torch.tensor(UP, device=cuda)

    def step():
        loss = hip_ops.shared_softmax_loss(Zs, NU, u, pos, pool, r.tau, history=hist)
        (dZ,) = torch.autograd.grad(loss, Zs, up)
        return loss.detach(), dZ

    eager = [t.clone() for t in step()]
    side = torch.cuda.Stream(cuda)
    side.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream(cuda).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = step()
    for _ in range(2):
        for t in static:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        diff = [float((a.double() - b.double()).abs().max()) for a, b in zip(static, eager)]
        assert all(torch.equal(a, b) for a, b in zip(static, eager)), diff


def test_layer_below_takes_its_ordinary_prologue(pkg, hip_ops, cuda):
    """Two-layer PyGGAT(hidden = 64) on the cfg1 graph: parameter gradients through
    shared_softmax_loss(Z).backward() against a second identical forward followed by
    Z.backward(dZ_ref), dZ_ref the float64 reference gradient of the loss at that Z cast to fp32 --
    every parameter within 1e-5 of its max-abs."""
    train = importlib.import_module(pkg.__name__ + ".train")
    cfg = train.Config("p", "r", "s", "g", "e", "m", hidden_dim=64, layers=2, attn_dropout=0.0)
    tr, va, te, n_users, n_items, feats_np = train.load_inputs(cfg, "cfg1")
    ei = pkg.data.build_edge_index(n_users, n_items, tr).to(cuda)
    feats = torch.tensor(feats_np, dtype=torch.float32, device=cuda)
    torch.manual_seed(3)
    model = train.build_model(cfg, n_users, n_items, feats.size(1)).to(cuda).eval()
    ptr, flat = train.user_csr(tr, n_users)
    smp = pkg.sampler.BPRSampler(ptr, flat, n_items, device=cuda)
    u, pos, _ = smp.sample(3000, seed=9)
    pool = smp.sample_pool(min(200, n_items), seed=5)
    Z = model(feats, ei)
    loss = hip_ops.shared_softmax_loss(Z, n_users, u, pos, pool, 0.5, history=smp)
    model.zero_grad(set_to_none=True)
    loss.backward()
    got = {k: p.grad.detach().clone() for k, p in model.named_parameters()}
    mask = ref.dense_mask(u.cpu(), pos.cpu(), pool.cpu(), smp.ptr.cpu(), smp.items.cpu()[:smp.nnz], n_items=n_items)
    assert bool(mask.any())
    _, dZ64 = ref.loss_autograd(Z.detach().cpu(), n_users, u.cpu(), pos.cpu(), pool.cpu(), mask, 0.5)
    Z2 = model(feats, ei)
    assert torch.equal(Z2, Z)
    model.zero_grad(set_to_none=True)
    Z2.backward(dZ64.float().to(cuda))
    fig = {}
    for k, p in model.named_parameters():
        fig[k] = float((got[k] - p.grad).abs().max() / p.grad.abs().max().clamp_min(1e-30))
    print("[shs handoff]", fig)
    write_report("shs_handoff", fig)
    assert set(fig) == set(got) and all(v <= TOL for v in fig.values()), fig


def test_sample_pool(pkg, cuda):
    smp = pkg.sampler.BPRSampler(np.array([0, 2, 3]), np.array([1, 5, 2]), 1000, device=cuda)
    a, b, c = smp.sample_pool(256, seed=3), smp.sample_pool(256, seed=3), smp.sample_pool(256, seed=4)
    assert a.dtype == torch.int64 and a.device.type == "cuda" and a.shape == (256,)
    assert bool((a[1:] > a[:-1]).all()) and int(a[0]) >= 0 and int(a[-1]) < 1000
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert torch.equal(smp.sample_pool(1000, seed=1), torch.arange(1000, device=cuda))
    with pytest.raises(ValueError):
        smp.sample_pool(1001)


def test_trainer(pkg, cuda, tmp_path, capsys):
    train = importlib.import_module(pkg.__name__ + ".train")
    out = train.main(["--synthetic", "cfg1", "--epochs", "2", "--loss", "softmax", "--shared-negatives", "256",
                      "--eval-neg-k", "100", "--device-eval", "--models-prefix", str(tmp_path)])
    assert "256 negatives shared" in out["notes"] and "--negatives unused" in out["notes"]
    log = capsys.readouterr().out
    losses = [float(v) for v in re.findall(r"\] loss=(\S+) \(softmax\)", log)]
    print("losses", losses)
    assert len(losses) == 2 and all(np.isfinite(losses)) and losses[1] <= losses[0], losses
    with pytest.raises(ValueError, match="catalogue"):
        train.main(["--synthetic", "cfg1", "--epochs", "1", "--loss", "softmax", "--shared-negatives", "100000000",
                    "--models-prefix", str(tmp_path)])
