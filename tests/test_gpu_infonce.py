"""ppgat_infonce and ppgat_relu_dropout on the GPU, called directly (fusion.infonce,
fusion.relu_dropout) and compared with the references of tests/_infonce_ref.py.

InfoNCE: the loss triple and every row of dF, dT, dI against torch autograd in float64 of the
formulae in csrc/ppgat_infonce.hip's header.  The gradients are judged by conftest.row_rel (per-row
2-norm relative error, per matrix: fused rows span six decades, so a per-matrix max-abs metric
would hide the small ones), the loss relatively.  The bound is not a constant: the same figures are
computed for a plain fp32 torch restatement on the CPU, and the kernel must stay within 4x of them
-- it sums in other, but fixed, orders.  One floor under that: a figure of the restatement below
the fp32 unit roundoff 2^-24 counts as 2^-24, because rounding the exact answer to fp32 already
costs up to that, and a scalar such as the loss lands closer than that only by luck.

ReLU/dropout: both directions bitwise against the numpy restatement (mask from
oracle.mlp_dropout_scale), on +0, -0, denormals, negatives and positives."""
import numpy as np
import pytest
import torch

import _infonce_ref as iref
from conftest import row_rel, write_report

pytestmark = pytest.mark.gpu

NAMES = ("dF", "dT", "dI")


def _kernel(pkg, cuda, F, T, I, tau):
    out = pkg.fusion.infonce(F.to(cuda), T.to(cuda), I.to(cuda), tau)
    assert all(o.dtype == torch.float32 and o.is_cuda for o in out)
    assert tuple(out[0].shape) == (3,) and all(tuple(o.shape) == tuple(F.shape) for o in out[1:])
    return tuple(o.cpu() for o in out)


def _figures(got, want):
    """{'loss': relative error of the triple, 'dF' / 'dT' / 'dI': (worst row_rel, its row, zero-row max)}."""
    fig = {"loss": iref.loss_rel(got[0].double().numpy(), want[0].numpy())}
    for name, a, b in zip(NAMES, got[1:4], want[1:4]):
        fig[name] = row_rel(a, b)
    return fig


def _judge(name, kern, rest, extra=None):
    """The 4x rule on every figure, after writing both sides to the parity report."""
    rec = {"loss": {"kernel": kern["loss"], "fp32_restatement": rest["loss"]}}
    for n in NAMES:
        rec[n] = {"kernel": kern[n][0], "kernel_row": kern[n][1], "fp32_restatement": rest[n][0],
                  "fp32_restatement_row": rest[n][1], "kernel_zero_rows_max_abs": kern[n][2]}
    rec.update(extra or {})
    write_report(name, rec)
    assert kern["loss"] <= 4 * max(rest["loss"], iref.U32), rec
    for n in NAMES:
        assert kern[n][0] <= 4 * max(rest[n][0], iref.U32), (n, rec)
        assert kern[n][2] == 0.0, (n, rec)      # rows the reference has exactly zero come out zero


# both temperatures up to B = 65; above that 0.01 on a subset
B_LADDER = [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 257, 511, 513, 1025, 4096]
CASES = [(B, 0.07) for B in B_LADDER] + [(B, 0.01) for B in B_LADDER if B <= 65 or B in (257, 1025)]


@pytest.mark.parametrize("B,tau", CASES)
def test_infonce_rows_vs_fp64(pkg, cuda, B, tau):
    F, T, I = iref.batch(B)
    want = iref.infonce(F.double(), T.double(), I.double(), tau)
    rest = _figures(iref.infonce(F, T, I, tau), want)
    got = _kernel(pkg, cuda, F, T, I, tau)
    assert all(torch.isfinite(g).all() for g in got)
    _judge(f"infonce_b{B}_tau{tau}", _figures(got, want), rest, {"B": B, "tau": tau})
    if B == 1:
        assert all((g == 0).all() for g in got)     # one row: the loss and every gradient are exactly 0
    if B in (33, 513):                               # the same call again: bitwise the same
        again = _kernel(pkg, cuda, F, T, I, tau)
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(got, again))


def test_infonce_aligned_batch(pkg, cuda):
    """F = T + 0.01 noise, I likewise: softmax - onehot cancels to about 1e-4 of its terms, so a
    row's error is judged absolutely on the scale of the terms it sums, 1 / (2 B tau |x_b|) (the
    precedent is conftest.dx_rows), and the loss -- lse - diagonal, both near 1 / tau -- absolutely
    on the scale of the row maxima.  Same 4x rule against the fp32 restatement."""
    B, tau = 64, 0.07
    F, T, I = iref.aligned_batch(B)
    want = iref.infonce(F.double(), T.double(), I.double(), tau)
    rest = iref.infonce(F, T, I, tau)
    got = _kernel(pkg, cuda, F, T, I, tau)
    top = float(want[4].max())
    assert float(want[0][0]) < 1e-2 * top            # the loss is far below the logits it is made of
    rec = {"B": B, "tau": tau, "loss_ref": float(want[0][0]), "row_max": top}
    bad = []
    for name, x, k in (("loss", None, 0), ("dF", F, 1), ("dT", T, 2), ("dI", I, 3)):
        if x is None:
            fk = float((got[0].double() - want[0]).abs().max()) / top
            fr = float((rest[0].double() - want[0]).abs().max()) / top
        else:
            fk = iref.term_scale_rows(got[k], want[k], x, B, tau)
            fr = iref.term_scale_rows(rest[k], want[k], x, B, tau)
            # the cancellation is real: the exact rows are far below the scale they are judged on
            assert iref.term_scale_rows(torch.zeros_like(want[k]), want[k], x, B, tau) < 1e-2
        rec[name] = {"kernel": fk, "fp32_restatement": fr}
        # the 2^-24 floor only where it is earned: the logits are fp32 numbers of the row maxima's
        # size, so the loss cannot be known better than that; the rows are held to the restatement alone
        if not fk <= 4 * (max(fr, iref.U32) if x is None else fr):
            bad.append(name)
    write_report("infonce_aligned_b64", rec)
    assert not bad, (bad, rec)


def test_infonce_zero_rows(pkg, cuda):
    """One row of fused and one of txt_p exactly zero: the |x| <= 1e-12 branch gives dy / 1e-12.
    Everything finite, and every row within the 4x rule of the fp64 reference written with the same clamp."""
    B, tau = 48, 0.07
    F, T, I = iref.batch(B, seed=11)
    F[7] = 0.0
    T[20] = 0.0
    want = iref.infonce(F.double(), T.double(), I.double(), tau)
    rest = _figures(iref.infonce(F, T, I, tau), want)
    got = _kernel(pkg, cuda, F, T, I, tau)
    assert all(torch.isfinite(g).all() for g in got)
    assert float(want[1][7].norm()) > 1e8 and float(want[2][20].norm()) > 1e8     # dy / 1e-12
    _judge("infonce_zero_rows_b48", _figures(got, want), rest, {"B": B, "tau": tau})
    for k, r in ((1, 7), (2, 20)):
        e = float((got[k][r].double() - want[k][r]).norm() / want[k][r].norm())
        assert e <= 4 * max(rest[NAMES[k - 1]][0], iref.U32), (k, r, e)


def test_infonce_refusals(pkg, cuda):
    z = torch.zeros(4097, 128, device=cuda)
    with pytest.raises(NotImplementedError, match="1 <= batch <= 4096"):
        pkg.fusion.infonce(z, z, z)
    with pytest.raises(NotImplementedError, match="dim 128"):
        pkg.fusion.infonce(z[:8, :64].contiguous(), z[:8, :64].contiguous(), z[:8, :64].contiguous())


def _z_values(n, rng):
    z = (rng.standard_normal(n) * 3).astype(np.float32)
    special = np.array([0.0, -0.0, 1e-40, -1e-40, 1.4e-45, -1.4e-45, 1.1754942e-38, -2.5, 3.0], np.float32)
    pos = rng.permutation(n)[:min(n, len(special) * 3)]
    z[pos] = np.resize(special, len(pos))
    return z


@pytest.mark.parametrize("p", [0.0, 0.3, 0.999])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 70001])
def test_relu_dropout_bitwise(pkg, oracle, cuda, n, p):
    rng = np.random.default_rng(n)
    z = _z_values(n, rng)
    if n == 1:
        z[0] = 1e-40                            # the one element: a positive denormal, which passes
    g = (rng.standard_normal(n) * 2).astype(np.float32)
    g[::7] = -0.0
    seed = 0x5EED0000 + n
    zd = torch.from_numpy(z).to(cuda)
    a = pkg.fusion.relu_dropout(zd, p, seed)
    want_a = iref.relu_dropout(z, p, seed, oracle.mlp_dropout_scale)
    assert np.array_equal(a.cpu().numpy().view(np.uint32), want_a.view(np.uint32))
    want_g = iref.relu_dropout(z, p, seed, oracle.mlp_dropout_scale, grad=g)
    gd = torch.from_numpy(g.copy()).to(cuda)
    out = pkg.fusion.relu_dropout(zd, p, seed, grad=gd)
    assert out.data_ptr() == gd.data_ptr()      # in place, on the gradient's own values
    assert np.array_equal(gd.cpu().numpy().view(np.uint32), want_g.view(np.uint32))
    assert torch.equal(zd.cpu(), torch.from_numpy(z))
    if n >= 255:
        gate = z > 0
        assert (want_a[~gate].view(np.uint32) == 0).all()             # +0 for -0, negatives and +0
        assert ((want_g != 0) <= gate).all()
        if p == 0.0:
            assert np.array_equal(want_a[gate], z[gate]) and np.array_equal(want_g[gate], g[gate])
        else:
            kept = want_a[gate] != 0
            assert abs(kept.mean() - (1 - p)) < 0.02 + 3.0 / np.sqrt(gate.sum())
