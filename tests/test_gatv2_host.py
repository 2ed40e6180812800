"""GATv2Conv without a GPU: the float64 reference's own consistency, the module's constructor,
state_dict and refusals, and the ABI's argument validation (no device work) -- CPU."""
import ctypes
import importlib
import inspect

import numpy as np
import pytest
import torch

import _gatv2_ref as ref


def test_reference_formulas_equal_autograd():
    """The explicit backward the kernels implement == float64 autograd of the restated forward."""
    for heads, channels, masked in ((2, 8, True), (1, 8, False), (4, 4, True)):
        assert ref.self_check(heads, channels, masked) <= 2e-14


def test_reference_graph_facts():
    ei = ref.make_graph()
    ind, outd = np.bincount(ei[1], minlength=ref.N_NODES), np.bincount(ei[0], minlength=ref.N_NODES)
    assert 6500 <= ei.shape[1] <= 7100
    assert {k: int(ind[k]) for k in ref.IN_DEGREES} == ref.IN_DEGREES
    assert outd[1] >= 700 and ind[880:].sum() == 0 and outd[880:].sum() == 0


def test_constructor_defaults_are_pygs(pkg):
    sig = inspect.signature(pkg.GATv2Conv.__init__).parameters
    want = dict(heads=1, concat=True, negative_slope=0.2, dropout=0.0, add_self_loops=True, edge_dim=None,
                fill_value="mean", bias=True, share_weights=False, residual=False)
    assert {k: sig[k].default for k in want} == want
    assert list(sig)[1:3] == ["in_channels", "out_channels"]
    assert pkg.GATv2Conv is importlib.import_module(pkg.__name__ + ".conv").GATv2Conv


def test_state_dict_keys_and_init(pkg):
    torch.manual_seed(0)
    conv = pkg.GATv2Conv(48, 64, heads=2, concat=False, add_self_loops=False)
    sd = conv.state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == {
        "att": (1, 2, 64), "bias": (64,), "lin_l.weight": (128, 48), "lin_l.bias": (128,),
        "lin_r.weight": (128, 48), "lin_r.bias": (128,)}
    assert sd["lin_l.weight"].data_ptr() != sd["lin_r.weight"].data_ptr()
    assert not torch.equal(sd["lin_l.weight"], sd["lin_r.weight"])
    for k in ("bias", "lin_l.bias", "lin_r.bias"):
        assert float(sd[k].abs().max()) == 0.0
    a = (6.0 / (48 + 128)) ** 0.5  # glorot
    for k in ("lin_l.weight", "lin_r.weight"):
        assert 0.9 * a < float(sd[k].abs().max()) <= a
    assert 0.5 * (6.0 / (2 + 64)) ** 0.5 < float(sd["att"].abs().max()) <= (6.0 / (2 + 64)) ** 0.5
    assert len(list(conv.parameters())) == 6


def test_share_weights_aliases_lin_r(pkg):
    conv = pkg.GATv2Conv(32, 32, heads=1, concat=False, add_self_loops=False, share_weights=True)
    assert conv.lin_r is conv.lin_l
    sd = conv.state_dict()
    assert sorted(sd) == ["att", "bias", "lin_l.bias", "lin_l.weight", "lin_r.bias", "lin_r.weight"]
    assert sd["lin_r.weight"].data_ptr() == sd["lin_l.weight"].data_ptr()
    assert sd["lin_r.bias"].data_ptr() == sd["lin_l.bias"].data_ptr()
    assert len(list(conv.parameters())) == 4
    other = pkg.GATv2Conv(32, 32, heads=1, concat=False, add_self_loops=False, share_weights=True)
    other.load_state_dict(sd)
    assert torch.equal(other.lin_r.weight, conv.lin_l.weight)


def test_bias_false_removes_all_three(pkg):
    conv = pkg.GATv2Conv(32, 64, heads=2, concat=False, add_self_loops=False, bias=False)
    assert sorted(conv.state_dict()) == ["att", "lin_l.weight", "lin_r.weight"]
    assert conv.bias is None and conv.lin_l.bias is None and conv.lin_r.bias is None


@pytest.mark.parametrize("kw", [dict(), dict(concat=False), dict(concat=False, add_self_loops=False, edge_dim=4),
                                dict(concat=False, add_self_loops=False, residual=True),
                                dict(concat=True, add_self_loops=False)])
def test_refused_options(pkg, kw):
    with pytest.raises(NotImplementedError):
        pkg.GATv2Conv(64, 64, **kw)


def test_refused_shapes(pkg):
    with pytest.raises(NotImplementedError):
        pkg.GATv2Conv((64, 64), 64, concat=False, add_self_loops=False)
    hip_ops = importlib.import_module(pkg.__name__ + ".hip_ops")
    for h, c in ref.SHAPES:
        assert hip_ops.gatv2_supported(h, c)
        pkg.GATv2Conv(16, c, heads=h, concat=False, add_self_loops=False)
    for h, c in ((3, 64), (8, 64), (2, 32), (1, 256), (1, 48), (0, 64)):
        assert not hip_ops.gatv2_supported(h, c)
        with pytest.raises(NotImplementedError):
            pkg.GATv2Conv(16, c, heads=h, concat=False, add_self_loops=False)


def test_abi_return_codes(pkg):
    lib = pkg._lib.load()
    assert lib.ppgat_version() == 3
    nb = ctypes.c_size_t(0)
    assert lib.ppgat_dynatt_workspace_bytes(10, 0, 0, 3, 64, 0, ctypes.byref(nb)) == 2
    assert lib.ppgat_dynatt_workspace_bytes(10, 0, 0, 2, 64, 0, None) == 1
    assert lib.ppgat_dynatt_workspace_bytes(1000, 5, 7, 2, 64, 0, ctypes.byref(nb)) == 0
    assert nb.value >= 5 * 2 * (64 + 4) * 4
    assert lib.ppgat_dynatt_workspace_bytes(1000, 5, 7, 2, 64, 1, ctypes.byref(nb)) == 0
    assert nb.value >= 1000 * 2 * 16 + 7 * 128 * 4
    s = pkg._lib.Schedule(None, None, None, 0, 0, None, None, 0, -1)
    fwd = lambda h, c, p: lib.ppgat_dynatt_fwd(ctypes.byref(s), None, None, 0, 0, h, c, None, None, None, None, 0.2,
                                               p, 0, None, None, None, None, None, 0, None)
    bwd = lambda h, c, p: lib.ppgat_dynatt_bwd(ctypes.byref(s), ctypes.byref(s), None, None, None, None, 0, 0, h, c,
                                               None, None, None, None, None, None, 0.2, p, None, None, None, None,
                                               None, None, 0, None)
    assert fwd(3, 64, 0.0) == 2 and b"(heads, channels)" in lib.ppgat_last_error()
    assert bwd(1, 256, 0.0) == 2
    assert fwd(2, 64, 1.0) == 1 and b"[0, 1)" in lib.ppgat_last_error()
    assert fwd(2, 64, float("nan")) == 1
    assert bwd(2, 64, 1.5) == 1
    assert fwd(2, 64, 0.5) == 1 and b"seed_used" in lib.ppgat_last_error()  # dropout without the seed slot
    assert lib.ppgat_dynatt_fwd(None, None, None, 0, 0, 2, 64, None, None, None, None, 0.2, 0.0, 0, None, None, None,
                                None, None, 0, None) == 1  # null schedule


def test_cpu_tensors_raise(pkg):
    hip_ops = importlib.import_module(pkg.__name__ + ".hip_ops")
    x = torch.zeros(4, 64)
    with pytest.raises(RuntimeError, match="ROCm"):
        hip_ops.gatv2_aggregate(x, x, torch.zeros(1, 64), torch.zeros(64), None, 1, 64, 0.2)
    with pytest.raises(RuntimeError, match="ROCm"):
        pkg.gatv2_aggregate(x, x, torch.zeros(1, 64), None, None, 1, 64, 0.2)


def test_model_keys_and_cli_options(pkg):
    m = pkg.PyGGATv2(7, 5, item_feat_dim=12, hidden=64, layers=2, heads=2, attn_dropout=0.1)
    want = {"user_emb.weight", "item_proj.weight", "item_proj.bias"}
    for l in range(2):
        want |= {f"convs.{l}.{k}" for k in ("att", "bias", "lin_l.weight", "lin_l.bias", "lin_r.weight", "lin_r.bias")}
    assert set(m.state_dict()) == want
    shared = pkg.PyGGATv2(7, 5, item_feat_dim=12, hidden=64, layers=1, heads=1, attn_dropout=0.0, share_weights=True)
    assert shared.convs[0].lin_r is shared.convs[0].lin_l
    shared.load_state_dict(shared.state_dict())
    train = importlib.import_module(pkg.__name__ + ".train")
    args = train.build_parser().parse_args(["--model-family", "gatv2_pyg", "--share-weights"])
    assert args.model_family == "gatv2_pyg" and args.share_weights is True
    assert train.build_parser().parse_args([]).share_weights is False
    cfg = train.Config("p", "r", "s", "g", "e", "m", hidden_dim=64, layers=1, heads=2, model_family="gatv2_pyg",
                       share_weights=True)
    built = train.build_model(cfg, 7, 5, 12)
    assert isinstance(built, pkg.PyGGATv2) and built.convs[0].share_weights and built.convs[0].heads == 2
    with pytest.raises(NotImplementedError):
        train.main(["--model-family", "gatv2_pyg", "--world-size", "2", "--synthetic", "cfg1"])
