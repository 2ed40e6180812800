"""Fan-out neighbour sampling, the parts that need no GPU: the numpy reference checks itself, the
rule is uniform over positions and pairs, the epoch seeds, the ABI's refusals (nothing launched),
the trainer's refusals -- CPU."""
import ctypes
import importlib
import itertools

import numpy as np
import pytest

import _nsample_ref as ref

M64 = (1 << 64) - 1


def _nb(pkg):
    return importlib.import_module(pkg.__name__ + ".neighbors")


# ---- the reference checks itself ---------------------------------------------------------
def _floyd_sets(seed, i, d, f, draw64):
    """Floyd's algorithm written again: Python integers, a set, the package's host draw64."""
    chosen = set()
    for s in range(f):
        j = d - f + s
        t = (draw64(seed, i, s) * (j + 1)) >> 64
        chosen.add(j if t in chosen else t)
    return chosen


def test_floyd_agrees_with_a_set_based_version(pkg):
    draw64 = _nb(pkg).draw64
    rng = np.random.default_rng(5)
    for _ in range(1000):
        f = int(rng.integers(1, 65))
        d = f + int(rng.integers(1, 2000)) if rng.random() < 0.8 else f + 1
        i, seed = int(rng.integers(0, 1 << 40)), int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(0, 2))
        got = ref.floyd(seed, i, d, f)
        assert len(got) == f and set(got) == _floyd_sets(seed, i, d, f, draw64), (seed, i, d, f)
        assert ref.floyd_rows(seed, np.array([i]), np.array([d]), np.array([f]))[0].tolist() == got


def test_every_row_keeps_min_d_f_distinct_positions():
    rng = np.random.default_rng(6)
    n = 400
    deg = rng.integers(0, 200, n)
    deg[:4] = [0, 1, 64, 65]
    dst = np.repeat(np.arange(n), deg)
    ei = np.stack([rng.integers(0, n, len(dst)), dst])
    ei = ei[:, rng.permutation(ei.shape[1])]
    fo = rng.integers(-1, 65, n).astype(np.int32)
    for fanout, fanout_of in ((1, None), (7, None), (64, None), (5, fo)):
        keep, ei_s, eid = ref.sample(ei, n, fanout, 42, fanout_of)
        f = ref.caps(deg, fanout, fanout_of)
        assert np.array_equal(np.bincount(ei_s[1], minlength=n), np.minimum(deg, f))
        assert np.array_equal(ei_s, ei[:, keep]) and np.array_equal(eid, np.flatnonzero(keep))
        assert (np.diff(eid) > 0).all()
    S = ref.floyd_rows(3, np.arange(n), np.full(n, 100), rng.integers(1, 65, n))
    for row in S:
        v = row[row >= 0]
        assert len(set(v.tolist())) == len(v) and (v < 100).all()


# ---- the rule is uniform --------------------------------------------------------------
Z_CAP = 4.5
CASES = [(20000, 10, 3, 42), (20000, 10, 3, 7), (20000, 65, 64, 42), (20000, 5, 1, 42), (4000, 1000, 64, 42),
         (20000, 12, 6, 1)]


@pytest.mark.parametrize("n,d,f,seed", CASES)
def test_positions_and_pairs_are_uniform(n, d, f, seed):
    """n rows of in-degree d: position p is kept n f / d times in expectation, a pair of positions
    n f (f - 1) / (d (d - 1)) times; rows are independent, so the counts are binomial."""
    S = ref.floyd_rows(seed, np.arange(n), np.full(n, d), np.full(n, f))
    assert (S >= 0).all() and (S < d).all()
    kept = np.zeros((n, d), bool)
    kept[np.arange(n)[:, None], S] = True
    assert (kept.sum(1) == f).all()
    p = f / d
    z = (kept.sum(0) - n * p) / np.sqrt(n * p * (1 - p))
    print(f"(n={n}, d={d}, f={f}, seed={seed}): max |z| over positions {np.abs(z).max():.2f}")
    assert np.abs(z).max() <= Z_CAP
    if (d, f) in ((10, 3), (12, 6)):
        p2 = f * (f - 1) / (d * (d - 1))
        z2 = [((kept[:, a] & kept[:, b]).sum() - n * p2) / np.sqrt(n * p2 * (1 - p2))
              for a, b in itertools.combinations(range(d), 2)]
        print(f"(n={n}, d={d}, f={f}, seed={seed}): max |z| over pairs {np.abs(z2).max():.2f}")
        assert np.abs(z2).max() <= Z_CAP


# ---- library and trainer ---------------------------------------------------------------
def test_epoch_seed_is_a_draw_of_the_stream(pkg):
    nb = _nb(pkg)
    from oracle.sampler_oracle import draw64
    for seed, e in ((42, 0), (42, 1), (0, 0), (M64, 0), (M64, 7), (123456789012345678, 1000)):
        want = int(draw64(seed, np.uint64(e), 1023))
        assert nb.epoch_seed(seed, e) == want == ref.epoch_seed(seed, e), (seed, e)
        assert nb.draw64(seed, e, 3) == int(draw64(seed, np.uint64(e), 3))
    # an additive epoch offset would alias (epoch e + 1, row t) with (epoch e, row t + 1); the draw does not
    assert nb.draw64(nb.epoch_seed(42, 1), 0, 0) != nb.draw64(nb.epoch_seed(42, 0), 1, 0)
    assert nb.MAX_FANOUT == ref.MAX_FANOUT == 64


def test_abi_refusals_launch_nothing(pkg):
    lib = pkg._lib.load()
    assert lib.ppgat_neighbor_max_fanout() == 64
    p = ctypes.c_void_p(256)  # never dereferenced: every call below is refused on the host
    for fanout in (0, -1, 65, 1000):
        assert lib.ppgat_neighbor_count(p, 10, 20, fanout, None, p, p, p, 1 << 20, None) == 2
        assert b"fanout" in lib.ppgat_last_error()
    assert lib.ppgat_neighbor_count(p, -1, 20, 5, None, p, p, p, 1 << 20, None) == 1
    assert lib.ppgat_neighbor_count(p, 10, -1, 5, None, p, p, p, 1 << 20, None) == 1
    assert lib.ppgat_neighbor_count(p, 1 << 31, 20, 5, None, p, p, p, 1 << 20, None) == 2
    for args in ((None, 10, 20, 5, None, p, p, p), (p, 10, 20, 5, None, None, p, p), (p, 10, 20, 5, None, p, None, p),
                 (p, 10, 20, 5, None, p, p, None)):
        assert lib.ppgat_neighbor_count(*args, 1 << 20, None) == 1, args
    assert lib.ppgat_neighbor_count(p, 10, 20, 5, None, p, p, p, 0, None) == 1
    assert b"workspace" in lib.ppgat_last_error()
    # sample: sizes, n_kept > n_edges, each required pointer
    ok = [p, p, p, p, p, 10, 20, 0, p, 15, p, p, p, p, p, 1 << 20, None]
    for pos, val in ((5, -1), (6, -1), (9, -1), (9, 21)):
        a = list(ok)
        a[pos] = val
        assert lib.ppgat_neighbor_sample(*a) == 1, (pos, val)
    for pos in (0, 1, 2, 3, 4, 8, 10, 11, 12, 13, 14):
        a = list(ok)
        a[pos] = None
        assert lib.ppgat_neighbor_sample(*a) == 1, pos
    # derive
    ok = [p, p, p, p, 10, 20, 15, p, p, p, p, p, p, 1 << 20, None]
    for pos, val in ((4, -1), (5, -1), (6, -1), (6, 21)):
        a = list(ok)
        a[pos] = val
        assert lib.ppgat_neighbor_derive(*a) == 1, (pos, val)
    for pos in (0, 1, 2, 3, 7, 8, 9, 10, 11, 12):
        a = list(ok)
        a[pos] = None
        assert lib.ppgat_neighbor_derive(*a) == 1, pos
    with pytest.raises(NotImplementedError):
        pkg._lib.check(lib.ppgat_neighbor_count(p, 10, 20, 65, None, p, p, p, 1 << 20, None), "neighbor_count")


def test_workspace_query_is_host_only(pkg):
    lib = pkg._lib.load()
    n = ctypes.c_size_t(0)
    assert lib.ppgat_neighbor_sample_workspace_bytes(1000, 5000, ctypes.byref(n)) == 0
    assert n.value >= 5000 * (2 + 3 * 4)  # the two keep-flag arrays and the three per-edge maps
    small = n.value
    assert lib.ppgat_neighbor_sample_workspace_bytes(1000, 50000, ctypes.byref(n)) == 0 and n.value > small
    assert lib.ppgat_neighbor_sample_workspace_bytes(100000, 0, ctypes.byref(n)) == 0 and n.value >= 100001 * 4
    assert lib.ppgat_neighbor_sample_workspace_bytes(-1, 0, ctypes.byref(n)) == 1
    assert lib.ppgat_neighbor_sample_workspace_bytes(10, -1, ctypes.byref(n)) == 1
    assert lib.ppgat_neighbor_sample_workspace_bytes(10, 10, None) == 1


def test_python_layer_refuses_cpu_tensors_and_bad_fanout(pkg):
    import torch
    ei = torch.tensor([[0, 1], [1, 2]])
    with pytest.raises(RuntimeError, match="ROCm"):
        pkg.sample_neighbors(ei, 3, 5, 42)
    with pytest.raises(RuntimeError, match="ROCm"):
        pkg.NeighborSampler(ei, 3, 5)
    assert callable(pkg.hip_ops.graph_cache.put) and callable(pkg.hip_ops.graph_cache.drop)


def test_trainer_refuses_fanout_where_it_cannot_run(pkg):
    train = importlib.import_module(pkg.__name__ + ".train")
    with pytest.raises(NotImplementedError, match="fanout"):
        train.main(["--synthetic", "cfg1", "--fanout", "5", "--model-family", "lightgcn"])
    with pytest.raises(NotImplementedError, match="fanout"):
        train.main(["--synthetic", "cfg1", "--fanout", "5", "--world-size", "2"])
    for bad in (["--fanout", "65"], ["--fanout", "-1"], ["--fanout-items", "3"], ["--fanout", "5", "--fanout-items", "65"],
                ["--fanout", "5", "--resample-every", "0"]):
        with pytest.raises(ValueError):
            train.main(["--synthetic", "cfg1"] + bad)
    args = train.build_parser().parse_args([])
    assert args.fanout == 0 and args.fanout_items is None and args.resample_every == 1
