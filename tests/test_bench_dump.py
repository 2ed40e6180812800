"""bench.py --dump-outputs: the writer behind it (host logic; the benchmark itself needs a GPU)."""
import importlib.util
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]


def _bench():
    spec = importlib.util.spec_from_file_location("ppgat_bench", ROOT / "bench.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_outputs_writes_float32_and_samples_large_arrays(tmp_path):
    bench = _bench()
    rows = 3 * bench.DUMP_ARRAY_BYTES // (4 * 128) + 7   # over the per-array limit, not a multiple of it
    big = torch.arange(rows, dtype=torch.float64).view(-1, 1).expand(rows, 128)
    arrays = {"loss": torch.tensor(0.25), "Z": big, "param.w": torch.ones(5, 3, dtype=torch.float64)}
    first = bench.dump_outputs(str(tmp_path / "a"), arrays)
    second = bench.dump_outputs(str(tmp_path / "b"), arrays)
    assert first == second == {"loss": [1, 1], "Z": [bench.DUMP_ARRAY_BYTES // 512, rows], "param.w": [5, 5]}
    total = 0
    for name in arrays:
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert a.dtype == np.float32 and np.array_equal(a, b)
        total += a.nbytes
    assert total <= bench.DUMP_TOTAL_BYTES
    z = np.load(tmp_path / "a" / "Z.npy")
    assert z.shape == (bench.DUMP_ARRAY_BYTES // 512, 128) and z.nbytes <= bench.DUMP_ARRAY_BYTES
    # the sample is whole rows of the array, distinct and in order
    assert (z == z[:, :1]).all() and (np.diff(z[:, 0]) > 0).all() and z[-1, 0] < rows
    assert float(np.load(tmp_path / "a" / "loss.npy")[0]) == 0.25
