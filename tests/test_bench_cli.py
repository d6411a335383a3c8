"""bench.py without a GPU: a plain run is the lean one, and --dump-outputs writes seeded float32 samples within its size limit."""
import numpy as np
import pytest
import torch

import bench


def test_side_measurements_are_opt_in():
    a = bench.parse_args(["--gpus", "1", "--steps", "3", "--warmup", "1"])
    assert (a.gpus, a.steps, a.warmup, a.full, a.dump_outputs) == (1, 3, 1, False, None)
    a = bench.parse_args(["--full", "--dump-outputs", "out"])
    assert a.full and a.dump_outputs == "out"


def test_dump_outputs_seeded_float32_and_capped(tmp_path):
    t = torch.arange(1000, dtype=torch.float64).reshape(100, 10)
    s = bench.seeded_rows(t, 16, 0)
    assert torch.equal(s, bench.seeded_rows(t, 16, 0)) and s.shape == (16, 10)
    rows = (s[:, 0] / 10).long()
    assert bool((rows[1:] > rows[:-1]).all())                     # distinct rows, in index order
    assert bench.seeded_rows(t, 100, 0) is t
    bench.write_outputs(str(tmp_path / "out"), {"maps": bench.to_host(s), "loss": np.array([0.5, 1.0])})
    got = np.load(tmp_path / "out" / "maps.npy")
    assert got.dtype == np.float32 and np.array_equal(got, s.numpy().astype(np.float32))
    assert np.load(tmp_path / "out" / "loss.npy").dtype == np.float32
    with pytest.raises(ValueError):
        bench.write_outputs(str(tmp_path / "big"), {"x": np.zeros(bench.DUMP_LIMIT_BYTES // 4 + 1, np.float32)})
    assert not (tmp_path / "big").exists()
