"""bench.py's options and its --dump-outputs writer, on CPU tensors (the GPU run writes the same way from device memory)."""
import os
import sys

import numpy as np
import torch

import bench


def test_plain_run_is_the_default_and_full_is_an_option(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    args = bench.parse()
    assert (args.steps, args.warmup, args.full, args.dump_outputs) == (7, 2, False, None)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out"])
    args = bench.parse()
    assert args.full and args.dump_outputs == "out"


def test_dump_outputs_writes_the_whole_small_slab(tmp_path):
    out = torch.arange(1000 + 24, dtype=torch.float32) * 0.5          # padded like bench.Run.out
    bench.dump_outputs(str(tmp_path), out, 300, 1000, 1, 0)
    field, index = np.load(tmp_path / "field.npy"), np.load(tmp_path / "field_index.npy")
    assert field.dtype == np.float32 and index.dtype == np.float64
    assert np.array_equal(field, out[:1000].numpy())
    assert np.array_equal(index, np.arange(300, 1300, dtype=np.float64))


def test_dump_outputs_samples_a_large_slab_the_same_way_every_time(tmp_path):
    count, start = 50_000, 7_000
    out = torch.arange(count + 256, dtype=torch.float32)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), out, start, count, 2, 1, points=4096)
    assert sorted(os.listdir(tmp_path / "a")) == ["field_index_rank1.npy", "field_rank1.npy"]
    fa, ia = np.load(tmp_path / "a" / "field_rank1.npy"), np.load(tmp_path / "a" / "field_index_rank1.npy")
    assert np.array_equal(fa, np.load(tmp_path / "b" / "field_rank1.npy"))
    assert np.array_equal(ia, np.load(tmp_path / "b" / "field_index_rank1.npy"))
    assert 0 < fa.size <= 4096 and fa.size == ia.size and np.all(np.diff(ia) > 0)
    assert ia.min() >= start and ia.max() < start + count
    assert np.array_equal(fa, (ia - start).astype(np.float32))            # each value sits at its recorded index


def test_default_dump_stays_within_64_mb():
    assert bench.DUMP_POINTS * (4 + 8) <= 64 * 2 ** 20
