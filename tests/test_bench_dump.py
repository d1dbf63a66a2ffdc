"""bench.py --dump-outputs on the host: the files it writes, their dtypes and size cap, and that the pixel sample is the
same from run to run and holds the frames' own values.  (The GPU side is bench.py itself: its frames come from the
timed path.)"""
import importlib.util
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
bench = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(bench)


def _frames(V, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (V, H, W, 4), dtype=torch.uint8, generator=g)


def _load(d):
    return np.load(os.path.join(d, "frame_pixels.npy")), np.load(os.path.join(d, "frame_pixel_index.npy"))


def test_small_step_is_written_whole(tmp_path):
    fr = _frames(2, 5, 7, 0)
    bench.dump_outputs(str(tmp_path / "out"), fr)
    px, idx = _load(tmp_path / "out")
    assert px.dtype == np.float32 and idx.dtype == np.float64
    assert np.array_equal(idx, np.arange(2 * 5 * 7))
    assert np.array_equal(px, fr.numpy().reshape(-1, 4).astype(np.float32))


def test_large_step_is_a_fixed_sample_of_its_pixels(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_PIXELS", 1000)
    fr = _frames(3, 40, 60, 1)
    bench.dump_outputs(str(tmp_path / "a"), fr)
    bench.dump_outputs(str(tmp_path / "b"), _frames(3, 40, 60, 2))
    px, idx = _load(tmp_path / "a")
    px_b, idx_b = _load(tmp_path / "b")
    assert px.shape == (1000, 4) and idx.shape == (1000,)
    assert np.array_equal(idx, idx_b)                                   # same pixels whatever the frames hold
    assert np.all(np.diff(idx) > 0) and idx[-1] < 3 * 40 * 60           # distinct, in range
    v, rem = np.divmod(idx.astype(np.int64), 40 * 60)
    y, x = np.divmod(rem, 60)
    assert np.array_equal(px, fr.numpy()[v, y, x].astype(np.float32))
    assert not np.array_equal(px, px_b)


def test_dump_fits_the_size_cap():
    assert bench.DUMP_PIXELS * (4 * 4 + 8) <= 64 * 10**6


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--warmup", "-1"]])
def test_steps_and_warmup_are_checked(monkeypatch, argv):
    monkeypatch.setattr("sys.argv", ["bench.py"] + argv)
    with pytest.raises(SystemExit):
        bench.parse()


def test_steps_warmup_and_dump_dir_are_parsed(monkeypatch):
    monkeypatch.setattr("sys.argv", ["bench.py", "--steps", "3", "--warmup", "1", "--dump-outputs", "d"])
    a = bench.parse()
    assert (a.steps, a.warmup, a.dump_outputs) == (3, 1, "d")
