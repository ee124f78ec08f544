"""bench.py --dump-outputs: the frame is written whole up to the size limit, else as a fixed sample of pixels."""
import os

import numpy as np
import torch

import bench


def test_small_frame_is_written_whole(tmp_path):
    frame = torch.rand((27, 48, 3), dtype=torch.float64)
    assert bench.dump_outputs(str(tmp_path), frame) == ["image.npy"]
    got = np.load(tmp_path / "image.npy")
    assert got.dtype == np.float64 and np.array_equal(got, frame.numpy())


def test_large_frame_is_a_fixed_sample_within_the_limit(tmp_path):
    H, W = 2160, 3840                      # 199 MB of f64
    frame = torch.rand((H, W, 3), dtype=torch.float64)
    names = bench.dump_outputs(str(tmp_path / "a"), frame)
    assert names == ["image_sample.npy", "image_sample_pixel.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in names) <= bench.DUMP_LIMIT_BYTES
    pix = np.load(tmp_path / "a" / "image_sample.npy")
    idx = np.load(tmp_path / "a" / "image_sample_pixel.npy")
    assert pix.shape == (bench.DUMP_SAMPLE_PIXELS, 3) and pix.dtype == np.float64 and idx.dtype == np.float64
    assert len(np.unique(idx)) == len(idx) and idx.min() >= 0 and idx.max() < H * W
    assert np.array_equal(pix, frame.numpy().reshape(H * W, 3)[idx.astype(np.int64)])
    # the same pixels on every run, whatever the frame holds
    bench.dump_outputs(str(tmp_path / "b"), torch.zeros((H, W, 3), dtype=torch.float32))
    assert np.array_equal(np.load(tmp_path / "b" / "image_sample_pixel.npy"), idx)
    assert np.load(tmp_path / "b" / "image_sample.npy").dtype == np.float32
