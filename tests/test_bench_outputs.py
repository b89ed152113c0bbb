"""bench.py --dump-outputs without a GPU: how the outputs of the last timed step are written (bench.write_outputs) -- float32
.npy files, whole when they fit the 64 MB budget, otherwise the same fixed, seeded sample of pixels from every array."""
import os

import numpy as np

import bench


def _images(h, w, seed=7):
    g = np.random.default_rng(seed)
    return {"rgb8": g.integers(0, 256, (h, w, 3), dtype=np.uint8), "accum": g.random((h * w, 3), dtype=np.float32)}


def test_outputs_within_the_budget_are_written_whole(tmp_path):
    arrays = _images(20, 30)
    assert bench.write_outputs(str(tmp_path), arrays) == ["accum", "rgb8"]
    assert sorted(os.listdir(tmp_path)) == ["accum.npy", "rgb8.npy"]
    for k, a in arrays.items():
        got = np.load(tmp_path / f"{k}.npy")
        assert got.dtype == np.float32 and got.shape == a.shape and np.array_equal(got, a.astype(np.float32))


def test_larger_outputs_keep_one_fixed_sample_of_pixels(tmp_path):
    arrays = _images(64, 96)
    limit = 20000
    names = bench.write_outputs(str(tmp_path / "a"), arrays, limit=limit)
    bench.write_outputs(str(tmp_path / "b"), _images(64, 96), limit=limit)
    assert names == ["accum", "pixel_index", "rgb8"]
    got = {k: np.load(tmp_path / "a" / f"{k}.npy") for k in names}
    assert sum(a.nbytes for a in got.values()) <= limit
    idx = got["pixel_index"]
    assert idx.dtype == np.float64 and np.all(np.diff(idx) > 0) and 0 <= idx[0] and idx[-1] < 64 * 96
    assert len(idx) == limit // (12 + 12 + 8)
    i = idx.astype(np.int64)
    assert np.array_equal(got["rgb8"], arrays["rgb8"].reshape(-1, 3)[i].astype(np.float32))
    assert np.array_equal(got["accum"], arrays["accum"][i])
    for k in names:  # the same arguments give the same sample
        assert np.array_equal(got[k], np.load(tmp_path / "b" / f"{k}.npy"))
