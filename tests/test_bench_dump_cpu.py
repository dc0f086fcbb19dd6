"""bench.py's --dump-outputs files and --steps, without a GPU: the sample is fixed, bounded and decodes the packed colours."""
import os
import sys

import numpy as np
import pytest

import bench


def _load(d, suffix=""):
    return {k: np.load(os.path.join(d, f"{k}{suffix}.npy"), allow_pickle=False) for k in ("index", "rgb", "has")}


def test_dump_is_a_fixed_bounded_sample_of_the_packed_colours(tmp_path):
    n = 3_000_000
    packed = np.random.default_rng(3).integers(0, 1 << 25, n, dtype=np.uint32)
    bench.dump_outputs(str(tmp_path / "a"), packed, 0, 1)
    bench.dump_outputs(str(tmp_path / "b"), packed.copy(), 0, 1)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 64 << 20
    assert a["index"].dtype == np.float64 and a["rgb"].dtype == np.float32 and a["has"].dtype == np.float32
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    idx = a["index"].astype(np.int64)
    assert len(idx) == bench.DUMP_MAX_POINTS and np.all(np.diff(idx) > 0) and 0 <= idx[0] and idx[-1] < n
    w = packed[idx]
    assert np.array_equal(a["rgb"], np.stack([w & 255, (w >> 8) & 255, (w >> 16) & 255], axis=1).astype(np.float32))
    assert np.array_equal(a["has"], (w >> 24).astype(np.float32))


def test_dump_of_a_small_cloud_holds_every_point_and_ranks_write_their_own_files(tmp_path):
    packed = np.arange(1000, dtype=np.uint32) | (1 << 24)
    bench.dump_outputs(str(tmp_path), packed, 0, 1)
    d = _load(tmp_path)
    assert np.array_equal(d["index"], np.arange(1000)) and np.all(d["has"] == 1)
    bench.dump_outputs(str(tmp_path), packed, 1, 2)
    assert np.array_equal(_load(tmp_path, "_rank1")["index"], np.arange(1000))


def test_steps_sets_the_timed_steps(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "7", "--warmup", "0"])
    args = bench.parse()
    assert args.steps == 7 and args.warmup == 0 and args.dump_outputs is None
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse()


def test_full_is_off_by_default(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "5", "--warmup", "2"])
    assert bench.parse().full is False
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "5", "--warmup", "2", "--full"])
    assert bench.parse().full is True
