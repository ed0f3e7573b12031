"""CPU tests: bench.py --dump-outputs helpers (frame sample, keypoint table, file types and size limit)."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import bench  # noqa: E402


def test_dump_frames_all_or_a_fixed_sample():
    assert np.array_equal(bench.dump_frames(256, 1000), np.arange(256))
    s = bench.dump_frames(128, 1 << 20)
    assert len(s) == 64 and np.all(np.diff(s) > 0) and s.max() < 128
    assert np.array_equal(s, bench.dump_frames(128, 1 << 20))   # depends on the arguments alone
    assert len(bench.dump_frames(4, bench.DUMP_LIMIT * 2)) == 1


def test_kp_table_is_exact():
    from orb_slam3_amd import KP_DTYPE
    k = np.zeros(3, KP_DTYPE)
    k["x"], k["y"], k["angle"], k["octave"], k["class_id"] = [1.5, 700.25, 3], [2, 3, 4], [359.9, 0, 12.5], [0, 7, 3], -1
    t = bench.kp_table(k.view(np.uint8).reshape(3, 28))
    assert t.dtype == np.float32 and t.shape == (3, 7)
    assert np.array_equal(t[:, 0], k["x"]) and np.array_equal(t[:, 5], k["octave"]) and np.all(t[:, 6] == -1)
    assert bench.kp_table(np.zeros((0, 28), np.uint8)).shape == (0, 7)


def test_save_dump_types_and_limit(tmp_path):
    info = bench.save_dump(tmp_path / "d", {"frame_index": np.arange(3.0), "x": np.ones((2, 2), np.float32)})
    assert info["files"] == ["frame_index", "x"] and info["frames"] == 3 and info["bytes"] == 24 + 16
    assert np.array_equal(np.load(tmp_path / "d" / "x.npy"), np.ones((2, 2), np.float32))
    with pytest.raises(AssertionError):
        bench.save_dump(tmp_path / "e", {"frame_index": np.arange(3.0), "n": np.arange(3)})
    with pytest.raises(AssertionError):
        bench.save_dump(tmp_path / "f", {"frame_index": np.zeros(bench.DUMP_LIMIT // 8 + 1)})
