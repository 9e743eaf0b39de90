"""bench.py --dump-outputs without a GPU: dump_outputs() against a stand-in for the backend's art_download."""
import os

import numpy as np

import bench


class FakeBackend:
    def __init__(self, H, W):
        rng = np.random.default_rng(5)
        self.accum = rng.random((H, W, 3), dtype=np.float32) * 40.0
        self.screen = rng.integers(0, 1 << 24, (H, W), dtype=np.uint32)

    def download(self, spp, want_screen=True):
        return self.accum.copy(), self.screen.copy()


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_small_frame_is_written_whole(tmp_path):
    be = FakeBackend(36, 64)
    bench.dump_outputs(be, 12, str(tmp_path))
    out = _load(str(tmp_path))
    assert sorted(out) == ["accum", "screen_rgb", "spp"]
    assert np.array_equal(out["accum"], be.accum) and out["spp"].tolist() == [12.0]
    s = be.screen
    assert np.array_equal(out["screen_rgb"], np.stack([s & 255, (s >> 8) & 255, (s >> 16) & 255], -1).astype(np.float32))


def test_large_frame_is_a_fixed_sample_within_the_budget(tmp_path):
    be = FakeBackend(1500, 2000)                         # 3 M pixels x 24 B = 72 MB of float32 output: over the budget
    bench.dump_outputs(be, 4, str(tmp_path / "a"))
    bench.dump_outputs(be, 4, str(tmp_path / "b"))
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    assert sum(os.path.getsize(str(tmp_path / "a" / (n + ".npy"))) for n in a) <= bench.DUMP_BUDGET_B
    idx = a["pixel_index"].astype(np.int64)
    assert np.array_equal(idx, a["pixel_index"]) and len(np.unique(idx)) == len(idx) and idx.min() >= 0 and idx.max() < 1500 * 2000
    assert np.array_equal(a["accum"], be.accum.reshape(-1, 3)[idx])
    for n in a:
        assert a[n].dtype in (np.float32, np.float64) and np.array_equal(a[n], b[n]), n
