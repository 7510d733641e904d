"""bench.py --dump-outputs without a GPU: dump_outputs() on host frames (the files two builds are compared by)."""
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_are_float32_seeded_and_bounded(tmp_path, monkeypatch):
    monkeypatch.setenv("HSA_ENABLE_IPC_MODE_LEGACY", os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))   # bench.py sets it on import
    monkeypatch.syspath_prepend(ROOT)
    import bench

    assert 4 * (bench.DUMP_BOX_ELEMS + bench.DUMP_FRAME_ELEMS) <= 64 << 20
    frames = torch.randint(0, 256, (4, 60, 80, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(0))
    box = (20, 40, 8, 72)
    bench.dump_outputs(str(tmp_path / "whole"), frames, box)
    got = np.load(tmp_path / "whole" / "inpainted_box.npy")
    assert got.dtype == np.float32 and np.array_equal(got, frames[:, 20:40, 8:72].numpy())

    monkeypatch.setattr(bench, "DUMP_BOX_ELEMS", 1000)
    monkeypatch.setattr(bench, "DUMP_FRAME_ELEMS", 500)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), frames, box)
    # capped: the sorted positions drawn from the fixed seed, taken from the box / from the whole frames
    for name, src, cap, seed in (("inpainted_box", frames[:, 20:40, 8:72], 1000, 11), ("frames_sample", frames, 500, 12)):
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        idx = np.sort(np.random.default_rng(seed).integers(0, src.numel(), cap))
        want = src.reshape(-1).numpy()[idx].astype(np.float32)
        assert a.dtype == np.float32 and np.array_equal(a, want) and np.array_equal(a, b)
    assert sorted(os.listdir(tmp_path / "a")) == ["frames_sample.npy", "inpainted_box.npy"]
