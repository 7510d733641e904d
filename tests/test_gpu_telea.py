"""--inpaint-mode opencv on the GPU (csrc/telea_kernels.hip through the C-ABI): the kernel executes the level replay of the
plan, and the result equals the float32 statement of OpenCV's Telea fill (tests/_telea_statement.py) BIT FOR BIT -- with
contraction off every operation on both sides is a correctly rounded fp32 add, multiply, divide or square root in the same
order.  tests/test_telea_plan.py ties the plan and its numpy level replay to the serial statement without a GPU."""
import time

import numpy as np
import pytest
import torch

from tests import _telea_statement as S
from tests.test_telea_plan import CASE_NAMES

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine(built_lib, gpu_device):
    from vsr_amd.engine import TeleaEngine

    eng = TeleaEngine(device=0, max_plans=16)
    yield eng
    eng.close()


def _run(engine, frames, mask):
    d = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    engine.inpaint(d, mask)
    torch.cuda.synchronize()
    return d.cpu().numpy()


@pytest.mark.parametrize("name", CASE_NAMES)
@pytest.mark.parametrize("kind", ["random", "smooth"])
def test_kernel_equals_serial_statement(engine, name, kind):
    img, mask, want, _ = S.serial_case(name, kind)
    got = _run(engine, img[None], mask)[0]
    assert np.array_equal(got[mask == 0], img[mask == 0]), "unmasked pixels are never touched"
    diff = got != want
    print(f"{name}/{kind}: {int(diff.sum())} of {int((mask != 0).sum()) * 3} values differ from the float32 statement")
    assert not diff.any()


@pytest.fixture(scope="module")
def full_hd(built_lib, engine):
    """one 1080p frame under the benchmark's mask: the numpy level replay (float32) of the C++ plan, once per module"""
    mask = S.benchmark_mask()
    img = S.smooth_image(1080, 1920, seed=7)
    t0 = time.perf_counter()
    h = engine.plan(mask)
    t_plan = time.perf_counter() - t0
    plan = S.plan_schedule(built_lib.lib, h, mask)
    t0 = time.perf_counter()
    want = S.replay(img, plan, np.float32)
    hist = np.bincount(plan["level"])[1:]
    print(f"1080p benchmark mask: {len(plan['yx'])} pixels, {plan['levels']} levels, pixels per level mean {hist.mean():.1f} median "
          f"{np.median(hist):.0f} min {hist.min()} max {hist.max()}, levels of <= 2 pixels {(hist <= 2).mean():.3f}; plan build + upload "
          f"{t_plan:.2f} s, numpy replay {time.perf_counter() - t0:.1f} s")
    return img, mask, want


def test_kernel_equals_level_replay_at_1080p(engine, full_hd):
    img, mask, want = full_hd
    got = _run(engine, img[None], mask)[0]
    assert np.array_equal(got[mask == 0], img[mask == 0])
    diff = got != want
    print(f"1080p: {int(diff.sum())} of {int((mask != 0).sum()) * 3} values differ from the float32 replay")
    assert not diff.any()


def test_batch_of_50_is_deterministic_and_independent(engine, full_hd):
    """frame i of a 50-frame batch == the same frame run alone == a second run, bit for bit"""
    img, mask, want = full_hd
    rng = np.random.default_rng(50)
    batch = np.empty((50, 1080, 1920, 3), np.uint8)
    batch[:] = img
    for i in range(1, 50):                                  # every frame differs under and around the mask
        batch[i, 860:1080] = rng.integers(0, 256, (220, 1920, 3), dtype=np.uint8) if i % 2 else np.roll(img[860:1080], 7 * i, 1)
    d = torch.from_numpy(batch).cuda()
    engine.inpaint(d, mask)
    first = d.cpu().numpy()
    assert np.array_equal(first[0], want)
    unmasked = mask == 0
    assert all(np.array_equal(first[i][unmasked], batch[i][unmasked]) for i in range(50))
    d2 = torch.from_numpy(batch).cuda()
    engine.inpaint(d2, mask)
    assert torch.equal(d, d2), "a second run gives the same bytes"
    for i in (1, 24, 49):
        assert np.array_equal(_run(engine, batch[i][None], mask)[0], first[i]), f"frame {i} alone == frame {i} of the batch"
    view = torch.from_numpy(batch).cuda()[3:11]             # a slice of a resident clip: in place, the frames around it untouched
    engine.inpaint(view, mask)
    assert np.array_equal(view.cpu().numpy(), first[3:11])


def test_out_argument_and_strided_frames(engine):
    img, mask, want, _ = S.serial_case("two_overlapping", "random")
    src = torch.from_numpy(np.stack([img, img[::-1].copy()])).cuda()
    out = torch.zeros_like(src)
    res = engine.inpaint(src, mask, out=out)
    torch.cuda.synchronize()
    assert res.data_ptr() == out.data_ptr() and np.array_equal(src[0].cpu().numpy(), img), "the source is left alone"
    assert np.array_equal(out[0].cpu().numpy(), want)
    wide = torch.zeros((2, 2) + tuple(img.shape), dtype=torch.uint8, device="cuda")    # frame stride of two frames
    wide[:, 0] = src
    engine.inpaint(wide[:, 0], mask)
    assert torch.equal(wide[:, 0], out) and not wide[:, 1].any()


def test_two_plugin_lanes_equal_one(built_lib, gpu_device):
    from vsr_amd.backend.inpaint.opencv_inpaint import OpenCVInpaint
    from vsr_amd.backend.tools import batch_lanes

    img, mask, want, _ = S.serial_case("hole", "smooth")
    rng = np.random.default_rng(2)
    clip = rng.integers(0, 256, (24,) + img.shape, dtype=np.uint8)
    clip[0] = img
    plugin = OpenCVInpaint("cuda:0")
    cache = {}
    try:
        one = torch.from_numpy(clip).cuda()
        for s in range(0, 24, 5):
            assert plugin(one[s:s + 5], mask) is not None
        torch.cuda.synchronize()
        two = torch.from_numpy(clip).cuda()
        plugins = batch_lanes.lane_plugins(plugin, 2, cache)
        assert len(plugins) == 2 and plugins[1] is not plugin
        batch_lanes.run_jobs([(two[s:s + 5], mask) for s in range(0, 24, 5)], plugins, two.device)
        torch.cuda.synchronize()
        assert torch.equal(one, two)
        assert np.array_equal(one[0].cpu().numpy(), want)
        host = plugin([f for f in clip[:3]], mask)          # the reference's list contract on the real engine
        assert all(np.array_equal(h, one[i].cpu().numpy()) for i, h in enumerate(host)) and np.array_equal(clip[0], img)
    finally:
        plugin.close()
        for clones in cache.values():
            for p in clones:
                p.close()


def test_alternating_masks_equal_fresh_engines(built_lib, gpu_device):
    """an interval's mask comes back after another one: plan cache eviction and reuse change nothing"""
    from vsr_amd.engine import TeleaEngine

    a = S.serial_case("rect", "random")
    b_mask = np.zeros_like(a[1])
    b_mask[5:30, 30:60] = 255
    rng = np.random.default_rng(9)
    frames = rng.integers(0, 256, (8,) + a[0].shape, dtype=np.uint8)
    frames[0] = a[0]
    for max_plans in (1, 2):
        eng = TeleaEngine(device=0, max_plans=max_plans)
        got = []
        for i in range(8):
            got.append(_run(eng, frames[i][None], a[1] if i % 2 == 0 else b_mask)[0])
        assert eng.plan_builds == (8 if max_plans == 1 else 2)
        eng.close()
        for i in range(8):
            fresh = TeleaEngine(device=0)
            assert np.array_equal(_run(fresh, frames[i][None], a[1] if i % 2 == 0 else b_mask)[0], got[i])
            fresh.close()
        assert np.array_equal(got[0], a[2])


def test_radius_other_than_3_runs_the_generic_kernel(built_lib, gpu_device):
    from vsr_amd.engine import TeleaEngine

    img, mask, _, _ = S.serial_case("line", "smooth")
    want, _ = S.serial(img, mask, radius=2)
    eng = TeleaEngine(device=0, radius=2)
    assert np.array_equal(_run(eng, img[None], mask)[0], want)
    eng.close()


def _read_all(path):
    from vsr_amd.backend.tools import video_io

    r = video_io.Y4mVideo(path)
    out = []
    while True:
        ok, fr = r.read()
        if not ok:
            break
        out.append(fr)
    r.release()
    return np.stack(out)


def test_run_opencv_mode_file_to_file(built_lib, gpu_device, tmp_path, monkeypatch):
    """*.y4m in -> SubtitleRemover.run() with config.inpaintMode = OPENCV and an injected detector -> *.y4m out: the written file
    is the statement applied frame by frame with the intervals' masks, on the HBM-resident path and on the host-frames path."""
    from vsr_amd import synth
    from vsr_amd.backend.config import config
    from vsr_amd.backend.inpaint.opencv_inpaint import OpenCVInpaint
    from vsr_amd.backend.main import SubtitleRemover
    from vsr_amd.backend.tools import video_io
    from vsr_amd.backend.tools.constant import InpaintMode

    H, W, N = 240, 432, 34
    box = (190, 210, 80, 300)                               # ymin, ymax, xmin, xmax
    clip = synth.make_clip(N, H, W, box, seed=5)
    on = [i for i in range(N) if 3 <= i < 15 or i >= 22]
    plain = synth.make_clip(N, H, W, (0, 1, 0, 1), seed=5)
    for i in range(N):
        if i not in on:
            clip[i] = plain[i]
    src = str(tmp_path / "in.y4m")
    monkeypatch.setenv("VSR_IO_COLOR", "host")
    monkeypatch.delenv("VSR_OPENCV_BACKEND", raising=False)
    w = video_io.Y4mWriter(src, 25.0, (W, H), chroma="420")
    for f in clip:
        w.write(f)
    w.release()
    decoded = _read_all(src)
    quad = np.array([[[box[2], box[0]], [box[3], box[0]], [box[3], box[1]], [box[2], box[1]]]])

    class Det:
        batch_size = 4

        def predict(self, img):
            white = (img[box[0] + 4:box[1] - 4, box[2] + 8:box[3] - 8] > 200).mean()
            return [{"dt_polys": quad if white > 0.05 else np.zeros((0, 4, 2), np.int32)}]

    calls = []

    class Recording(OpenCVInpaint):
        def __call__(self, frames, mask):
            if isinstance(frames, torch.Tensor):            # a slice of the resident clip: its place in the clip is its frame number
                first = frames.storage_offset() // (H * W * 3)
            else:                                           # host frames are the decoded input frames themselves
                first = next(i for i in range(N) if np.array_equal(decoded[i], frames[0]))
                assert all(np.array_equal(decoded[first + k], f) for k, f in enumerate(frames))
            calls.append((first, len(frames), np.array(mask, copy=True)))
            return super().__call__(frames, mask)

    old_mode, old_load = config.inpaintMode.value, config.sttnMaxLoadNum.value
    outs, batches = {}, {}
    plugin = Recording("cuda:0")
    try:
        config.inpaintMode.value = InpaintMode.OPENCV
        config.sttnMaxLoadNum.value = 8
        for how, color, resident in (("host", "host", "0"), ("resident", "device", "1")):
            monkeypatch.setenv("VSR_IO_COLOR", color)
            monkeypatch.setenv("VSR_IO_RESIDENT", resident)
            del calls[:]
            sr = SubtitleRemover(src, device="cuda:0")
            sr.sub_areas = [(0, H, 0, W)]
            sr.text_detector = Det()
            sr.opencv_inpaint = plugin
            sr.video_out_path = str(tmp_path / f"out_{how}.y4m")
            sr.run()
            outs[how] = open(sr.video_out_path, "rb").read()
            batches[how] = list(calls)
    finally:
        config.inpaintMode.value, config.sttnMaxLoadNum.value = old_mode, old_load
        plugin.close()
    assert outs["host"] == outs["resident"], "the HBM-resident loop must write the host loop's file"
    assert [(f, n, m.tobytes()) for f, n, m in batches["host"]] == [(f, n, m.tobytes()) for f, n, m in batches["resident"]]
    assert batches["resident"] and all(m.shape == (H, W) and m.any() for _, _, m in batches["resident"])
    from vsr_amd.engine import TeleaEngine

    host_eng = TeleaEngine(device=None)
    expected = decoded.copy()                               # frames outside the intervals pass through
    serial_checked = False
    for first, n, m in batches["resident"]:
        plan = S.plan_schedule(built_lib.lib, host_eng.plan(m), m)
        for k in range(first, first + n):
            expected[k] = S.replay(decoded[k], plan)        # (tests/test_telea_plan.py: the replay of the plan == the serial statement)
            if not serial_checked:
                assert np.array_equal(expected[k], S.serial(decoded[k], m)[0])
                serial_checked = True
    host_eng.close()
    want_path = str(tmp_path / "want.y4m")
    ww = video_io.Y4mWriter(want_path, 25.0, (W, H))          # the run's own sink: open_writer's Y4mWriter, 4:4:4
    for f in expected:
        ww.write(f)
    ww.release()
    assert open(want_path, "rb").read() == outs["resident"], "the file is the statement applied with the intervals' masks"
    covered = np.zeros(N, bool)
    for first, n, _ in batches["resident"]:
        covered[first:first + n] = True
    assert covered[on].all(), "every frame with the subtitle on screen was inpainted"


def test_matches_cv2_if_present(engine):
    """the only place parity with OpenCV itself is pinned; skipped wherever opencv-python is absent"""
    cv2 = pytest.importorskip("cv2")
    for name in CASE_NAMES:
        mask = S.mask_cases()[name]
        img = S.smooth_image(*mask.shape, seed=3)
        want = cv2.inpaint(img, mask, 3, cv2.INPAINT_TELEA)
        assert np.array_equal(_run(engine, img[None], mask)[0], want), name
