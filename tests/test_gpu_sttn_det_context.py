"""sttn-det with look-back context frames and scene-bounded intervals on the GPU: the engine's context entry point against the plain
call on the extended list (bit for bit), one oracle anchor, and the two loops of SubtitleRemover.video_inpaint against the definition
(tools/det_lookback.py):

    pieces    SubtitleDetect.split_range_by_scene(intervals, get_scene_div_frame_no(...)); a piece keeps its interval's mask
    batches   batch_generator(frames of the piece, getSttnMaxLoadNum())
    context   the source frames [max(a - N, c), a) of a batch [a, b) in the piece starting at c
    result    the last b - a frames of the plain plugin call STTNDetInpaint.__call__(context ++ batch, mask)
"""
import numpy as np
import pytest
import torch

from vsr_amd import synth
from vsr_amd.backend.tools import video_io
from vsr_amd.backend.tools.det_lookback import det_jobs
from vsr_amd.backend.tools.inpaint_tools import create_mask, get_inpaint_area_by_mask
from oracle.sttn_auto import calculate_psnr
from vsr_amd.synth import make_state_dict

pytestmark = pytest.mark.gpu

H, W = 480, 852
BOX = (150, 400, 50, 800)
SPLIT_H = int(W * 5 / 18)
PSNR_MIN_DB = 50.0      # the bar of tests/test_gpu_sttn.py::test_det_plugin_call_vs_oracle


@pytest.fixture(scope="module")
def sd():
    return make_state_dict(1, "det")


def _mask_and_areas(boxes=(BOX,)):
    mask = create_mask((H, W), [(b[2], b[3], b[0], b[1]) for b in boxes])
    return mask, get_inpaint_area_by_mask(W, H, SPLIT_H, mask[:, :, None])


@pytest.fixture(scope="module")
def engines(built_lib, gpu_device, sd):
    """one engine per arithmetic, default window schedule (stride 5, references every 10)"""
    from vsr_amd.engine import SttnEngine

    made = {}

    def get(mode):
        if mode not in made:
            made[mode] = SttnEngine(sd, "det", device=0, precision=mode)
        return made[mode]

    yield get
    for e in made.values():
        e.close()


@pytest.fixture(scope="module")
def clip19():
    return synth.make_clip(19, H, W, BOX, seed=17)


def _run(eng, dev, frames, mask, areas, context=None):
    d = torch.from_numpy(np.ascontiguousarray(frames)).to(dev)
    c = None if context is None else torch.from_numpy(np.ascontiguousarray(context)).to(dev)
    keep = None if c is None else c.clone()
    eng.det_batch(d, torch.from_numpy(np.ascontiguousarray(mask)).to(dev), areas, mask_host=mask, context=c)
    torch.cuda.synchronize()
    if c is not None:
        assert torch.equal(c, keep), "the context tensor is read-only"
    return d.cpu().numpy()


def _outside(areas):
    rows = np.ones(H, dtype=bool)
    for a in areas:
        rows[a[0]:a[1]] = False
    return rows


@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("mode", ["f32", "f16"])
@pytest.mark.parametrize("n_ctx", [3, 7])
def test_context_call_equals_the_extended_list(built_lib, gpu_device, engines, clip19, n_ctx, mode, lanes):
    """L = 12 frames behind n_ctx context frames: the frames written are frames n_ctx: of the plain call on all n_ctx + 12, bit for
    bit (7 is no multiple of the stride: the window grid sits elsewhere on the written frames)."""
    eng = engines(mode)
    eng.set_lanes(lanes)
    mask, areas = _mask_and_areas()
    ctx, frames = clip19[7 - n_ctx:7], clip19[7:19]
    got = _run(eng, gpu_device, frames, mask, areas, context=ctx)
    want = _run(eng, gpu_device, np.concatenate([ctx, frames]), mask, areas)[n_ctx:]
    assert np.array_equal(got, want)
    out = _outside(areas)
    assert out.any() and np.array_equal(got[:, out], frames[:, out]), "rows outside the inpaint areas are untouched"
    assert (got[:, mask > 0] != frames[:, mask > 0]).any()
    alone = _run(eng, gpu_device, frames, mask, areas)
    assert not np.array_equal(alone, got), "the context changes the fill"


def test_context_call_two_areas(built_lib, gpu_device, engines, clip19):
    eng = engines("f32")
    eng.set_lanes(2)
    mask, areas = _mask_and_areas(((20, 60, 200, 600), (400, 450, 100, 700)))
    assert len(areas) >= 2
    n_ctx = 5
    ctx, frames = clip19[2:7], clip19[7:19]
    got = _run(eng, gpu_device, frames, mask, areas, context=ctx)
    ext = _run(eng, gpu_device, np.concatenate([ctx, frames]), mask, areas)
    assert np.array_equal(got, ext[n_ctx:])
    assert (got != frames).any()


def test_empty_context_is_the_plain_call(built_lib, gpu_device, engines, clip19):
    eng = engines("f32")
    eng.set_lanes(2)
    mask, areas = _mask_and_areas()
    frames = clip19[:12]
    got = _run(eng, gpu_device, frames, mask, areas, context=np.zeros((0, H, W, 3), np.uint8))
    assert np.array_equal(got, _run(eng, gpu_device, frames, mask, areas))


def test_context_call_vs_oracle(built_lib, gpu_device, sd):
    """the one anchor: 3 context + 4 written frames (stride 2, references every 3) against the reference's call on the 7-frame list"""
    from oracle.sttn_det import STTNDetOracle
    from vsr_amd.engine import SttnEngine

    eng = SttnEngine(sd, "det", device=0, neighbor_stride=2, ref_length=3)
    clip = synth.make_clip(7, H, W, BOX, seed=23)
    mask, areas = _mask_and_areas()
    got = _run(eng, gpu_device, clip[3:], mask, areas, context=clip[:3])
    ref = np.stack(STTNDetOracle(sd, 2, 3)(list(clip), mask))[3:]
    strip = ~_outside(areas)
    psnr = calculate_psnr(got[:, strip], ref[:, strip])
    dmax = np.abs(got.astype(int) - ref.astype(int)).max()
    print(f"det context 3 + 4 frames vs oracle: PSNR over the rewritten strip {psnr:.2f} dB, max |d| {dmax}")
    assert np.array_equal(got[:, ~strip], clip[3:][:, ~strip])
    assert psnr >= PSNR_MIN_DB
    assert dmax <= 2
    eng.close()


# ------------------------------------------------------------------------------------------------
# the driver: SubtitleRemover.video_inpaint
# ------------------------------------------------------------------------------------------------
QUAD = np.array([[[BOX[2], BOX[0]], [BOX[3], BOX[0]], [BOX[3], BOX[1]], [BOX[2], BOX[1]]]])


class Det:
    """an injected detector that reports the same box on every frame (the reference's host signature)"""
    batch_size = 4

    def predict(self, img):
        return [{"dt_polys": QUAD}]


class config_values:
    """batches of at most 12 frames, stride 2, references every 3, sttn-det; put back afterwards"""

    def __enter__(self):
        from vsr_amd.backend.config import config
        from vsr_amd.backend.tools.constant import InpaintMode

        self.keys = {"sttnMaxLoadNum": 12, "sttnNeighborStride": 2, "sttnReferenceLength": 3}
        self.old = {k: getattr(config, k).value for k in self.keys}
        self.old_mode = config.inpaintMode.value
        for k, v in self.keys.items():
            getattr(config, k).value = v
        config.inpaintMode.value = InpaintMode.STTN_DET
        assert config.getSttnMaxLoadNum() == 12

    def __exit__(self, *exc):
        from vsr_amd.backend.config import config

        for k, v in self.old.items():
            getattr(config, k).value = v
        config.inpaintMode.value = self.old_mode


@pytest.fixture(scope="module")
def plugin(built_lib, gpu_device, sd):
    from vsr_amd.backend.inpaint.sttn_det_inpaint import STTNDetInpaint

    with config_values():
        return STTNDetInpaint("cuda:0", {"netG": sd})


class Recording:
    """the plugin, with the masks the driver hands it written down"""
    accepts_device_frames = True
    accepts_context = True

    def __init__(self, inner):
        self.inner, self.masks = inner, []

    def __call__(self, frames, mask, context=None):
        self.masks.append(np.array(mask))
        return self.inner(frames, mask, context=context)


def _write_y4m(path, frames):
    w = video_io.Y4mWriter(path, 25.0, (W, H), chroma="444")
    for f in frames:
        w.write(f)
    w.release()


def _read_all(path):
    r = video_io.Y4mVideo(path)
    out = []
    while True:
        ok, fr = r.read()
        if not ok:
            break
        out.append(fr)
    r.release()
    return np.stack(out)


def _records(path):
    """the FRAME records of a *.y4m file, header line dropped"""
    data = open(path, "rb").read()
    return data[data.index(b"\n") + 1:]


def _driver_run(plugin, monkeypatch, src, out, resident="1", context=0, scene_split=False, lanes=1):
    """one file-to-file run of video_inpaint; returns the remover (phase_seconds, scene_cuts)"""
    from vsr_amd.backend.main import SubtitleRemover

    monkeypatch.setenv("VSR_IO_COLOR", "device")
    monkeypatch.setenv("VSR_IO_RESIDENT", resident)
    monkeypatch.setenv("VSR_BATCH_LANES", str(lanes))
    monkeypatch.setenv("VSR_STTN_CONTEXT", str(context))
    monkeypatch.setenv("VSR_SCENE_SPLIT", "1" if scene_split else "0")
    with config_values():
        sr = SubtitleRemover(src, device="cuda:0")
        sr.sub_areas = [(0, sr.frame_height, 0, sr.frame_width)]
        sr.video_out_path = out
        sr.update_progress = lambda tbar, increment: None
        sr.video_inpaint(object(), plugin, text_detector=Det())
        sr.video_writer.release()
    return sr


def test_driver_context_across_batch_seams(built_lib, gpu_device, plugin, tmp_path, monkeypatch):
    """30 frames in one interval, batches 12 / 12 / 6, context 5: the second and third batch look back at source frames 7..11 and
    19..23.  The resident loop (in place: the source rows are copied aside first), the host-frame loop and two plugin instances side
    by side write the same records, and those are the definition's: the plain two-argument plugin call on every batch's extended
    list, read back from the source file."""
    N_FR, N = 30, 5
    src = str(tmp_path / "in.y4m")
    monkeypatch.setenv("VSR_IO_COLOR", "host")
    _write_y4m(src, synth.make_clip(N_FR, H, W, BOX, seed=29))
    frames = _read_all(src)                                # what every loop decodes
    outs, rec = {}, Recording(plugin)
    for mode, resident, lanes in (("resident", "1", 1), ("host", "0", 1), ("lanes2", "1", 2)):
        out = str(tmp_path / f"out_{mode}.y4m")
        sr = _driver_run(rec if mode == "host" else plugin, monkeypatch, src, out, resident=resident, context=N, lanes=lanes)
        assert ("read + upload + YUV->BGR" in sr.phase_seconds) == (resident == "1"), "the loop the test means to run"
        outs[mode] = _records(out)
    # the definition, through the plain plugin call, with the interval's mask (one mask, as today: the context frames get it too)
    assert len(rec.masks) == 3 and all(np.array_equal(x, rec.masks[0]) for x in rec.masks)
    mask = rec.masks[0]
    assert mask.shape == (H, W) and mask.any()
    jobs = det_jobs({1: N_FR}, N_FR, lambda a, b: None, (), N, 12)
    assert [j[:3] for j in jobs] == [(0, 12, 0), (12, 24, 7), (24, 30, 19)]
    expected = frames.copy()
    for lo, hi, ctx_lo, _ in jobs:
        res = plugin(list(frames[ctx_lo:hi]), mask)
        expected[lo:hi] = np.stack(res[lo - ctx_lo:])
    want = str(tmp_path / "want.y4m")
    monkeypatch.setenv("VSR_IO_COLOR", "host")
    w = video_io.open_writer(want, 25.0, (W, H), frames=N_FR)
    for f in expected:
        w.write(f)
    w.release()
    assert outs["resident"] == outs["host"]
    assert outs["resident"] == outs["lanes2"]
    assert outs["resident"] == _records(want)
    plain = str(tmp_path / "plain.y4m")
    _driver_run(plugin, monkeypatch, src, plain, context=0)
    assert _records(plain) != outs["resident"], "the look-back changes what is written"


def test_driver_context_with_two_owners_and_two_lanes(built_lib, gpu_device, plugin, tmp_path, monkeypatch):
    """27 frames at a batch limit of 12 give batches 10 / 10 / 7 (batch_generator shrinks the batch size), so with N = 12 =
    getSttnMaxLoadNum() the third batch looks back at source frames 8..19: rows of the first AND of the second batch, copied aside by
    two owners -- with two lanes from two streams into one buffer.  Two plugin instances side by side, one lane and the host-frame loop
    write the same records, and those are the definition's."""
    N_FR, N = 27, 12
    src = str(tmp_path / "in.y4m")
    monkeypatch.setenv("VSR_IO_COLOR", "host")
    _write_y4m(src, synth.make_clip(N_FR, H, W, BOX, seed=31))
    frames = _read_all(src)
    jobs = det_jobs({1: N_FR}, N_FR, lambda a, b: None, (), N, 12)
    assert [j[:3] for j in jobs] == [(0, 10, 0), (10, 20, 0), (20, 27, 8)]
    outs, rec = {}, Recording(plugin)
    for mode, resident, lanes in (("lanes2", "1", 2), ("resident", "1", 1), ("host", "0", 1), ("lanes2 again", "1", 2)):
        out = str(tmp_path / f"out_{mode.replace(' ', '_')}.y4m")
        _driver_run(rec if mode == "host" else plugin, monkeypatch, src, out, resident=resident, context=N, lanes=lanes)
        outs[mode] = _records(out)
    mask = rec.masks[0]
    expected = frames.copy()
    for lo, hi, ctx_lo, _ in jobs:
        expected[lo:hi] = np.stack(plugin(list(frames[ctx_lo:hi]), mask)[lo - ctx_lo:])
    want = str(tmp_path / "want.y4m")
    monkeypatch.setenv("VSR_IO_COLOR", "host")
    w = video_io.open_writer(want, 25.0, (W, H), frames=N_FR)
    for f in expected:
        w.write(f)
    w.release()
    assert outs["resident"] == _records(want)
    assert outs["lanes2"] == outs["resident"] and outs["lanes2 again"] == outs["resident"]
    assert outs["host"] == outs["resident"]


@pytest.fixture(scope="module")
def two_scenes():
    """scene A (17 frames) then scene B (16): two seeded textures, each translating slowly"""
    return synth.make_clip(17, H, W, BOX, seed=1), synth.make_clip(16, H, W, BOX, seed=2)


@pytest.mark.parametrize("N", [0, 5], ids=["split", "split+context5"])
def test_driver_scene_split(built_lib, gpu_device, plugin, two_scenes, tmp_path, monkeypatch, N):
    """With scene_split the clip A ++ B is written as run(A) followed by run(B), byte for byte (with a context too: it stops at the
    cut); without it the batch (12, 24) straddles the cut at frame 17 and the output differs."""
    from vsr_amd.backend.tools.subtitle_detect import SubtitleDetect

    A, B = two_scenes
    paths = {k: str(tmp_path / f"{k}.y4m") for k in ("a", "b", "ab")}
    monkeypatch.setenv("VSR_IO_COLOR", "host")
    _write_y4m(paths["a"], A)
    _write_y4m(paths["b"], B)
    _write_y4m(paths["ab"], np.concatenate([A, B]))
    assert SubtitleDetect.get_scene_div_frame_no(paths["ab"], 0) == [18]
    rec = {}
    for k in ("a", "b"):
        out = str(tmp_path / f"out_{k}.y4m")
        _driver_run(plugin, monkeypatch, paths[k], out, context=N)
        rec[k] = _records(out)
    out = str(tmp_path / "out_split.y4m")
    sr = _driver_run(plugin, monkeypatch, paths["ab"], out, context=N, scene_split=True)
    assert sr.scene_cuts == [17]
    assert sr.phase_seconds.get("scene cuts", 0.0) > 0.0
    assert _records(out) == rec["a"] + rec["b"]
    out2 = str(tmp_path / "out_grid.y4m")
    _driver_run(plugin, monkeypatch, paths["ab"], out2, context=N, scene_split=False)
    assert _records(out2) != rec["a"] + rec["b"], "a batch across the cut feeds frames of the other scene to the attention"


def test_ranks_and_windows_are_refused_before_a_frame_is_read(built_lib, gpu_device, plugin, tmp_path, monkeypatch):
    from vsr_amd.backend import main as m
    from vsr_amd.backend.tools.resident import ResidentClip
    from vsr_amd.backend.tools.subtitle_detect import SubtitleDetect

    class FakeDist:
        @staticmethod
        def get_world_size():
            return 2

        @staticmethod
        def get_rank():
            return 0

    src = str(tmp_path / "in.y4m")
    monkeypatch.setenv("VSR_IO_COLOR", "host")
    _write_y4m(src, synth.make_clip(6, H, W, BOX, seed=3))
    monkeypatch.setenv("VSR_IO_COLOR", "device")
    reads = []

    def no_read(*a, **kw):
        reads.append(1)
        raise AssertionError("a frame was read")

    with config_values():
        sr = m.SubtitleRemover(src, device="cuda:0")
        sr.sub_areas = [(0, sr.frame_height, 0, sr.frame_width)]
        sr.video_out_path = str(tmp_path / "out.y4m")
        monkeypatch.setattr(ResidentClip, "load", no_read)
        monkeypatch.setattr(SubtitleDetect, "find_subtitle_frame_no", no_read)
        for env in ({"VSR_STTN_CONTEXT": "5", "VSR_SCENE_SPLIT": "0"}, {"VSR_STTN_CONTEXT": "0", "VSR_SCENE_SPLIT": "1"}):
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            # several ranks: the source is not even opened
            with monkeypatch.context() as mp:
                mp.setattr(sr, "_distributed", lambda: FakeDist)
                mp.setattr(m, "open_video", no_read)
                with pytest.raises(RuntimeError, match="one process"):
                    sr.video_inpaint(object(), plugin, text_detector=Det())
            # a windowed run: the header says the clip is over the budget (3 of its 6 frames fit), no frame is read
            with monkeypatch.context() as mp:
                mp.setenv("VSR_IO_RESIDENT", "windows")
                mp.setenv("VSR_RESIDENT_GB", repr(3 * H * W * 3 / 2 ** 30))
                with pytest.raises(RuntimeError, match="resident windows"):
                    sr.video_inpaint(object(), plugin, text_detector=Det())
        monkeypatch.setenv("VSR_STTN_CONTEXT", "13")           # more than getSttnMaxLoadNum() = 12
        monkeypatch.setenv("VSR_SCENE_SPLIT", "0")
        monkeypatch.setattr(m, "open_video", no_read)
        with pytest.raises(ValueError, match="context"):
            sr.video_inpaint(object(), plugin, text_detector=Det())
    assert not reads
