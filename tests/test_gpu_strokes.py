"""--text-detect strokes on the MI355X: the two kernels of csrc/stroke_kernels.hip against tests/_strokes_statement.py bit
for bit, StrokeTextDetection against the statement's boxes and scores, and whole runs of opencv mode that need no weights at all."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _strokes_statement as st

pytestmark = pytest.mark.gpu

SHAPES = [(37, 61), (64, 64), (70, 130), (33, 257)]       # no multiple of the 32 x 64 tile or of F CELL; tile seams; all four borders
SCALES = (1, 2, 3)
COUNTS = (1, 3)
SLACK = 5                                                  # bytes between two frames: every frame at another alignment


def p(t):
    return C.c_void_p(t.data_ptr())


def bar_frames(H, W, F, k, seed):
    """grey noise of 24 levels around 110 with bright (230) and dark (8) bars pasted over it, 1..8 analysis pixels wide, along both
    directions: a bar of width S is a ridge throughout, one of S + 1 loses its rim"""
    rng = np.random.default_rng(seed)
    out = np.empty((k, H, W, 3), np.uint8)
    for f in range(k):
        grey = rng.integers(98, 123, size=(H, W)).astype(np.uint8)
        for width in rng.permutation(np.arange(1, 9)).tolist() * 2:
            level, wide = (230 if rng.integers(2) else 8), width * F
            if rng.integers(2):
                x, y0, y1 = int(rng.integers(0, max(W - wide, 1))), int(rng.integers(0, H // 2)), int(rng.integers(H // 2, H + 1))
                grey[y0:y1, x:x + wide] = level
            else:
                y, x0, x1 = int(rng.integers(0, max(H - wide, 1))), int(rng.integers(0, W // 2)), int(rng.integers(W // 2, W + 1))
                grey[y:y + wide, x0:x1] = level
        out[f] = grey[..., None] + rng.integers(0, 3, size=(H, W, 3)).astype(np.uint8)       # (the three weights of the luma matter)
    return out


class Case:
    """one shape at one scale: 3 frames on the device `SLACK` bytes apart and the statement's count planes"""

    def __init__(self, H, W, F, device):
        self.H, self.W, self.F, self.K = H, W, F, max(COUNTS)
        self.host = bar_frames(H, W, F, self.K, seed=(H * 1000 + W) * 10 + F)
        self.stride = H * W * 3 + SLACK
        flat = np.full(self.K * self.stride, 255, np.uint8)
        for f in range(self.K):
            flat[f * self.stride:f * self.stride + H * W * 3] = self.host[f].ravel()
        self.dev = torch.from_numpy(flat).to(device)
        want = [st.cells(fr, F) for fr in self.host]
        self.cv, self.ch = np.stack([w[0] for w in want]), np.stack([w[1] for w in want])
        self.hc, self.wc = self.cv.shape[1:]


@pytest.fixture(scope="module")
def cases(built_lib, gpu_device):
    return {(shape, F): Case(*shape, F, gpu_device) for shape in SHAPES for F in SCALES}


def cells_call(lib_mod, case, frames_n, cv_t, ch_t, **over):
    a = dict(frames=p(case.dev), stride=case.stride, n=frames_n, H=case.H, W=case.W, F=case.F, S=st.S, C=st.C, cv=p(cv_t), ch=p(ch_t))
    a.update(over)
    return lib_mod.lazy("vsr_strokes_cells")(a["frames"], a["stride"], a["n"], a["H"], a["W"], a["F"], a["S"], a["C"], a["cv"], a["ch"], None)


def test_the_bars_sit_on_the_boundary():
    y = np.full((40, 90), 110, np.int64)
    y[:, 10:10 + st.S] = 230
    y[:, 30:30 + st.S + 1] = 230
    y[:, 50:50 + 2 * st.S] = 230
    y[8:8 + st.S] = np.where(y[8:8 + st.S] == 110, 8, y[8:8 + st.S])
    v, h = st.ridges(y)
    assert v[20, 10:10 + st.S].all(), "a bar of width S is a ridge throughout"
    assert v[20, 31:30 + st.S].all() and not v[20, 30] and not v[20, 30 + st.S], "one of S + 1 loses its two rim pixels"
    assert not v[20, 50:50 + 2 * st.S].any() and not v[20, :10].any(), "one of 2 S is none, nor is a step edge"
    assert h[8:8 + st.S, 0].all() and not v[9, 0:8].any(), "a dark bar along the row is an H-stroke"


@pytest.mark.parametrize("F", SCALES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_cells_equal_the_statement(built_lib, gpu_device, cases, shape, F):
    from vsr_amd._lib import check

    case = cases[(shape, F)]
    for n in COUNTS:
        cv = torch.full((n, case.hc, case.wc), 77, dtype=torch.uint8, device=gpu_device)
        ch = torch.full((n, case.hc, case.wc), 78, dtype=torch.uint8, device=gpu_device)
        check(cells_call(built_lib, case, n, cv, ch))
        torch.cuda.synchronize()
        for name, got, want in (("cv", cv, case.cv[:n]), ("ch", ch, case.ch[:n])):
            got = got.cpu().numpy().astype(np.int64)
            assert np.array_equal(got, want), f"{name} at n = {n}: {np.argwhere(got != want)[:4].tolist()}"
    assert case.cv.max() >= 8 and case.ch.max() >= 8 and (case.cv == 0).any() and (case.ch == 0).any(), "the frames exercise both planes"


def text_call(lib_mod, cv_t, ch_t, frames_n, rows, cols, text_t, **over):
    a = dict(cv=p(cv_t), ch=p(ch_t), n=frames_n, hc=rows, wc=cols, WX=st.WX, WY=st.WY, NV=st.NV, NH=st.NH, text=p(text_t))
    a.update(over)
    return lib_mod.lazy("vsr_strokes_text")(a["cv"], a["ch"], a["n"], a["hc"], a["wc"], a["WX"], a["WY"], a["NV"], a["NH"], a["text"], None)


def check_text(built_lib, device, cv, ch, wx, wy, nv, nh):
    from vsr_amd._lib import check

    n, hc, wc = cv.shape
    text = torch.full((n, hc, wc), 0.5, dtype=torch.float32, device=device)
    check(text_call(built_lib, torch.from_numpy(cv.astype(np.uint8)).to(device), torch.from_numpy(ch.astype(np.uint8)).to(device), n, hc, wc, text,
                    WX=wx, WY=wy, NV=nv, NH=nh))
    torch.cuda.synchronize()
    got = text.cpu().numpy()
    want = np.stack([st.text_cells(cv[k], ch[k], wx, wy, nv, nh) for k in range(n)])
    assert set(np.unique(got).tolist()) <= {0.0, 1.0} and np.array_equal(got == 1.0, want), f"text at {(wx, wy, nv, nh)}"
    return want


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_text_equals_the_statement(built_lib, gpu_device, cases, shape):
    seen = []
    for F in SCALES:
        case = cases[(shape, F)]
        # the statement's thresholds, and thresholds at which about half of these small planes are text
        sv, sh = st.box_sum(case.cv[0], st.WX, st.WY), st.box_sum(case.ch[0], st.WX, st.WY)
        for nv, nh in ((st.NV, st.NH), (int(np.median(sv)), int(np.median(sh))), (int(np.median(sv)) + 1, 0)):
            seen.append(check_text(built_lib, gpu_device, case.cv, case.ch, st.WX, st.WY, nv, nh))
    assert any(w.any() and not w.all() for w in seen), "some maps are mixed"


def test_text_window_clips_at_the_borders(built_lib, gpu_device):
    """planes that are all 16: the sums are 16 times the cells of the window inside the plane; (70, 130) cells have a seam each way"""
    for hc, wc in ((9, 15), (70, 130), (33, 65)):
        full = np.full((2, hc, wc), 16, np.int64)
        inside = 16 * (2 * st.WX + 1) * (2 * st.WY + 1)
        want = check_text(built_lib, gpu_device, full, full, st.WX, st.WY, inside, inside)
        assert (not want.any()) if hc < 2 * st.WY + 1 or wc < 2 * st.WX + 1 else (want[:, st.WY:-st.WY, st.WX:-st.WX].all() and want.sum() == 2 * (hc - 2 * st.WY) * (wc - 2 * st.WX))
        check_text(built_lib, gpu_device, full, full, st.WX, st.WY, inside // 2, inside // 2)
        check_text(built_lib, gpu_device, full, full, 8, 8, 16 * 17 * 9, 16 * 9 * 17)          # the widest window
        check_text(built_lib, gpu_device, full, full, 0, 0, 16, 17)                              # none


def test_bad_arguments_launch_nothing(built_lib, gpu_device, cases):
    case = cases[((37, 61), 1)]
    cv = torch.full((1, case.hc, case.wc), 77, dtype=torch.uint8, device=gpu_device)
    ch = torch.full((1, case.hc, case.wc), 78, dtype=torch.uint8, device=gpu_device)
    bad = [dict(frames=None), dict(cv=None), dict(ch=None), dict(n=0), dict(n=-1), dict(n=65536), dict(H=0), dict(W=-3), dict(H=46341, W=46341),
           dict(F=0), dict(F=9), dict(F=8, H=7), dict(S=0), dict(S=9), dict(C=0), dict(C=256), dict(stride=case.H * case.W * 3 - 1)]
    for over in bad:
        assert cells_call(built_lib, case, 1, cv, ch, **over) == built_lib.VSR_ERR_ARG, over
        assert "strokes" in built_lib.last_error()
    text = torch.full((1, case.hc, case.wc), 0.5, dtype=torch.float32, device=gpu_device)
    bad = [dict(cv=None), dict(ch=None), dict(text=None), dict(n=0), dict(n=65536), dict(hc=0), dict(wc=-1), dict(hc=30000, wc=30000), dict(WX=-1),
           dict(WX=9), dict(WY=-1), dict(WY=9), dict(NV=-1), dict(NH=65536), dict(text=C.c_void_p(text.data_ptr() + 2))]
    for over in bad:
        assert text_call(built_lib, cv, ch, 1, case.hc, case.wc, text, **over) == built_lib.VSR_ERR_ARG, over
    torch.cuda.synchronize()
    assert (cv == 77).all() and (ch == 78).all() and (text == 0.5).all(), "the canaries are untouched"


# ---- the detector class -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pictures():
    """the 9 pictures and the 3 clean ones with the statement's answers"""
    frames = [st.picture(name, k)[0] for name in st.BACKGROUNDS for k in (2, 3, 4)] + [st.background(name) for name in st.BACKGROUNDS]
    want = [st.detect(f) for f in frames]
    assert [len(w[0]) for w in want] == [1] * 9 + [0] * 3
    return frames, want


def same(res, want):
    found, scores = want
    exp = st.result(found, scores)[0]
    return (res["dt_polys"].dtype == np.int32 and res["dt_scores"].dtype == np.float32 and res["dt_polys"].shape == exp["dt_polys"].shape
            and np.array_equal(res["dt_polys"], exp["dt_polys"]) and np.array_equal(res["dt_scores"], exp["dt_scores"]))


def test_detector_returns_the_statements_boxes(built_lib, gpu_device, pictures):
    from vsr_amd.backend.tools import stroke_det as sd

    frames, want = pictures
    det = sd.StrokeTextDetection(0)
    assert det.batch_size == 8 and not hasattr(det, "clone")
    before = dict(sd.stats)
    dev = torch.from_numpy(np.stack(frames)).to(gpu_device)
    got = det.predict_batch_device(dev[:8]) + det.predict_batch_device(dev[8:])
    assert len(got) == 12 and all(same(g, w) for g, w in zip(got, want)), "predict_batch_device"
    assert sd.stats["calls"] == before["calls"] + 2 and sd.stats["frames"] == before["frames"] + 12
    assert sd.stats["launches"] == before["launches"] + (2 + 8) + (2 + 4), "2 + n launches per call"
    assert sd.stats["boxes"] == before["boxes"] + 9
    assert det.predict_batch_device(dev[:0]) == [] and det.predict_batch([]) == []
    batch = det.predict_batch(frames[:8])
    batch_rest = det.predict_batch(frames[8:])
    assert len(batch) == 8 and len(batch_rest) == 4 and all(same(g, w) for g, w in zip(batch + batch_rest, want)), "predict_batch"
    singles_rest = [det.predict(f) for f in frames[8:]]
    assert all(isinstance(s, list) and len(s) == 1 for s in singles_rest)
    assert all(same(s[0], w) for s, w in zip(singles_rest, want[8:])), "predict, the desk at k = 4 and the three pictures without text"
    assert [len(s[0]["dt_scores"]) for s in singles_rest] == [1, 0, 0, 0] and all(s[0]["dt_polys"].shape == (0, 4, 2) for s in singles_rest[1:])
    before = dict(sd.stats)
    singles = [det.predict(f) for f in frames[:8]]
    assert all(isinstance(s, list) and len(s) == 1 for s in singles)
    assert all(same(s[0], w) for s, w in zip(singles, want)), "predict"
    assert all(np.array_equal(s[0]["dt_polys"], b["dt_polys"]) and np.array_equal(s[0]["dt_scores"], b["dt_scores"]) for s, b in zip(singles, batch)), \
        "a batch of 8 equals 8 single calls"
    assert sd.stats["launches"] == before["launches"] + 8 * 3
    # a view whose frames are apart (every second frame of a clip) is read where it is
    apart = det.predict_batch_device(dev[0:12:2])
    assert all(same(g, w) for g, w in zip(apart, want[0:12:2]))


def test_more_components_than_rows(built_lib, gpu_device, monkeypatch):
    """two lines of text are two components of the text map; with room for one row per frame the frame is labelled once more with room
    for all: the statement's boxes, one more launch, counted"""
    from vsr_amd.backend.tools import stroke_det as sd

    frame, _ = st.put_text(st.background("wave"), "HELLO NATION", 2, corner=(20, 20))
    frame, _ = st.put_text(frame, "HELLO NATION", 2, corner=(100, 20))
    one, _ = st.picture("wave", 2)
    want = [st.detect(frame), st.detect(one)]
    assert len(st.components(st.text_cells(*st.cells(frame, 1)))) == 2 and [len(w[0]) for w in want] == [2, 1]
    plenty = sd.StrokeTextDetection(0).predict_batch([frame, one])
    monkeypatch.setattr(sd, "COMPONENT_CAP", 1)
    det = sd.StrokeTextDetection(0)
    before = dict(sd.stats)
    got = det.predict_batch([frame, one])
    assert det._buffers[(2, 144, 256)].cap == 1
    assert all(same(g, w) for g, w in zip(got, want)) and all(same(g, w) for g, w in zip(plenty, want))
    assert sd.stats["relabelled"] == before["relabelled"] + 1 and sd.stats["launches"] == before["launches"] + 2 + 2 + 1
    assert sd.stats["calls"] == before["calls"] + 1 and sd.stats["boxes"] == before["boxes"] + 3


def test_detector_at_F_2(built_lib, gpu_device):
    from vsr_amd.backend.tools import stroke_det as sd

    frames = [np.pad(st.large_picture(k)[0], ((0, 1080 - 288), (0, 1920 - 512), (0, 0)), mode="edge") for k in (6, 5)]
    assert sd.scale(1080, 1920) == 2
    det = sd.StrokeTextDetection(0)
    got = det.predict_batch(frames)
    assert all(same(g, st.detect(f)) for g, f in zip(got, frames))
    assert all(len(g["dt_scores"]) >= 1 for g in got)


# ---- whole runs -------------------------------------------------------------------------------------------------------------------------------
FIRST, LAST = 11, 29                                       # the 1-based frames that carry the text


@pytest.fixture(scope="module")
def text_clip():
    clip, glyphs = st.text_clip(first=FIRST, last=LAST)
    return clip, glyphs


def write_y4m(path, clip):
    from vsr_amd.backend.tools import video_io

    w = video_io.Y4mWriter(str(path), 25.0, (clip.shape[2], clip.shape[1]), chroma="444")
    for f in clip:
        w.write(f)
    w.release()
    return str(path)


def records(path, n):
    """the stored samples of a 4:4:4 8-bit *.y4m: uint8 [n,3,H,W] (Y, U, V)"""
    from vsr_amd.backend.tools import video_io

    r = video_io.Y4mVideo(path)
    rec = np.empty((n, r._fsize), np.uint8)
    assert r.read_planes_into(rec) == n
    r.release()
    return rec.reshape(n, 3, r.h, r.w)


class Run:
    """one file-to-file run of opencv mode with no injected detector and no detector weights configured; the frames the ranges are
    widened by (config.subtitleTimeline*FrameCount, 3 each way by default) are set to 0, so the frames inpainted are the keys of the
    detector pass"""

    SMALL = {"sttnMaxLoadNum": 8, "sttnNeighborStride": 1, "sttnReferenceLength": 6}      # batches of at most 8 frames: windows of ten hold them

    def __init__(self, monkeypatch, src, out, detect, env=(), values=None):
        from vsr_amd.backend.config import config
        from vsr_amd.backend.main import SubtitleRemover
        from vsr_amd.backend.tools.constant import InpaintMode
        from vsr_amd.backend.tools.subtitle_detect import SubtitleDetect

        monkeypatch.setenv("VSR_Y4M_OUT", "source")
        for name in ("VSR_DET_MODEL_DIR", "VSR_DET_WEIGHTS", "VSR_OPENCV_BACKEND", "VSR_OPENCV_FILL", "VSR_LOGO_SCAN", "VSR_LOGO_UNBLEND", "VSR_SEAM_FEATHER",
                     "VSR_REGRAIN", "VSR_DEFLICKER", "VSR_TONE_MATCH", "VSR_GLYPH_KEY", "VSR_GLYPH_HOLD", "VSR_BORROW", "VSR_IO_RESIDENT",
                     "VSR_RESIDENT_GB", "VSR_TEXT_DETECT"):
            monkeypatch.delenv(name, raising=False)
        if detect is not None:
            monkeypatch.setenv("VSR_TEXT_DETECT", detect)
        for name, value in env:
            monkeypatch.setenv(name, value)
        self.keys = []
        found = SubtitleDetect.find_subtitle_frame_no

        def spy(detector, *a, **k):
            sub_list = found(detector, *a, **k)
            self.keys.append(sub_list)
            return sub_list

        monkeypatch.setattr(SubtitleDetect, "find_subtitle_frame_no", spy)
        values = dict(values or {}, inpaintMode=InpaintMode.OPENCV, subtitleTimelineBackwardFrameCount=0, subtitleTimelineForwardFrameCount=0)
        old = {k: getattr(config, k).value for k in values}
        try:
            for k, v in values.items():
                getattr(config, k).value = v
            self.sr = SubtitleRemover(src, device="cuda:0")
            self.sr.append_output = lambda *a: None
            self.sr.video_out_path = str(out)
            self.sr.run()
        finally:
            for k, v in old.items():
                getattr(config, k).value = v
            plugin = getattr(self.sr, "opencv_inpaint", None) if hasattr(self, "sr") else None
            if plugin is not None and hasattr(plugin, "close"):
                plugin.close()
            monkeypatch.setattr(SubtitleDetect, "find_subtitle_frame_no", found)


def check_run(run, src, clip, glyphs):
    from vsr_amd.backend.tools.inpaint_tools import create_mask

    n, H, W = clip.shape[:3]
    assert run.sr.isFinished and len(run.keys) == 1
    sub_list = run.keys[0]
    assert sorted(sub_list) == list(range(FIRST, LAST + 1)), "every sampled frame in 11..29 is a key (the gaps of one frame are filled), none outside"
    before, after = records(src, n), records(run.sr.video_out_path, n)
    text = np.zeros(n, bool)
    text[FIRST - 1:LAST] = True
    assert np.array_equal(after[~text], before[~text]), "frames without text come back as the source's samples, byte for byte"
    assert (before[text][:, 0][:, glyphs] >= 200).all(), "the source's glyphs"
    assert (after[text][:, 0][:, glyphs] < 200).all(), "no luma sample at a glyph pixel stays >= 200"
    masked = np.zeros((H, W), bool)
    for boxes in sub_list.values():
        masked |= create_mask((H, W), boxes) != 0
    assert masked[glyphs].all() and not masked.all()
    assert np.array_equal(after[:, :, ~masked], before[:, :, ~masked]), "every sample outside the masked pixels is the source's"
    return after


def test_a_run_without_any_weights(built_lib, gpu_device, text_clip, tmp_path, monkeypatch):
    from vsr_amd.backend.tools import stroke_det as sd

    clip, glyphs = text_clip
    src = write_y4m(tmp_path / "in.y4m", clip)
    before = dict(sd.stats)
    run = Run(monkeypatch, src, tmp_path / "out.y4m", "strokes")
    check_run(run, src, clip, glyphs)
    assert isinstance(run.sr._stroke_detector, sd.StrokeTextDetection)
    sampled = len(range(0, len(clip), 2))                               # 25 fps: every second frame
    assert sd.stats["frames"] == before["frames"] + sampled and sd.stats["calls"] == before["calls"] + -(-sampled // 8)
    assert sd.stats["launches"] - before["launches"] == 2 * -(-sampled // 8) + sampled


@pytest.mark.parametrize("detect", (None, "model"), ids=("unset", "model"))
def test_without_the_option_no_detector_is_configured(built_lib, gpu_device, text_clip, tmp_path, monkeypatch, detect):
    from vsr_amd.backend.tools import stroke_det as sd

    clip, _ = text_clip
    src = write_y4m(tmp_path / "in.y4m", clip)
    bound, before = set(built_lib.lazy_bound), dict(sd.stats)
    with pytest.raises(RuntimeError, match="no text detector configured"):
        Run(monkeypatch, src, tmp_path / "out.y4m", detect)
    assert sd.stats == before and built_lib.lazy_bound == bound, "nothing of the stroke detector ran"


def test_exemplar_fill_and_windows(built_lib, gpu_device, text_clip, tmp_path, monkeypatch):
    """the same clip with the exemplar fill, and as resident windows under a budget of 2 x 10 frames: the same key frames; the windowed
    run writes the resident run's file, byte for byte"""
    clip, glyphs = text_clip
    n, H, W = clip.shape[:3]
    src = write_y4m(tmp_path / "in.y4m", clip)
    ex = Run(monkeypatch, src, tmp_path / "exemplar.y4m", "strokes", env=(("VSR_OPENCV_FILL", "exemplar"),))
    check_run(ex, src, clip, glyphs)
    resident = Run(monkeypatch, src, tmp_path / "resident.y4m", "strokes", env=(("VSR_IO_COLOR", "device"), ("VSR_IO_RESIDENT", "1")),
                   values=Run.SMALL)
    check_run(resident, src, clip, glyphs)
    gb = repr((2 * 10 * (H * W * 3 + 3 * H * W) + 1024) / 2 ** 30)     # half the budget holds 10 frames (BGR + the kept record)
    windows = Run(monkeypatch, src, tmp_path / "windows.y4m", "strokes",
                  env=(("VSR_IO_COLOR", "device"), ("VSR_IO_RESIDENT", "windows"), ("VSR_RESIDENT_GB", gb)), values=Run.SMALL)
    check_run(windows, src, clip, glyphs)
    assert ex.keys == resident.keys == windows.keys, "the same key frames"
    assert getattr(resident.sr, "resident_windows", None) is None and getattr(windows.sr, "resident_windows", None) is not None and len(windows.sr.resident_windows["windows"]) >= 2
    assert open(windows.sr.video_out_path, "rb").read() == open(resident.sr.video_out_path, "rb").read()
