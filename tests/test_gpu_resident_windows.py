"""VSR_IO_RESIDENT=windows (backend/tools/resident_windows.py): a clip over VSR_RESIDENT_GB runs as a sequence of HBM-resident windows
and writes the file the resident path writes, byte for byte -- sttn-det, lama, propainter, opencv; the source-format sink; the
detector's batches and the scene cuts of pass A; A/B sections; a sink that fails.

The clip is the one of tests/test_gpu_io.py::test_resident_detector_modes_write_the_same_file (two subtitle intervals with a gap,
synthetic weights, injected detector) with a hard cut where the second interval begins (ContentDetector accepts no cut within 15
frames of the clip's start or of another cut, and 34 frames leave room for one)."""
import threading

import numpy as np
import pytest

from tests.test_gpu_y4m_formats import _make_source
from tests.test_y4m_formats import records_of
from vsr_amd.backend.tools import video_io

pytestmark = pytest.mark.gpu

N, CUT = 34, 22
ON = [i for i in range(N) if 3 <= i < 15 or i >= 22]              # the frames that carry the subtitle
RESIDENT_KEY = "read + upload + YUV->BGR"
PER_WINDOW = 10                                                   # frames half the budget of the windowed runs holds


def make_clip(H, W, box):
    """the recipe's clip; from frame CUT on the background is inverted (the glyph blocks stay): a hard cut for ContentDetector"""
    from vsr_amd import synth

    clip = synth.make_clip(N, H, W, box, seed=5)
    plain = synth.make_clip(N, H, W, (0, 1, 0, 1), seed=5)
    for i in range(N):
        if i not in ON:
            clip[i] = plain[i]
    for i in range(CUT, N):
        glyph = (clip[i] != plain[i]).any(axis=-1, keepdims=True)
        clip[i] = np.where(glyph, clip[i], 255 - clip[i])
    return clip


def write_source(path, clip, monkeypatch, depth=8):
    """8 bits: the 4:2:0 file of the recipe; 10: the 4:2:0 source of tests/test_gpu_y4m_formats.py -> bytes of one stored record"""
    _, H, W, _ = clip.shape
    if depth != 8:
        return video_io.record_bytes(_make_source(path, clip, depth, f"420p{depth}"))
    monkeypatch.setenv("VSR_IO_COLOR", "host")
    w = video_io.Y4mWriter(path, 25.0, (W, H), chroma="420")
    for f in clip:
        w.write(f)
    w.release()
    monkeypatch.setenv("VSR_IO_COLOR", "device")
    return H * W + 2 * ((H + 1) // 2) * ((W + 1) // 2)


def make_detector(box):
    quad = np.array([[[box[2], box[0]], [box[3], box[0]], [box[3], box[1]], [box[2], box[1]]]])

    class Det:                                             # the reference's host signature
        batch_size = 4

        def predict(self, img):
            white = (img[box[0] + 8:box[1] - 8, box[2] + 8:box[3] - 8] > 200).mean()
            return [{"dt_polys": quad if white > 0.05 else np.zeros((0, 4, 2), np.int32)}]

    return Det


def budget_gb(H, W, keep_bytes=0, per_window=PER_WINDOW):
    """VSR_RESIDENT_GB whose half holds per_window frames (BGR + the kept record) and not one more"""
    return repr((2 * per_window * (H * W * 3 + keep_bytes) + 1024) / 2 ** 30)


def run(sr_cls, src, out, mode, plugin, det, monkeypatch, resident, gb, ab=None, writer=None):
    """one file-to-file run -> (bytes written, the SubtitleRemover)"""
    monkeypatch.setenv("VSR_IO_COLOR", "device")
    monkeypatch.setenv("VSR_IO_RESIDENT", resident)
    if gb is None:
        monkeypatch.delenv("VSR_RESIDENT_GB", raising=False)
    else:
        monkeypatch.setenv("VSR_RESIDENT_GB", gb)
    sr = sr_cls(src, device="cuda:0")
    sr.sub_areas = [(0, sr.frame_height, 0, sr.frame_width)]
    sr.ab_sections = ab
    sr.video_out_path = out
    if writer is not None:
        sr.video_writer = writer(sr)
    sr.ticks = []
    sr.update_progress = lambda tbar, increment: sr.ticks.append(increment)
    if mode == "propainter":
        sr.propainter_mode(object(), propainter_inpaint=plugin, text_detector=det, single_frame_inpaint=None)
    else:
        sr.video_inpaint(object(), plugin, text_detector=det)
    sr.video_writer.release()
    return open(out, "rb").read(), sr


def check_windowed(sr, budget, boundaries=True):
    rep = getattr(sr, "resident_windows", None)
    assert rep is not None, "the run did not take the windowed path"
    windows = rep["windows"]
    assert len(windows) >= 3, windows
    assert windows[0][0] == 0 and windows[-1][1] == N and all(a[1] == b[0] for a, b in zip(windows, windows[1:]))
    cuts = [hi for _, hi in windows[:-1]]
    if boundaries:
        assert any(c - 1 in ON and c in ON for c in cuts), f"no boundary inside a subtitle interval: {windows}"
        assert any(15 <= c - 1 and c < 22 for c in cuts), f"no boundary inside the gap: {windows}"
    assert 0 < rep["bytes_max"] <= budget
    assert sum(sr.ticks) == N
    assert RESIDENT_KEY not in sr.phase_seconds and any(k.startswith("windows, pass B") for k in sr.phase_seconds)


class config_values:
    """batches of at most 8 frames (so that windows of ten can hold them) and the mode, put back afterwards"""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        from vsr_amd.backend.config import config
        from vsr_amd.backend.tools.constant import InpaintMode

        # (getSttnMaxLoadNum() = max(sttnMaxLoadNum, sttnNeighborStride * sttnReferenceLength): batches of 8 need the product below 8 too)
        self.keys = {"sttnMaxLoadNum": 8, "propainterMaxLoadNum": 8, "sttnNeighborStride": 1, "sttnReferenceLength": 6}
        self.old = {k: getattr(config, k).value for k in self.keys}
        self.old_mode = config.inpaintMode.value
        for k, v in self.keys.items():
            getattr(config, k).value = v
        config.inpaintMode.value = {"sttn-det": InpaintMode.STTN_DET, "lama": InpaintMode.LAMA, "propainter": InpaintMode.PROPAINTER,
                                    "opencv": InpaintMode.OPENCV}[self.mode]

    def __exit__(self, *exc):
        from vsr_amd.backend.config import config

        for k, v in self.old.items():
            getattr(config, k).value = v
        config.inpaintMode.value = self.old_mode


def make_plugin(mode):
    from vsr_amd import synth

    if mode == "sttn-det":
        from vsr_amd.backend.inpaint.sttn_det_inpaint import STTNDetInpaint
        return STTNDetInpaint("cuda:0", {"netG": synth.make_state_dict(0, "det")})
    if mode == "lama":
        from vsr_amd.backend.inpaint.lama_inpaint import LamaInpaint
        return LamaInpaint("cuda:0", synth.make_lama_state_dict(3, 2))
    if mode == "opencv":
        from vsr_amd.backend.inpaint.opencv_inpaint import OpenCVInpaint
        return OpenCVInpaint("cuda:0")
    from vsr_amd.backend.inpaint.propainter_inpaint import PropainterInpaint
    plugin = PropainterInpaint("cuda:0", {"raft": synth.make_raft_state_dict(0), "rfc": synth.make_rfc_state_dict(0),
                                          "propainter": synth.make_propainter_state_dict(0)})
    plugin.raft_iter = 4
    return plugin


@pytest.mark.parametrize("mode", ["sttn-det", "lama", "propainter", "opencv"])
def test_windowed_run_writes_the_resident_file(built_lib, gpu_device, tmp_path, monkeypatch, mode):
    """VSR_IO_RESIDENT=1 under the default budget against VSR_IO_RESIDENT=windows under a budget of 2 x 10 frames: the same bytes, at
    least three windows with a boundary inside a subtitle interval and one inside the gap, bytes_max within the budget, one tick per
    frame, the resident phase key absent; propainter: the cuts of pass A are those of the scene kernels on the resident clip."""
    from vsr_amd.backend.main import SubtitleRemover

    # (RAFT wants strips of at least 128 rows: the propainter case runs on a larger frame)
    H, W = (480, 852) if mode == "propainter" else (240, 432)
    box = (400, 450, 100, 760) if mode == "propainter" else (180, 214, 60, 380)        # ymin, ymax, xmin, xmax
    src = str(tmp_path / "in.y4m")
    write_source(src, make_clip(H, W, box), monkeypatch)
    Det = make_detector(box)
    plugin = make_plugin(mode)
    gb = budget_gb(H, W)
    try:
        with config_values(mode):
            want, sr_res = run(SubtitleRemover, src, str(tmp_path / "resident.y4m"), mode, plugin, Det(), monkeypatch, "1", None)
            got, sr_win = run(SubtitleRemover, src, str(tmp_path / "windows.y4m"), mode, plugin, Det(), monkeypatch, "windows", gb)
            fits, sr_fit = run(SubtitleRemover, src, str(tmp_path / "fits.y4m"), mode, plugin, Det(), monkeypatch, "windows", None)
    finally:
        if hasattr(plugin, "close"):
            plugin.close()
    assert RESIDENT_KEY in sr_res.phase_seconds and sum(sr_res.ticks) == N
    check_windowed(sr_win, float(gb) * 2 ** 30)
    assert got == want, "the windowed run must write the resident run's file"
    # with `windows`, a clip that fits runs the resident code unchanged
    assert RESIDENT_KEY in sr_fit.phase_seconds and getattr(sr_fit, "resident_windows", None) is None and fits == want
    monkeypatch.setenv("VSR_IO_COLOR", "host")
    r, frames = video_io.open_video(str(tmp_path / "windows.y4m")), []
    while True:
        ok, f = r.read()
        if not ok:
            break
        frames.append(f)
    r.release()
    r, changed = video_io.open_video(src), []
    for f in frames:
        changed.append(bool((r.read()[1] != f).any()))
    r.release()
    assert len(frames) == N and np.array(changed)[ON].mean() > 0.7, "something was inpainted"
    if mode == "propainter":
        from vsr_amd.backend.tools.resident import ResidentClip
        from vsr_amd.backend.tools.scene_detect import get_scene_div_frame_no

        monkeypatch.setenv("VSR_IO_COLOR", "device")
        reader = video_io.open_video(src)
        clip = ResidentClip.load(reader, reader.planes_format(), N, H, W, "cuda:0")
        reader.release()
        cuts = get_scene_div_frame_no(src, clip=clip)
        assert cuts == [CUT + 1], "the clip's hard cut"
        assert sr_win.resident_windows["scene_cuts"] == cuts
        assert sr_win.resident_windows["records_read_pass_a"] == N      # the scene kernels see every frame
    else:
        assert sr_win.resident_windows["records_read_pass_a"] == len(range(0, N, 2))      # 25 fps: every second frame is sampled


def test_windowed_source_format_output(built_lib, gpu_device, tmp_path, monkeypatch):
    """VSR_Y4M_OUT=source on a 10-bit 4:2:0 source, sttn-det: the budget counts BGR + the kept records; the resident run's file; frames
    without a subtitle come back as stored"""
    from vsr_amd.backend.main import SubtitleRemover

    H, W, box = 240, 432, (180, 214, 60, 380)
    src = str(tmp_path / "in.y4m")
    rec = write_source(src, make_clip(H, W, box), monkeypatch, depth=10)
    monkeypatch.setenv("VSR_Y4M_OUT", "source")
    Det = make_detector(box)
    plugin = make_plugin("sttn-det")
    gb = budget_gb(H, W, rec)
    try:
        with config_values("sttn-det"):
            want, sr_res = run(SubtitleRemover, src, str(tmp_path / "resident.y4m"), "sttn-det", plugin, Det(), monkeypatch, "1", None)
            got, sr_win = run(SubtitleRemover, src, str(tmp_path / "windows.y4m"), "sttn-det", plugin, Det(), monkeypatch, "windows", gb)
    finally:
        if hasattr(plugin, "close"):
            plugin.close()
    assert RESIDENT_KEY in sr_res.phase_seconds
    check_windowed(sr_win, float(gb) * 2 ** 30, boundaries=False)
    longest = max(hi - lo for lo, hi in sr_win.resident_windows["windows"])
    assert sr_win.resident_windows["bytes_max"] == 2 * longest * (H * W * 3 + rec), "the kept records are part of the live bytes"
    assert got == want
    assert got.split(b"\n", 1)[0] == open(src, "rb").readline().rstrip(b"\n")
    from tests.test_y4m_formats import fmt_of

    fmt = fmt_of("420", 10, False, H, W)
    srcs, outs = records_of(src, fmt), records_of(str(tmp_path / "windows.y4m"), fmt)
    differ = np.array([not np.array_equal(a, b) for a, b in zip(srcs, outs)])
    assert len(outs) == N and differ[ON].mean() > 0.7
    untouched = [k for k in range(N) if not differ[k]]
    assert any(15 <= k < 22 for k in untouched), "a frame of the gap comes back as stored"
    assert not differ[0], "frame 0 lies in front of every interval"


class RecordingDetector:
    """keeps the frames of every call; the device signature (batches of batch_size frames) and no clone(): one lane"""
    batch_size = 4

    def __init__(self, box):
        self.box, self.calls = box, []
        self.quad = np.array([[[box[2], box[0]], [box[3], box[0]], [box[3], box[1]], [box[2], box[1]]]])

    def predict_batch_device(self, frames_dev):
        imgs = frames_dev.cpu().numpy()
        self.calls.append(imgs.copy())
        b = self.box
        return [{"dt_polys": self.quad if (img[b[0] + 8:b[1] - 8, b[2] + 8:b[3] - 8] > 200).mean() > 0.05 else np.zeros((0, 4, 2), np.int32)}
                for img in imgs]

    def predict(self, img):
        raise AssertionError("a detector with predict_batch_device must not get host frames")


@pytest.mark.parametrize("ab", [None, [range(2, 13), range(20, 31)]])
@pytest.mark.parametrize("everything", [False, True])
def test_pass_a_feeds_the_detector_the_resident_batches(built_lib, gpu_device, tmp_path, monkeypatch, ab, everything):
    """the batches an injected detector sees in pass A are those of SubtitleDetect._find_resident in composition and order
    (VSR_DET_LANES=1), the sub_list is equal, with A/B sections too; `everything`: every record is read and the scene kernels ride
    along -- the cuts of get_scene_div_frame_no(clip=...) on the resident clip"""
    from vsr_amd.backend.main import SubtitleRemover
    from vsr_amd.backend.tools.scene_detect import get_scene_div_frame_no
    from vsr_amd.backend.tools.subtitle_detect import SubtitleDetect

    H, W, box = 240, 432, (180, 214, 60, 380)
    src = str(tmp_path / "in.y4m")
    write_source(src, make_clip(H, W, box), monkeypatch)
    monkeypatch.setenv("VSR_DET_LANES", "1")
    seen = {}
    # sampled records only: 17 (12 with the sections) frames, 5 to a window, so that they too need several.  Every record: the
    # budget of ten frames less the side buffer of one batch leaves windows of three -- a batch of four sampled frames spans 7
    # frames of the file and 13 across the hole between the sections (7 frames, longer than two windows): gathered across windows
    tight = budget_gb(H, W, per_window=5)
    for how, resident, gb in (("resident", "1", None), ("windows", "windows", tight)):
        monkeypatch.setenv("VSR_IO_RESIDENT", resident)
        if gb is None:
            monkeypatch.delenv("VSR_RESIDENT_GB", raising=False)
        else:
            monkeypatch.setenv("VSR_RESIDENT_GB", gb)
        sr = SubtitleRemover(src, device="cuda:0")
        sr.sub_areas = [(0, H, 0, W)]
        sr.ab_sections = ab
        sr.video_out_path = str(tmp_path / f"{how}.y4m")
        det = RecordingDetector(box)
        finder = SubtitleDetect(src, sr.sub_areas, text_detector=det)
        if how == "resident":
            assert sr._open_windowed() is None
            clip = sr._open_resident()[0]
            cuts = get_scene_div_frame_no(src, clip=clip)
        else:
            assert sr._open_resident() is None
            clip = sr._open_windowed()
            clip.want_scene_cuts = everything
        seen[how] = (finder.find_subtitle_frame_no(sub_remover=sr, clip=clip), det.calls, clip)
        sr.video_writer.release()
    (sub_res, calls_res, _), (sub_win, calls_win, wclip) = seen["resident"], seen["windows"]
    assert len(calls_res) >= 3 and len(sub_res) > 8
    assert [c.shape for c in calls_win] == [c.shape for c in calls_res]
    assert all(np.array_equal(a, b) for a, b in zip(calls_win, calls_res)), "a batch of pass A differs from the resident pass's"
    assert sub_win == sub_res
    sampled = sum(c.shape[0] for c in calls_res)
    assert wclip.report["pass_a_windows"] >= (10 if everything else 2) and 0 < wclip.report["bytes_max"] <= float(tight) * 2 ** 30
    if everything:
        assert wclip.report["records_read_pass_a"] == N and wclip.scene_cuts == cuts == [CUT + 1]
    else:
        assert wclip.report["records_read_pass_a"] == sampled and wclip.scene_cuts is None


@pytest.mark.parametrize("mode,pass_a", [("opencv", "sampled"), ("opencv", "all"), ("propainter", "sampled")])
def test_windowed_ab_sections(built_lib, gpu_device, tmp_path, monkeypatch, mode, pass_a):
    """sr.ab_sections set, the hole between the sections (11 frames) longer than a window: the detector samples inside the sections
    only, on both paths; the same file -- also when pass A reads every record (VSR_WINDOWS_PASS_A=all; propainter always does)"""
    from vsr_amd.backend.main import SubtitleRemover

    H, W = (480, 852) if mode == "propainter" else (240, 432)
    box = (400, 450, 100, 760) if mode == "propainter" else (180, 214, 60, 380)
    src = str(tmp_path / "in.y4m")
    write_source(src, make_clip(H, W, box), monkeypatch)
    Det = make_detector(box)
    plugin = make_plugin(mode)
    gb = budget_gb(H, W)
    ab = [range(2, 13), range(24, 31)]
    monkeypatch.setenv("VSR_WINDOWS_PASS_A", pass_a)
    try:
        with config_values(mode):
            want, _ = run(SubtitleRemover, src, str(tmp_path / "resident.y4m"), mode, plugin, Det(), monkeypatch, "1", None, ab=ab)
            got, sr_win = run(SubtitleRemover, src, str(tmp_path / "windows.y4m"), mode, plugin, Det(), monkeypatch, "windows", gb, ab=ab)
            whole, _ = run(SubtitleRemover, src, str(tmp_path / "whole.y4m"), mode, plugin, Det(), monkeypatch, "windows", gb)
    finally:
        if hasattr(plugin, "close"):
            plugin.close()
    check_windowed(sr_win, float(gb) * 2 ** 30, boundaries=False)
    assert sr_win.resident_windows["records_read_pass_a"] == (10 if (mode, pass_a) == ("opencv", "sampled") else N)
    assert got == want and got != whole, "the sections change what is inpainted, the windows do not"


def test_sttn_auto_takes_windows_as_one(built_lib, gpu_device, tmp_path, monkeypatch):
    """in sttn-auto, whose chunk loop handles any length, VSR_IO_RESIDENT=windows behaves like 1: the same file, no windowed run"""
    from vsr_amd import synth
    from vsr_amd.backend.config import config
    from vsr_amd.backend.main import SubtitleRemover
    from vsr_amd.backend.tools.constant import InpaintMode

    H, W, n, box = 480, 852, 14, (400, 450, 100, 760)
    src = str(tmp_path / "in.y4m")
    monkeypatch.setenv("VSR_IO_COLOR", "host")
    w = video_io.Y4mWriter(src, 25.0, (W, H), chroma="420")
    for f in synth.make_clip(n, H, W, box, seed=11):
        w.write(f)
    w.release()
    monkeypatch.setenv("VSR_IO_COLOR", "device")
    monkeypatch.setenv("VSR_RESIDENT_GB", budget_gb(H, W, per_window=3))
    keys = {"sttnMaxLoadNum": 6, "sttnNeighborStride": 1, "sttnReferenceLength": 6}
    old = {k: getattr(config, k).value for k in keys}
    old_mode = config.inpaintMode.value
    outs = {}
    try:
        for k, v in keys.items():
            getattr(config, k).value = v
        config.inpaintMode.value = InpaintMode.STTN_AUTO
        for resident in ("1", "windows"):
            monkeypatch.setenv("VSR_IO_RESIDENT", resident)
            sr = SubtitleRemover(src, model_path={"netG": synth.make_state_dict(0, "auto")})
            sr.sub_areas = [box]
            sr.video_out_path = str(tmp_path / f"out_{resident}.y4m")
            ticks = []
            sr.update_progress = lambda tbar, increment: ticks.append(increment)
            sr.sttn_auto_mode(tbar=object())
            sr.video_writer.release()
            assert sum(ticks) == n and sr.resident_windows is None
            outs[resident] = open(sr.video_out_path, "rb").read()
    finally:
        for k, v in old.items():
            getattr(config, k).value = v
        config.inpaintMode.value = old_mode
    assert outs["windows"] == outs["1"] and len(outs["1"]) > n * H * W


@pytest.mark.parametrize("per_window,what", [(1, "a detector batch"), (5, "an inpainting batch")])
def test_a_batch_over_half_the_budget_takes_the_host_frame_loop(built_lib, gpu_device, tmp_path, monkeypatch, per_window, what):
    """half the budget holds one frame: a detector batch of four does not fit pass A; five frames: pass A runs in windows, a batch of
    eight does not fit pass B.  Either way one line is logged, the host-frame loop writes the resident run's file, and the run does
    not report windows."""
    from vsr_amd.backend.main import SubtitleRemover

    H, W, box = 240, 432, (180, 214, 60, 380)
    src = str(tmp_path / "in.y4m")
    write_source(src, make_clip(H, W, box), monkeypatch)
    Det = make_detector(box)
    plugin = make_plugin("opencv")
    lines = []
    monkeypatch.setattr(SubtitleRemover, "append_output", lambda self, *a: lines.append(" ".join(str(x) for x in a)))
    with config_values("opencv"):
        want, _ = run(SubtitleRemover, src, str(tmp_path / "resident.y4m"), "opencv", plugin, Det(), monkeypatch, "1", None)
        got, sr = run(SubtitleRemover, src, str(tmp_path / "windows.y4m"), "opencv", plugin, Det(), monkeypatch, "windows",
                      budget_gb(H, W, per_window=per_window))
    said = [ln for ln in lines if "host-frame loop" in ln]
    assert len(said) == 1 and what in said[0], lines
    assert sr.resident_windows is None and "read + inpainting + write (host frames)" in sr.phase_seconds
    assert not any(k.startswith("windows, pass B") for k in sr.phase_seconds) and sum(sr.ticks) == N
    assert got == want


def test_windowed_short_file(built_lib, gpu_device, tmp_path, monkeypatch):
    """the last record cut short: the clip ends with the frames in front of it, as on the resident path -- same file, one tick each"""
    import os

    from vsr_amd.backend.main import SubtitleRemover

    H, W, box = 240, 432, (180, 214, 60, 380)
    src = str(tmp_path / "in.y4m")
    rec = write_source(src, make_clip(H, W, box), monkeypatch)
    os.truncate(src, os.path.getsize(src) - rec // 2)
    Det = make_detector(box)
    plugin = make_plugin("opencv")
    gb = budget_gb(H, W)
    with config_values("opencv"):
        want, sr_res = run(SubtitleRemover, src, str(tmp_path / "resident.y4m"), "opencv", plugin, Det(), monkeypatch, "1", None)
        got, sr_win = run(SubtitleRemover, src, str(tmp_path / "windows.y4m"), "opencv", plugin, Det(), monkeypatch, "windows", gb)
    windows = sr_win.resident_windows["windows"]
    assert len(windows) >= 3 and windows[-1][1] == N - 1
    assert sum(sr_res.ticks) == sum(sr_win.ticks) == N - 1
    assert got == want and got.count(b"FRAME\n") >= N - 1


def test_windowed_batch_lanes(built_lib, gpu_device, tmp_path, monkeypatch):
    """VSR_BATCH_LANES=2 per window: windows of up to 15 frames hold two batches each, two plugin instances share them; the same file"""
    from vsr_amd.backend.main import SubtitleRemover

    H, W, box = 240, 432, (180, 214, 60, 380)
    src = str(tmp_path / "in.y4m")
    write_source(src, make_clip(H, W, box), monkeypatch)
    Det = make_detector(box)
    plugin = make_plugin("opencv")
    gb = budget_gb(H, W, per_window=15)
    with config_values("opencv"):
        want, _ = run(SubtitleRemover, src, str(tmp_path / "resident.y4m"), "opencv", plugin, Det(), monkeypatch, "1", None)
        monkeypatch.setenv("VSR_BATCH_LANES", "2")
        got, sr_win = run(SubtitleRemover, src, str(tmp_path / "windows.y4m"), "opencv", plugin, Det(), monkeypatch, "windows", gb)
    windows = sr_win.resident_windows["windows"]
    assert len(windows) >= 2 and max(hi - lo for lo, hi in windows) > 8, "a window with more than one batch"
    assert sum(sr_win.ticks) == N and sr_win.resident_windows["bytes_max"] <= float(gb) * 2 ** 30
    assert got == want


def test_a_failing_sink_raises_and_leaves_no_thread(built_lib, gpu_device, tmp_path, monkeypatch):
    """a writer whose write_planes raises in the second window: the run raises that error, loader and store threads are gone"""
    from vsr_amd.backend.main import SubtitleRemover

    H, W, box = 240, 432, (180, 214, 60, 380)
    src = str(tmp_path / "in.y4m")
    write_source(src, make_clip(H, W, box), monkeypatch)
    Det = make_detector(box)
    plugin = make_plugin("opencv")
    gb = budget_gb(H, W)
    before = {t.ident for t in threading.enumerate()}

    class SinkFailed(Exception):
        pass

    class FailingWriter:
        def __init__(self, sr):
            self.inner = video_io.Y4mWriter(sr.video_out_path, sr.fps, (sr.frame_width, sr.frame_height))
            self.records, self.fail_from = 0, None

        def planes_format(self):
            return self.inner.planes_format()

        def write_planes(self, recs):
            if self.fail_from is not None and self.records + len(recs) > self.fail_from:
                raise SinkFailed(f"record {self.records}")
            self.records += len(recs)
            self.inner.write_planes(recs)

        def release(self):
            self.inner.release()

    writers = []

    def writer(fail):
        def make(sr):
            writers.append(FailingWriter(sr))
            writers[-1].fail_from = fail
            return writers[-1]
        return make

    with config_values("opencv"):
        _, sr_ok = run(SubtitleRemover, src, str(tmp_path / "ok.y4m"), "opencv", plugin, Det(), monkeypatch, "windows", gb, writer=writer(None))
        windows = sr_ok.resident_windows["windows"]
        assert writers[0].records == N and len(windows) >= 3
        with pytest.raises(SinkFailed):
            run(SubtitleRemover, src, str(tmp_path / "bad.y4m"), "opencv", plugin, Det(), monkeypatch, "windows", gb,
                writer=writer(windows[1][0]))
    assert windows[1][0] <= writers[1].records < windows[1][1], "the first window was written, the second was not finished"
    writers[1].release()
    left = [t.name for t in threading.enumerate() if t.ident not in before and t.name.startswith(("vsr-window", "vsr-batch-lane", "vsr-streaming"))]
    assert left == [], f"threads of the run are still alive: {left}"
