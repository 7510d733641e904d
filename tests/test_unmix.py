"""--logo-unblend without a device: the numpy statement tests/_unmix_statement.py on the clips of the design's table,
backend/tools/unblend.solve held to it, the option, the refusals, the wiring of run() and the order of the chain.  The kernels are held
to the statement in tests/test_gpu_unmix.py, the plugin calls and a whole run in tests/test_gpu_seam_unmix.py."""
import ctypes as C

import numpy as np
import pytest

from tests import _static_statement as st
from tests import _unmix_statement as us

FOUR = ("VSR_SEAM_FEATHER", "VSR_REGRAIN", "VSR_DEFLICKER", "VSR_TONE_MATCH")
PASSES = FOUR + ("VSR_GLYPH_KEY", "VSR_GLYPH_HOLD", "VSR_BORROW", "VSR_BORROW_PAN")


def sampled(clip):
    return [clip[i] for i in st.sample_indices(len(clip))]


def restore(clip, areas, info=None):
    """the whole definition on a clip: every area the statement accepts un-mixed on every frame; a refused area keeps every byte"""
    out = clip.copy()
    verdicts = []
    for box in areas:
        one = {}
        solved = us.plan(sampled(clip), box, one)
        verdicts.append((box, solved if isinstance(solved, str) else "accepted", one))
        if not isinstance(solved, str):
            for f in range(len(clip)):
                us.unmix(out[f], clip[f], solved[0], solved[1], box)
    if info is not None:
        info.extend(verdicts)
    return out


# ---- the statement on the design's clips ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a", [64, 128])
def test_a_translucent_logo_on_the_wave_is_un_mixed(a):
    clean = st.wave()
    clip = us.blend(clean, a)
    areas = st.areas(clip)
    assert areas == [st.LOGO_AREA], "one area"
    info = []
    out = restore(clip, areas, info)
    (box, verdict, one), = info
    assert verdict == "accepted" and one["seeds"] == 0, "the gate leaves no seed"
    assert one["lvl"] == 256 - a - 1 and one["opaque"] == 0
    y0, y1, x0, x1 = box
    inside = np.abs(out[:, y0:y1, x0:x1].astype(np.int64) - clean[:, y0:y1, x0:x1])
    blended = np.abs(clip[:, y0:y1, x0:x1].astype(np.int64) - clean[:, y0:y1, x0:x1])
    print(f"a = {a}: restored max {inside.max()} mean {inside.mean():.3f}; blended max {blended.max()} mean {blended.mean():.2f}")
    assert inside.max() <= 2, "every restored frame lies within 2 levels of the clean wave"
    outside = np.ones(clip.shape[1:3], bool)
    outside[y0:y1, x0:x1] = False
    assert np.array_equal(out[:, outside], clip[:, outside]), "nothing outside the box is written"


def test_a_nearly_opaque_logo_shows_through_the_gate():
    clip = us.blend(st.wave(), 224)
    info = {}
    assert us.plan(sampled(clip), st.LOGO_AREA, info) == "shows"
    assert info["lvl"] == 31 and info["opaque"] == (st.LOGO[1] - st.LOGO[0]) * (st.LOGO[3] - st.LOGO[2]) and info["seeds"] > 0
    print("a = 224: seeds left", info["seeds"])


def test_an_opaque_logo_is_refused_and_nothing_is_written():
    clip = st.clip_logo()
    areas = st.areas(clip)
    assert areas == [st.LOGO_AREA]
    info = []
    out = restore(clip, areas, info)
    assert info[0][1] == "shows" and info[0][2]["lvl"] == 0
    assert np.array_equal(out, clip), "a refused area keeps what the run without the option writes"


@pytest.fixture(scope="module")
def smooth():
    return us.texture()


def test_random_crops_of_a_texture_give_the_level_and_the_offset(smooth):
    """M = 120 frames at random offsets into one smooth texture, a = 96 toward white: g = 160, o = 96 * 255 / 16 = 1530 in Q4"""
    rng = np.random.default_rng(11)
    off = [(int(rng.integers(0, 1024 - st.CLIP_H)), int(rng.integers(0, 1024 - st.CLIP_W))) for _ in range(120)]
    clean = us.crops(smooth, off)
    clip = us.blend(clean, 96)
    box = st.LOGO_AREA
    info = {}
    solved = us.plan(list(clip), box, info)
    assert not isinstance(solved, str), solved
    gt, ot = solved
    level = gt == info["lvl"]
    print("level", info["lvl"], "offset", ot[level][0].tolist(), "classes", info["level"], info["clear"], info["rim"])
    assert abs(info["lvl"] - 160) <= 4
    assert (np.abs(ot[level] - 1530) <= 32).all()
    assert gt.min() >= 0 and gt.max() <= us.GMAX and ot.min() >= -8160 and ot.max() <= 4080
    y0, y1, x0, x1 = box
    out = np.stack([us.unmix(f.copy(), f, gt, ot, box) for f in clip])
    restored = np.abs(out[:, y0:y1, x0:x1].astype(np.int64) - clean[:, y0:y1, x0:x1]).mean()
    blended = np.abs(clip[:, y0:y1, x0:x1].astype(np.int64) - clean[:, y0:y1, x0:x1]).mean()
    print(f"mean error: restored {restored:.2f}, blended {blended:.2f}")
    assert restored < blended


def test_a_pan_of_forty_frames_un_mixes_nothing_when_the_gate_refuses(smooth):
    clean = us.crops(smooth, [(3 * f, 5 * f) for f in range(40)])
    clip = us.blend(clean, 96)
    areas = st.areas(clip)
    info = []
    out = restore(clip, areas, info)
    print("pan:", [(v, one.get("seeds")) for _, v, one in info])
    for box, verdict, one in info:
        if verdict != "accepted":
            y0, y1, x0, x1 = box
            assert np.array_equal(out[:, y0:y1, x0:x1], clip[:, y0:y1, x0:x1]), "a refused area is not un-mixed"
        else:
            assert one["seeds"] == 0


def test_refusals_still_none_and_text():
    from vsr_amd.backend.tools import unblend

    still = us.blend(st.wave(still=True), 128)
    assert us.plan(sampled(still), st.LOGO_AREA) == "still"
    assert us.plan(sampled(st.wave()), st.LOGO_AREA) == "none", "no pixel of the box with a gain below 232"
    faint = us.blend(st.wave(), 24)
    info = {}
    assert us.plan(sampled(faint), st.LOGO_AREA, info) == "faint" and info["lvl"] > us.FAINT

    class Scan:                                         # an area that meets a text box is refused before any work
        H, W = st.CLIP_H, st.CLIP_W

        @property
        def pieces(self):
            raise AssertionError("work was started")

    y0, y1, x0, x1 = st.LOGO_AREA
    crossing = (y1 - 1, y1 + 20, x0 - 30, x0 + 1)
    beside = (y1, y1 + 20, x0, x1)
    assert us.meets(st.LOGO_AREA, crossing) and not us.meets(st.LOGO_AREA, beside)
    assert unblend.meets(st.LOGO_AREA, crossing) and not unblend.meets(st.LOGO_AREA, beside)
    assert unblend.make_plans(Scan(), [st.LOGO_AREA], [beside, crossing]) == ([], [(st.LOGO_AREA, "text")])


# ---- the host part of the package against the statement -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a64", "a128", "a224", "opaque", "plain", "still", "faint", "texture"])
def test_solve_equals_the_statement(name, smooth):
    from vsr_amd.backend.tools import unblend

    assert (unblend.RING, unblend.GMIN, unblend.GMAX, unblend.BAND, unblend.HIST_BELOW, unblend.FAINT, unblend.STILL) == \
           (us.RING, us.GMIN, us.GMAX, us.BAND, us.HIST_BELOW, us.FAINT, us.STILL)
    if name == "texture":
        rng = np.random.default_rng(5)
        clip = us.blend(us.crops(smooth, [(int(rng.integers(0, 800)), int(rng.integers(0, 700))) for _ in range(48)]), 96)
    else:
        clip = {"a64": lambda: us.blend(st.wave(), 64), "a128": lambda: us.blend(st.wave(), 128), "a224": lambda: us.blend(st.wave(), 224),
                "opaque": st.clip_logo, "plain": st.wave, "still": lambda: us.blend(st.wave(still=True), 128),
                "faint": lambda: us.blend(st.wave(), 24)}[name]()
    frames = sampled(clip)
    box = st.LOGO_AREA
    gbox = us.grown_box(box, st.CLIP_H, st.CLIP_W)
    assert unblend.grown_box(box, st.CLIP_H, st.CLIP_W) == gbox == (0, 71, 165, 256), "the ring is clipped at two sides"
    S1, S2 = us.moments(frames, gbox)
    want = us.solve(S1, S2, len(frames), box, gbox)
    got = unblend.solve(S1.astype(np.uint32), S2.astype(np.uint32), len(frames), box, gbox)
    if isinstance(want, str):
        assert got == want
    else:
        assert got[0].dtype == np.uint16 and got[1].dtype == np.int16
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


# ---- options ----------------------------------------------------------------------------------------------------------------------------
def test_option_parsing():
    from vsr_amd.backend import main as m
    from vsr_amd.backend.tools import unblend
    from vsr_amd.backend.tools.args_handler import parse_args

    assert unblend.ENV == "VSR_LOGO_UNBLEND"
    assert unblend.unblend_option(env={}) is False and unblend.unblend_option(env={"VSR_LOGO_UNBLEND": ""}) is False
    assert unblend.unblend_option(env={"VSR_LOGO_UNBLEND": "0"}) is False and unblend.unblend_option(env={"VSR_LOGO_UNBLEND": "1"}) is True
    assert unblend.unblend_option(True, env={}) is True and unblend.unblend_option(0, env={"VSR_LOGO_UNBLEND": "1"}) is False
    for bad in ("2", "x", "-1", "yes"):
        with pytest.raises(ValueError, match="logo unblend"):
            unblend.unblend_option(env={"VSR_LOGO_UNBLEND": bad})
    assert unblend.refuse(0, 0) is False and unblend.refuse(1, 1) is True and unblend.refuse(0, 1) is False
    with pytest.raises(ValueError, match="--logo-unblend .* --logo-scan"):
        unblend.refuse(1, 0)
    assert parse_args(["-i", "x.y4m"]).logo_unblend is False
    assert parse_args(["-i", "x.y4m", "--logo-scan", "--logo-unblend"]).logo_unblend is True
    with pytest.raises(SystemExit):
        parse_args(["-i", "x.y4m", "--logo-unblend"])
    entry = [e for e in m.FLAG_ENV if e[0] == "logo_unblend"]
    assert len(entry) == 1 and entry[0][1] == "VSR_LOGO_UNBLEND" and entry[0][2](True) == "1"


def test_flag_sets_the_environment_variable(monkeypatch):
    import os

    from vsr_amd.backend import main as m

    seen = {}

    class Stop(Exception):
        pass

    def fake_remover(path):
        seen["env"] = os.environ.get("VSR_LOGO_UNBLEND"), os.environ.get("VSR_LOGO_SCAN")
        raise Stop

    monkeypatch.setenv("VSR_LOGO_UNBLEND", "0")
    monkeypatch.setenv("VSR_LOGO_SCAN", "0")
    monkeypatch.setattr(m, "SubtitleRemover", fake_remover)
    with pytest.raises(Stop):
        m.main(["-i", "x.y4m", "--logo-scan", "--logo-unblend"])
    assert seen["env"] == ("1", "1")


def test_run_refuses_before_a_frame_is_read(monkeypatch):
    from vsr_amd.backend import main as m
    from vsr_amd.backend.tools import logo_scan
    from vsr_amd.backend.tools.video_io import ArrayVideo

    class Source(ArrayVideo):
        def read(self):
            raise AssertionError("a frame was read")

    def no_work(*a, **kw):
        raise AssertionError("work was started")

    for name in PASSES:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setattr(logo_scan, "find_areas", no_work)
    monkeypatch.setattr(logo_scan, "run_scan", no_work)
    sr = m.SubtitleRemover(Source(np.zeros((4, 48, 64, 3), np.uint8)))
    monkeypatch.setenv("VSR_LOGO_UNBLEND", "1")
    monkeypatch.delenv("VSR_LOGO_SCAN", raising=False)
    with pytest.raises(ValueError, match="--logo-unblend .* --logo-scan"):
        sr.run()
    monkeypatch.setenv("VSR_LOGO_SCAN", "1")
    monkeypatch.setenv("VSR_LOGO_UNBLEND", "2")
    with pytest.raises(ValueError, match="logo unblend"):
        sr.run()


class FakePlan:
    def __init__(self, box, H, W, gt=None, ot=None):
        self.box, self.H, self.W, self.gt, self.ot, self.level = box, H, W, gt, ot, 127


def test_run_makes_the_plans_behind_the_detector_pass_and_clears_them(monkeypatch):
    """run() keeps the scan, _with_static_areas makes the plans from the detector's boxes of all frames, registers them, and every
    area stays in every frame's list; when run() ends the registry is empty.  With the option off nothing of this is called."""
    from vsr_amd.backend import main as m
    from vsr_amd.backend.config import config
    from vsr_amd.backend.tools import logo_scan, unblend
    from vsr_amd.backend.tools.constant import InpaintMode
    from vsr_amd.backend.tools.video_io import ArrayVideo

    for name in PASSES:
        monkeypatch.delenv(name, raising=False)
    areas = [(1, 47, 189, 251), (100, 130, 10, 60)]
    calls = []

    class FakeScan:
        found = areas

    def run_scan(video, device=0, clip=None, report=None, keep=False):
        calls.append(("run_scan", keep))
        return FakeScan()

    def find_areas(video, device=0, clip=None, report=None):
        calls.append(("find_areas",))
        return list(areas)

    def make_plans(scan, given, text_boxes=()):
        calls.append(("make_plans", type(scan).__name__, list(given), list(text_boxes)))
        return [FakePlan(areas[0], 144, 256)], [(areas[1], "text")]

    monkeypatch.setattr(logo_scan, "run_scan", run_scan)
    monkeypatch.setattr(logo_scan, "find_areas", find_areas)
    monkeypatch.setattr(unblend, "make_plans", make_plans)
    seen = {}

    def video_inpaint(self, tbar, model, text_detector=None):
        # the detector pass found one box (xmin, xmax, ymin, ymax) on frame 3 that crosses the second area
        sub_list = self._with_static_areas({3: [(20, 80, 110, 125)]})
        seen.update(sub_list=sub_list, active=unblend.active(), scan=self._logo_scan)

    monkeypatch.setattr(m.SubtitleRemover, "video_inpaint", video_inpaint)
    monkeypatch.setattr(m.SubtitleRemover, "_default_detector", lambda self: None)
    old = config.inpaintMode.value
    try:
        config.inpaintMode.value = InpaintMode.OPENCV
        monkeypatch.setenv("VSR_LOGO_SCAN", "1")
        monkeypatch.setenv("VSR_LOGO_UNBLEND", "1")
        said = []
        sr = m.SubtitleRemover(ArrayVideo(np.zeros((16, 144, 256, 3), np.uint8), fps=25.0))
        sr.opencv_inpaint = object()
        sr.append_output = lambda *a: said.append(" ".join(str(x) for x in a))
        sr.run()
        assert calls == [("run_scan", True), ("make_plans", "FakeScan", areas, [(110, 125, 20, 80)])]
        assert [p.box for p in seen["active"]] == [areas[0]] and seen["scan"] is None
        static = [(189, 251, 1, 47), (10, 60, 100, 130)]
        assert all(seen["sub_list"][no][-2:] == static for no in range(1, 17)), "every area stays in every frame's list"
        assert unblend.active() == [] and sr.unblend_refusals == [(areas[1], "text")]
        assert any("is un-mixed" in s and str(areas[0]) in s for s in said)
        assert any("stays inpainted (text)" in s and str(areas[1]) in s for s in said)
        # off: the calls of before
        del calls[:]
        monkeypatch.delenv("VSR_LOGO_UNBLEND")
        sr = m.SubtitleRemover(ArrayVideo(np.zeros((16, 144, 256, 3), np.uint8), fps=25.0))
        sr.opencv_inpaint = object()
        sr.append_output = lambda *a: None
        sr.run()
        assert calls == [("find_areas",)] and seen["active"] == [] and sr.unblend_plans == []
    finally:
        config.inpaintMode.value = old
        unblend.clear()


# ---- the order of the chain -----------------------------------------------------------------------------------------------------------
class Plugin:
    def __init__(self, log, accepts_device_frames):
        self.log, self.accepts_device_frames = log, accepts_device_frames

    def composite_mask(self, mask):
        return (np.asarray(mask) != 0).astype(np.uint8) * 255

    def sample_rows(self, mask):
        return 0, np.asarray(mask).shape[0]

    def body(self, frames, mask, **kw):
        self.log.append("body")
        if isinstance(frames, list):
            return [f.copy() for f in frames]
        return frames


@pytest.fixture
def recorded(monkeypatch):
    from vsr_amd.backend.tools import borrow, deflicker, glyph_key, regrain, seam_feather, tone_match, unblend

    log = []
    monkeypatch.setattr(tone_match, "sets", lambda cm, rows, device: ("bands", tuple(rows)))
    monkeypatch.setattr(regrain, "sets", lambda cm, rows, device: ("sets", tuple(rows)))
    monkeypatch.setattr(glyph_key, "mask", lambda cm, device: ("mask", int((cm != 0).sum())))
    monkeypatch.setattr(seam_feather, "alpha", lambda cm, feather, device: np.zeros(cm.shape, np.uint8))
    monkeypatch.setattr(tone_match, "apply", lambda frames, src, s, percent, y0=0: log.append(("tone", s, percent, y0)))
    monkeypatch.setattr(deflicker, "apply", lambda frames, src, s, radius, y0=0: log.append(("deflicker", s, radius, y0)))
    monkeypatch.setattr(regrain, "apply", lambda frames, src, s, percent, y0=0: log.append(("regrain", s, percent, y0)))
    monkeypatch.setattr(borrow, "apply", lambda frames, src, s, m, t, b, y0=0: log.append(("borrow", s, m, t, b, y0)))
    monkeypatch.setattr(glyph_key, "apply", lambda frames, src, m, t, y0=0: log.append(("key", m, t, y0)))
    monkeypatch.setattr(seam_feather, "composite", lambda frames, src, d, feather: log.append(("feather", feather)))
    monkeypatch.setattr(unblend, "apply",
                        lambda frames, src, plans, y0=0, H=None: log.append(("unblend", [p.box for p in plans], y0, H, src is not frames)))
    yield log
    unblend.clear()


@pytest.mark.parametrize("form", ["device tensor", "list, device body", "list, host body"])
def test_a_plugin_call_runs_unblend_last(monkeypatch, recorded, form):
    import torch

    from vsr_amd.backend.tools import seam_feather, unblend

    Hh, Ww = 24, 40
    mask = np.zeros((Hh, Ww), np.uint8)
    mask[10:16, 5:30] = 255
    frames = [np.full((Hh, Ww, 3), i, np.uint8) for i in range(3)]
    plugin = Plugin(recorded, accepts_device_frames=form != "list, host body")
    given = torch.from_numpy(np.stack(frames)) if form == "device tensor" else frames

    def call(these=given, **kw):
        del recorded[:]
        seam_feather.plugin_call(plugin, plugin.body, these, mask, "cpu", **kw)
        return list(recorded)

    for name in PASSES:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("VSR_LOGO_SCAN", "1")
    monkeypatch.setenv("VSR_LOGO_UNBLEND", "1")
    assert call() == ["body"], "no plans registered: the calls of before, whatever the environment says"
    box = (11, 15, 6, 20)
    unblend.register([FakePlan(box, Hh, Ww)])
    last = ("unblend", [box], 0, Hh, True)
    assert call() == ["body", last], "with plans the call clones its source though every other option is off"
    assert call(given[:1]) == ["body", last], "a single frame is un-mixed too"
    assert call(unmix=[]) == ["body"], "the keyword wins over the registry"
    monkeypatch.setenv("VSR_GLYPH_KEY", "12")
    monkeypatch.setenv("VSR_BORROW", "2")
    monkeypatch.setenv("VSR_SEAM_FEATHER", "4")
    monkeypatch.setenv("VSR_REGRAIN", "100")
    monkeypatch.setenv("VSR_DEFLICKER", "2")
    monkeypatch.setenv("VSR_TONE_MATCH", "80")
    chain = ["body", ("tone", ("bands", (0, Hh)), 80, 0), ("deflicker", ("sets", (0, Hh)), 2, 0), ("regrain", ("sets", (0, Hh)), 100, 0),
             ("borrow", ("sets", (0, Hh)), ("mask", 6 * 25), 12, 2, 0), ("key", ("mask", 6 * 25), 12, 0), ("feather", 4)]
    assert call() == chain + [last], "behind the feather"
    unblend.clear()
    assert call() == chain, "no plans: the six passes of before"


def test_strip_rows_reach_the_pass_as_picture_rows(monkeypatch, recorded):
    import torch

    from vsr_amd.backend.inpaint import sttn_auto_inpaint as sa
    from vsr_amd.backend.tools import seam_feather, unblend

    cm = np.zeros((48, 40), np.uint8)
    cm[20:30, 4:30] = 255
    strip = torch.zeros((2, 22, 40, 3), dtype=torch.uint8)
    box = (18, 32, 2, 34)
    seam_feather.device_call(strip, cm, lambda t: recorded.append("body"), 0, rows=(14, 36), sample_rows=(14, 36), unmix=[FakePlan(box, 48, 40)])
    assert recorded == ["body", ("unblend", [box], 14, 48, True)]

    class Engine:
        def auto_chunk(self, frames, mask, areas, **kw):
            recorded.append("body")

    plugin = object.__new__(sa.STTNInpaint)
    plugin.engine = Engine()
    for name in PASSES:
        monkeypatch.delenv(name, raising=False)
    del recorded[:]
    plugin.auto_chunk(strip, None, [(6, 16, 0, 40)], cmask=cm, rows=(14, 36))
    assert recorded == ["body"], "no plans: the call of before"
    unblend.register([FakePlan(box, 48, 40)])
    del recorded[:]
    plugin.auto_chunk(strip, None, [(6, 16, 0, 40)], cmask=cm, rows=(14, 36))
    assert recorded == ["body", ("unblend", [box], 14, 48, True)]


def test_pixels_outside_the_accepted_boxes_are_the_run_without_the_option(monkeypatch):
    """the chain on host tensors with the statement standing in for the kernel: the bytes outside the boxes are those of the call
    without plans, inside an accepted box they are the un-mixed source, whatever the body wrote there"""
    import torch

    from vsr_amd.backend.tools import seam_feather, unblend

    for name in PASSES:
        monkeypatch.delenv(name, raising=False)
    clean = st.wave()
    clip = us.blend(clean, 128)
    box = st.LOGO_AREA
    gt, ot = us.plan(sampled(clip), box)

    def apply(frames, src, plans, y0=0, H=None):
        for plan in plans:
            for f, s in zip(frames.numpy(), src.numpy()):
                us.unmix(f, s, plan.gt, plan.ot, plan.box, y0=y0)

    monkeypatch.setattr(unblend, "apply", apply)
    cm = np.zeros(clip.shape[1:3], np.uint8)
    cm[0:60, 180:256] = 255

    def call(rows=None, **kw):
        lo, hi = (0, clip.shape[1]) if rows is None else rows
        t = torch.from_numpy(clip[:4, lo:hi].copy())

        def strip_body(d):
            d[:, cm[lo:hi] != 0] = 7

        seam_feather.device_call(t, cm, strip_body, 0, rows=rows, **kw)
        return t.numpy()

    off = call()
    on = call(unmix=[FakePlan(box, clip.shape[1], clip.shape[2], gt, ot)])
    y0, y1, x0, x1 = box
    outside = np.ones(cm.shape, bool)
    outside[y0:y1, x0:x1] = False
    assert np.array_equal(on[:, outside], off[:, outside]) and (off[:, y0:y1, x0:x1] == 7).all()
    assert np.abs(on[:, y0:y1, x0:x1].astype(np.int64) - clean[:4, y0:y1, x0:x1]).max() <= 2
    strip = call(rows=(20, 70), unmix=[FakePlan(box, clip.shape[1], clip.shape[2], gt, ot)])
    assert np.array_equal(strip, on[:, 20:70]), "a strip that cuts the box holds the rows of the full-frame result"


# ---- the entry points without a device ------------------------------------------------------------------------------------------------
def test_argument_errors_then_no_gpu(built_lib):
    lib = built_lib.lib
    buf = (C.c_uint8 * 4096)()
    words = (C.c_uint32 * 1024)()
    p, q = C.cast(buf, C.c_void_p), C.cast(words, C.c_void_p)
    odd = C.c_void_p(q.value + 1)
    size = 8 * 8 * 3
    ok = dict(frames=p, fs=size, idx=q, n=2, H=8, W=8, gy0=1, gy1=6, gx0=2, gx1=8, first=1, S1=q, S2=q)

    def accum(**kw):
        a = dict(ok, **kw)
        return lib.vsr_unmix_accum(a["frames"], a["fs"], a["idx"], a["n"], a["H"], a["W"], a["gy0"], a["gy1"], a["gx0"], a["gx1"], a["first"],
                                   a["S1"], a["S2"], None)

    for kw in (dict(frames=None), dict(idx=None), dict(S1=None), dict(S2=None), dict(n=0), dict(n=65536), dict(H=0), dict(W=-1),
               dict(H=32768, W=32768), dict(gy0=-1), dict(gy1=9), dict(gy0=6), dict(gx1=9), dict(gx0=8), dict(first=2), dict(fs=size - 1),
               dict(S1=odd), dict(idx=odd)):
        assert accum(**kw) == built_lib.VSR_ERR_ARG, kw
        assert "logo unblend" in built_lib.last_error(), kw
    box = (C.c_int32 * 4)(2, 6, 1, 7)
    ok2 = dict(frames=p, fs=size, src=p, ss=size, g=q, o=q, n=2, H=8, W=8, y0=0, rows=8, box=box)

    def apply(**kw):
        a = dict(ok2, **kw)
        return lib.vsr_unmix_apply(a["frames"], a["fs"], a["src"], a["ss"], a["g"], a["o"], a["n"], a["H"], a["W"], a["y0"], a["rows"], a["box"],
                                   None)

    for kw in (dict(frames=None), dict(src=None), dict(g=None), dict(o=None), dict(box=None), dict(n=-1), dict(H=0), dict(y0=-1), dict(rows=0),
               dict(y0=4, rows=5), dict(fs=size - 1), dict(ss=size - 1), dict(box=(C.c_int32 * 4)(2, 9, 1, 7)), dict(box=(C.c_int32 * 4)(2, 6, 7, 7)),
               dict(box=(C.c_int32 * 4)(-1, 6, 1, 7)), dict(g=odd), dict(o=odd)):
        assert apply(**kw) == built_lib.VSR_ERR_ARG, kw
        assert "logo unblend" in built_lib.last_error(), kw
    small = 2 * 8 * 3
    assert apply(n=0) == 0, "no frame is success without a launch"
    assert apply(y0=6, rows=2, fs=small, ss=small) == 0 and apply(y0=0, rows=2, fs=small, ss=small) == 0, "a box outside the rows, likewise"
    if lib.vsr_device_count() <= 0:
        assert accum() == built_lib.VSR_ERR_NOGPU and apply() == built_lib.VSR_ERR_NOGPU
