"""--logo-scan without a GPU: the numpy statement on the design's clips, the sample numbers, the host's choice among
the components, the option and its refusals, and what run() does with the areas in every mode (the scan itself monkeypatched)."""
import ctypes as C

import numpy as np
import pytest

from tests import _static_statement as ss


# ---- the statement ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def verdicts():
    """{clip name: (areas, info)} of the statement on the five clips of the design's table, computed once"""
    out = {}
    for name in ("clip_logo", "clip_still_logo", "clip_letterbox_logo", "clip_plain", "clip_desk_logo"):
        info = []
        out[name] = (ss.areas(getattr(ss, name)(), info), info)
    return out


def test_the_wave_is_what_the_design_says():
    clip = ss.wave()
    assert clip.shape == (40, 144, 256, 3) and clip.dtype == np.uint8
    lo, hi, e = ss.accumulate(clip)
    assert max(int(ss.gradient(ss.luma(f)).max()) for f in clip[:3]) <= 12 and int(e.max()) == 0
    # (40 frames visit 40 of the 64 phases, one step of 3 short of the full swing at some pixels)
    assert int((hi - lo).max()) == 96 and int((hi - lo).min()) == 93 >= ss.MV


def test_logo_on_the_moving_wave(verdicts):
    areas, info = verdicts["clip_logo"]
    y0, y1, x0, x1 = ss.LOGO
    assert areas == [ss.LOGO_AREA] == [(y0 - 11, y1 + 11, x0 - 11, x1 + 11)], "the logo's box grown by 1 + D + PAD"
    assert info == [((5, 43, 193, 247), "kept", 3777, 3777)]


def test_logo_on_the_still_wave(verdicts):
    areas, info = verdicts["clip_still_logo"]
    assert areas == [] and info == [((5, 43, 193, 247), "still", 0, 3777)], "a static shot tells nothing"


def test_letterbox_bars_and_the_logo(verdicts):
    areas, info = verdicts["clip_letterbox_logo"]
    assert areas == [ss.LOGO_AREA]
    assert [v for _, v, _, _ in info] == ["kept"] and info[0][2] < info[0][3], "the bar's rows of the ring stand still"


def test_no_logo(verdicts):
    assert verdicts["clip_plain"] == ([], [])


def test_still_desk_and_the_logo(verdicts):
    areas, info = verdicts["clip_desk_logo"]
    assert areas == [ss.LOGO_AREA]
    desk = [i for i in info if i[1] != "kept"]
    assert len(desk) == 1 and desk[0][1] == "large"
    y0, y1, x0, x1 = desk[0][0]
    assert y1 - y0 == 54 > ss.CLIP_H // 3 == 48 and x1 - x0 <= ss.CLIP_W // 3


def test_pieces_of_a_clip_accumulate_to_the_whole():
    rng = np.random.default_rng(0)
    clip = rng.integers(0, 256, (7, 9, 11, 3), dtype=np.uint8)
    whole = ss.accumulate(clip)
    parts = ss.accumulate(clip[4:], state=ss.accumulate(clip[:4]))
    assert all(np.array_equal(a, b) for a, b in zip(whole, parts))
    Y = ss.luma(clip[0])
    g = ss.gradient(Y)
    assert g[0, 0] == abs(Y[0, 1] - Y[0, 0]) + abs(Y[1, 0] - Y[0, 0]) and g[8, 10] == abs(Y[8, 10] - Y[8, 9]) + abs(Y[8, 10] - Y[7, 10])
    seed = np.zeros((20, 30), bool)
    seed[0, 0] = seed[10, 15] = True
    grown = ss.dilate(seed, ss.D)
    assert grown.sum() == 7 * 7 + 13 * 13 and grown[4:17, 9:22].all(), "one stray seed grows to 169"


# ---- the module against the statement -------------------------------------------------------------------------------------------------
def test_constants_are_the_statements():
    from vsr_amd.backend.tools import logo_scan as ls

    for name in ("GE", "MV", "D", "MAX_SAMPLES", "MIN_FRAMES", "MIN_AREA", "RING", "PAD", "MAX_AREAS"):
        assert getattr(ls, name) == getattr(ss, name), name
    assert (ls.GE, ls.MV, ls.D, ls.MIN_AREA, ls.RING, ls.PAD, ls.MAX_AREAS) == (24, 48, 6, 400, 24, 4, 8)


@pytest.mark.parametrize("N", [16, 17, 119, 120, 121, 1200, 100000])
def test_sample_indices(N):
    from vsr_amd.backend.tools import logo_scan as ls

    idx = ls.sample_indices(N)
    M = min(N, 120)
    assert idx == ss.sample_indices(N) == [(k * N) // M for k in range(M)]
    assert len(idx) == M and idx[0] == 0 and idx[-1] < N
    assert all(b > a for a, b in zip(idx, idx[1:])), "distinct and increasing"
    if N <= 120:
        assert idx == list(range(N)), "every frame of a short clip"
    if N == 1200:
        assert idx == list(range(0, 1200, 10))


@pytest.mark.parametrize("N", [15, 1, 0])
def test_a_short_clip_is_refused(N):
    from vsr_amd.backend.tools import logo_scan as ls

    with pytest.raises(ValueError, match="at least 16"):
        ls.sample_indices(N)
    with pytest.raises(ValueError):
        ss.sample_indices(N)


def ccl_rows(comps):
    """the statement's components as the rows vsr_det_launch_ccl gives: (label, area, xmin, xmax, ymin, ymax), boxes inclusive"""
    return np.array([(k, a, x0, x1 - 1, y0, y1 - 1) for k, (a, y0, y1, x0, x1) in enumerate(comps)], np.int32).reshape(-1, 6)


@pytest.mark.parametrize("name", ["clip_logo", "clip_still_logo", "clip_letterbox_logo", "clip_plain", "clip_desk_logo"])
def test_the_hosts_choice_is_the_statements(verdicts, name):
    from vsr_amd.backend.tools import logo_scan as ls

    clip = getattr(ss, name)()
    M = len(clip)
    grown, moving = ss.classify(*ss.accumulate(clip), M - M // 8)
    got, dropped = ls.select_areas(ccl_rows(ss.components(grown)), moving.astype(np.uint8))
    assert got == verdicts[name][0] and dropped == 0


def test_at_most_eight_areas_the_largest_first():
    from vsr_amd.backend.tools import logo_scan as ls

    H, W = 400, 900
    moving = np.ones((H, W), np.uint8)
    comps = [(400 + 10 * (k % 5), 10 + 36 * k, 10 + 36 * k + 20, 5 + 80 * k, 5 + 80 * k + 25 + k) for k in range(10)]   # areas tie in pairs
    info = []
    want = ss.select(comps, moving.astype(bool), info)
    got, dropped = ls.select_areas(ccl_rows(comps), moving)
    assert got == want and len(got) == 8 and dropped == 2 and info[-1] == ("dropped", 2)
    assert got == sorted(got, key=lambda b: (b[0], b[2]))
    gone = {(10 + 36 * k - 4, 10 + 36 * k + 24, 5 + 80 * k - 4, 5 + 80 * k + 25 + k + 4) for k in (0, 5)}
    assert len(gone) == 2 and not gone & set(got), "the two smallest (400 pixels), the one nearer the top among equals kept first"
    assert ls.select_areas(np.zeros((0, 6), np.int32), moving) == ([], 0)


# ---- option, flag, refusal ----------------------------------------------------------------------------------------------------------------
def test_option_parsing(monkeypatch):
    from vsr_amd.backend.tools import logo_scan as ls
    from vsr_amd.backend.tools.args_handler import parse_args

    assert ls.ENV == "VSR_LOGO_SCAN"
    assert ls.scan_option(env={}) is False and ls.scan_option(env={"VSR_LOGO_SCAN": ""}) is False
    assert ls.scan_option(env={"VSR_LOGO_SCAN": "0"}) is False and ls.scan_option(env={"VSR_LOGO_SCAN": "1"}) is True
    assert ls.scan_option(1, env={}) is True and ls.scan_option(True, env={}) is True
    assert ls.scan_option(0, env={"VSR_LOGO_SCAN": "1"}) is False, "an argument wins over the environment"
    for bad in ("2", "yes", "-1", "1.5"):
        with pytest.raises(ValueError, match="logo scan"):
            ls.scan_option(env={"VSR_LOGO_SCAN": bad})
    monkeypatch.setenv("VSR_LOGO_SCAN", "1")
    assert ls.scan_option() is True
    monkeypatch.delenv("VSR_LOGO_SCAN")
    assert ls.scan_option() is False
    assert parse_args(["-i", "x.y4m"]).logo_scan is False
    assert parse_args(["-i", "x.y4m", "--logo-scan"]).logo_scan is True
    with pytest.raises(SystemExit):
        parse_args(["-i", "x.y4m", "--logo-scan", "1"])


def test_flag_sets_the_environment_variable(monkeypatch):
    import os

    from vsr_amd.backend import main as m

    seen = {}

    class Stop(Exception):
        pass

    def fake_remover(path):
        seen["env"] = os.environ.get("VSR_LOGO_SCAN")
        raise Stop

    entry = [e for e in m.FLAG_ENV if e[0] == "logo_scan"]
    assert len(entry) == 1 and entry[0][1] == "VSR_LOGO_SCAN" and entry[0][2](True) == "1"
    monkeypatch.setenv("VSR_LOGO_SCAN", "0")
    monkeypatch.setattr(m, "SubtitleRemover", fake_remover)
    with pytest.raises(Stop):
        m.main(["-i", "x.y4m"])
    assert seen["env"] == "0", "without the flag the variable is left alone"
    with pytest.raises(Stop):
        m.main(["-i", "x.y4m", "--logo-scan"])
    assert seen["env"] == "1"


class FakeDist:
    @staticmethod
    def get_world_size():
        return 2

    @staticmethod
    def get_rank():
        return 0


def test_refuse_ranks(monkeypatch):
    from vsr_amd.backend.tools import logo_scan as ls

    monkeypatch.delenv("VSR_LOGO_SCAN", raising=False)
    assert ls.refuse_ranks(None) is False and ls.refuse_ranks(FakeDist) is False and ls.refuse_ranks(None, 1) is True
    with pytest.raises(RuntimeError, match="--logo-scan .* one process"):
        ls.refuse_ranks(FakeDist, 1)
    monkeypatch.setenv("VSR_LOGO_SCAN", "1")
    with pytest.raises(RuntimeError, match="world size 2"):
        ls.refuse_ranks(FakeDist)
    monkeypatch.setenv("VSR_LOGO_SCAN", "7")
    with pytest.raises(ValueError, match="logo scan"):
        ls.refuse_ranks(None)


# ---- run() ---------------------------------------------------------------------------------------------------------------------------------
N, H, W = 40, 144, 256
AREAS = [(1, 47, 189, 251), (60, 130, 20, 50)]           # the second is taller than wide by more than subtitleYXAxisDifferencePixel


def flipped(areas):
    return [(xmin, xmax, ymin, ymax) for ymin, ymax, xmin, xmax in areas]


class Mode:
    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        from vsr_amd.backend.config import config

        self.old = config.inpaintMode.value
        config.inpaintMode.value = self.mode

    def __exit__(self, *exc):
        from vsr_amd.backend.config import config

        config.inpaintMode.value = self.old


def remover(monkeypatch, found, scan=True):
    """a SubtitleRemover over an in-memory clip whose scan is `found` (or raises when it must not run) -> (remover, calls of the scan)"""
    from vsr_amd.backend import main as m
    from vsr_amd.backend.tools import logo_scan as ls
    from vsr_amd.backend.tools.video_io import ArrayVideo

    calls = []

    def fake_find(video, device=0, clip=None, report=None):
        calls.append(video)
        if not scan:
            raise AssertionError("the scan ran with the option off")
        return list(found)

    monkeypatch.setattr(ls, "find_areas", fake_find)
    if scan:
        monkeypatch.setenv("VSR_LOGO_SCAN", "1")
    else:
        monkeypatch.delenv("VSR_LOGO_SCAN", raising=False)
    clip = np.zeros((N, H, W, 3), np.uint8)
    clip[:, 0, 0, 0] = np.arange(N)
    sr = m.SubtitleRemover(ArrayVideo(clip, fps=25.0), device="cpu", model_path="unused")
    sr.append_output = lambda *a: None
    return sr, calls


@pytest.mark.parametrize("boxes", [[], [(100, 140, 10, 200)]], ids=["no -c", "-c"])
def test_sttn_auto_masks_the_areas(monkeypatch, boxes):
    from vsr_amd.backend import main as m
    from vsr_amd.backend.tools.constant import InpaintMode
    from vsr_amd.backend.tools.inpaint_tools import create_mask

    masks = []

    class FakeAuto:
        last_error = None

        def __init__(self, device, model_path, video_path):
            pass

        def __call__(self, input_mask, input_sub_remover, tbar):
            masks.append(input_mask.copy())

    monkeypatch.setattr(m, "STTNAutoInpaint", FakeAuto)
    sr, calls = remover(monkeypatch, AREAS)
    sr.sub_areas = list(boxes)
    with Mode(InpaintMode.STTN_AUTO):
        sr.run()
    assert len(calls) == 1 and sr.static_areas == AREAS and "logo scan" in sr.phase_seconds
    assert len(masks) == 1 and np.array_equal(masks[0], create_mask((H, W), flipped(list(boxes) + AREAS)))
    assert masks[0].any() and not masks[0].all(), "the areas, not the whole-frame default"
    # nothing found: -c alone as ever; without -c there is nothing to inpaint
    del masks[:]
    sr, _ = remover(monkeypatch, [])
    sr.sub_areas = list(boxes)
    with Mode(InpaintMode.STTN_AUTO):
        if boxes:
            sr.run()
            assert np.array_equal(masks[0], create_mask((H, W), flipped(boxes)))
        else:
            with pytest.raises(Exception, match="No static overlay found"):
                sr.run()
            assert masks == []


class NoText:
    def predict(self, img):
        return [{"dt_polys": np.zeros((0, 4, 2))}]


class TextOnSome:
    """a line of text on the 0-based frames 10 .. 19"""
    quad = np.array([[[40, 100], [120, 100], [120, 115], [40, 115]]])

    def predict(self, img):
        return [{"dt_polys": self.quad if 10 <= int(img[0, 0, 0]) < 20 else np.zeros((0, 4, 2))}]


@pytest.mark.parametrize("boxes", [[], [(90, 130, 0, 200)]], ids=["no -c", "-c"])
def test_video_inpaint_masks_the_areas_on_frames_without_text(monkeypatch, boxes):
    from vsr_amd.backend.tools.constant import InpaintMode
    from vsr_amd.backend.tools.inpaint_tools import create_mask

    seen = []

    def model(batch, mask):
        seen.append(([int(f[0, 0, 0]) for f in batch], mask.copy()))
        return [f for f in batch]

    sr, calls = remover(monkeypatch, AREAS)
    sr.sub_areas = list(boxes)
    sr.text_detector, sr.opencv_inpaint = TextOnSome(), model
    with Mode(InpaintMode.OPENCV):
        sr.run()
    assert len(calls) == 1 and sr.static_areas == AREAS
    assert sr.sub_areas == (list(boxes) or [(0, H, 0, W)]), "-c keeps restricting the text detector only"
    assert sorted(i for b, _ in seen for i in b) == list(range(N)), "every frame is inpainted"
    logo_only = create_mask((H, W), flipped(AREAS))
    text = (40, 120, 100, 115)
    both = create_mask((H, W), [text] + flipped(AREAS))
    assert not np.array_equal(logo_only, both)
    for frames, mask in seen:
        assert (mask[logo_only != 0] == 255).all(), "both areas, the tall one too, on every batch"
        # (the detector samples every second frame: it saw the text on the 0-based frames 10, 12 .. 18; where the intervals are cut is the
        # code's as it is)
        assert np.array_equal(mask, both) if any(10 <= f <= 18 for f in frames) else np.array_equal(mask, logo_only)
    assert any(np.array_equal(mask, logo_only) for _, mask in seen), "a batch where the detector found nothing"


def test_propainter_mode_masks_the_areas(monkeypatch):
    from vsr_amd.backend.tools.constant import InpaintMode
    from vsr_amd.backend.tools.inpaint_tools import create_mask

    seen = []

    def plugin(batch, mask):
        seen.append((len(batch), mask.copy()))
        return [f for f in batch]

    sr, _ = remover(monkeypatch, AREAS[:1])
    sr.text_detector, sr.propainter_inpaint, sr.scene_div_points = NoText(), plugin, []
    with Mode(InpaintMode.PROPAINTER):
        sr.run()
    assert sum(n for n, _ in seen) == N and len(sr.video_writer.frames) == N
    assert all(np.array_equal(mask, create_mask((H, W), flipped(AREAS[:1]))) for _, mask in seen)


def test_off_is_off(monkeypatch):
    """without the option: the scan is not called, its counters stay zero, and a clip without text fails as it does today"""
    from vsr_amd.backend.tools import logo_scan as ls
    from vsr_amd.backend.tools.constant import InpaintMode

    before = dict(ls.stats)
    assert set(before) == {"scans", "frames", "accum_launches", "components", "areas", "dropped"}
    sr, calls = remover(monkeypatch, AREAS, scan=False)
    sr.text_detector, sr.opencv_inpaint = NoText(), lambda batch, mask: batch
    with Mode(InpaintMode.OPENCV):
        with pytest.raises(Exception, match="No subtitle detected"):
            sr.run()
    assert calls == [] and sr.static_areas == [] and "logo scan" not in sr.phase_seconds
    assert ls.stats == before and not any(before.values())


def test_refusals_come_before_a_frame_is_read(monkeypatch):
    from vsr_amd.backend import main as m
    from vsr_amd.backend.tools.constant import InpaintMode
    from vsr_amd.backend.tools.video_io import ArrayVideo

    class Source(ArrayVideo):
        def read(self):
            raise AssertionError("a frame was read")

    sr = m.SubtitleRemover(Source(np.zeros((4, 48, 64, 3), np.uint8)))
    monkeypatch.setattr(m.SubtitleRemover, "_distributed", staticmethod(lambda: FakeDist))
    monkeypatch.setenv("VSR_LOGO_SCAN", "1")
    with Mode(InpaintMode.OPENCV):
        with pytest.raises(RuntimeError, match="--logo-scan"):
            sr.run()
    monkeypatch.setenv("VSR_LOGO_SCAN", "maybe")
    monkeypatch.setattr(m.SubtitleRemover, "_distributed", staticmethod(lambda: None))
    with Mode(InpaintMode.OPENCV):
        with pytest.raises(ValueError, match="logo scan"):
            sr.run()


# ---- the entry points without a device ----------------------------------------------------------------------------------------------------
def test_entry_points_without_a_device(built_lib):
    """argument errors first, then no device -- never a plane made up on the host"""
    lib = built_lib.lib
    Hh, Ww, n = 8, 16, 2
    frames, idx = np.zeros((n, Hh, Ww, 3), np.uint8), np.arange(n, dtype=np.int32)
    lo, hi, edges = np.zeros((Hh, Ww), np.uint8), np.zeros((Hh, Ww), np.uint8), np.zeros((Hh, Ww), np.uint16)
    grown, moving = np.zeros((Hh, Ww), np.float32), np.zeros((Hh, Ww), np.uint8)
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    fs = Hh * Ww * 3
    ok = dict(frames=P(frames), fs=fs, idx=P(idx), n=n, H=Hh, W=Ww, ge=24, first=1, lo=P(lo), hi=P(hi), edges=P(edges))

    def accum(**kw):
        a = dict(ok, **kw)
        return lib.vsr_static_accum(a["frames"], a["fs"], a["idx"], a["n"], a["H"], a["W"], a["ge"], a["first"], a["lo"], a["hi"], a["edges"], None)

    for bad in (dict(frames=None), dict(idx=None), dict(lo=None), dict(hi=None), dict(edges=None), dict(n=0), dict(n=-1), dict(n=65536),
                dict(H=0), dict(W=-3), dict(H=32768, W=32768), dict(ge=-1), dict(ge=511), dict(first=2), dict(fs=fs - 1)):
        assert accum(**bad) == built_lib.VSR_ERR_ARG, bad
        assert "logo scan" in built_lib.last_error()
    okc = dict(lo=P(lo), hi=P(hi), edges=P(edges), H=Hh, W=Ww, need=2, mv=48, grow=6, grown=P(grown), moving=P(moving))

    def classify(**kw):
        a = dict(okc, **kw)
        return lib.vsr_static_classify(a["lo"], a["hi"], a["edges"], a["H"], a["W"], a["need"], a["mv"], a["grow"], a["grown"], a["moving"], None)

    for bad in (dict(lo=None), dict(hi=None), dict(edges=None), dict(grown=None), dict(moving=None), dict(H=0), dict(W=0), dict(need=-1),
                dict(need=65537), dict(mv=-1), dict(mv=257), dict(grow=-1), dict(grow=17)):
        assert classify(**bad) == built_lib.VSR_ERR_ARG, bad
        assert "logo scan" in built_lib.last_error()
    if lib.vsr_device_count() > 0:
        return                                           # (host buffers: nothing may be launched on them)
    assert accum() == built_lib.VSR_ERR_NOGPU and "no CPU fallback" in built_lib.last_error()
    assert classify() == built_lib.VSR_ERR_NOGPU and "no CPU fallback" in built_lib.last_error()
    assert not lo.any() and not edges.any() and not grown.any()
    from vsr_amd.backend.tools import logo_scan as ls

    with pytest.raises(RuntimeError, match="no HIP device"):
        ls.Scan(Hh, Ww)
