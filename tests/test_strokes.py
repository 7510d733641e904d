"""--text-detect strokes without a GPU: what the statement tests/_strokes_statement.py finds on its test pictures, the
edges of a frame, the option with its refusals, the host's choice among components against the statement's, and the result format."""
import numpy as np
import pytest

from tests import _static_statement as ss
from tests import _strokes_statement as st


def margins(box, glyphs):
    """how far `box` reaches beyond the glyphs' box on the four sides (negative: it cuts into them)"""
    return (glyphs[0] - box[0], box[1] - glyphs[1], glyphs[2] - box[2], box[3] - glyphs[3])


# ---- the statement on its pictures ------------------------------------------------------------------------------------------------------
def test_constants_and_scale():
    assert (st.S, st.C, st.CELL, st.WX, st.WY, st.NV, st.NH, st.MINC, st.MIN_H) == (6, 48, 4, 5, 3, 64, 40, 2, 8)
    assert [st.scale(*s) for s in ((720, 1280), (1080, 1920), (2160, 3840), (144, 256), (1280, 720), (721, 1280), (8000, 8000))] == [1, 2, 3, 1, 1, 2, 8]


@pytest.mark.parametrize("k", (2, 3, 4))
@pytest.mark.parametrize("name", st.BACKGROUNDS)
def test_one_box_around_the_text(name, k):
    frame, glyphs = st.picture(name, k)
    found, scores = st.detect(frame)
    assert len(found) == 1 and scores.dtype == np.float32 and 0.25 <= float(scores[0]) <= 1.0, found
    m = margins(found[0], st.mask_box(glyphs))
    assert min(m) >= 0 and max(m) <= 12, f"the box {found[0]} holds the glyphs {st.mask_box(glyphs)} and exceeds them by at most 12: {m}"


@pytest.mark.parametrize("name", st.BACKGROUNDS)
def test_no_box_without_text(name):
    assert st.detect(st.background(name))[0] == []


def test_backgrounds_are_what_the_design_says():
    wave, noise, desk = (st.background(n)[..., 0].astype(np.int64) for n in st.BACKGROUNDS)
    assert np.abs(np.diff(wave, axis=0)).max() <= 3 and np.abs(np.diff(wave, axis=1)).max() <= 3, "at most 18 over S"
    assert np.abs(noise - wave).max() <= 12 and (noise != wave).mean() > 0.8, "range 24 + 18 < C: no ridge"
    v, h = st.ridges(noise)
    assert not v.any() and not h.any()
    v, h = st.ridges(desk)
    assert v.sum() > 500 and h.sum() < v.sum() // 8, "the stripes are ridges one way; the block's step edges are none"


@pytest.mark.parametrize("k", (6, 5))
def test_twice_the_size_at_F_2(k):
    frame, glyphs = st.large_picture(k)
    assert frame.shape == (288, 512, 3)
    found, _ = st.detect(frame, 2)
    assert len(found) == 1
    m = margins(found[0], st.mask_box(glyphs))
    assert min(m) >= 0 and max(m) <= 24, m


# ---- edges -----------------------------------------------------------------------------------------------------------------------------------
def test_stripes_alone_give_no_box():
    frame = ss.wave(1)[0]
    frame[20:120, 16:240] = np.where((np.arange(16, 240) // 4) % 2 == 0, 255, 0).astype(np.uint8)[None, :, None]
    cv, ch = st.cells(frame, 1)
    assert st.box_sum(cv, st.WX, st.WY).max() >= st.NV and not st.text_cells(cv, ch).any(), "strokes one way only"
    assert st.detect(frame)[0] == []


@pytest.mark.parametrize("F", (1, 2))
def test_a_row_cut_by_the_frame_stays_inside(F):
    H, W = 141 * F + F - 1, 250 * F + F - 1                  # h, w no multiples of the cell; rows and columns beyond h F, w F exist
    frame, glyphs = st.put_text(ss.wave(1, H, W)[0], "HELLO NATION", 3 * F, corner=(H - 15 * F, W - 150 * F), outline=2 * F)
    assert glyphs[-1].any() and glyphs[:, -1].any(), "the glyph row is cut by the bottom and the right edge"
    h, w = H // F, W // F
    cv, ch = st.cells(frame, F)
    assert cv.shape == (-(-h // 4), -(-w // 4)) and h % 4 and w % 4, "hc, wc are ceilings"
    found, _ = st.detect(frame, F)
    assert found, "(cut to 15 of its 21 rows, the line may come apart at the space)"
    for ymin, ymax, xmin, xmax in found:
        assert 0 <= ymin < ymax <= H and 0 <= xmin < xmax <= W
    assert max(b[1] for b in found) == H and max(b[3] for b in found) == W, "the last cells reach beyond h F, w F: clipped to H, W"


# ---- option, flag, refusals -------------------------------------------------------------------------------------------------------------
def test_option_parsing(monkeypatch):
    from vsr_amd.backend.tools import stroke_det as sd
    from vsr_amd.backend.tools.args_handler import parse_args

    assert sd.ENV == "VSR_TEXT_DETECT"
    assert sd.detect_option(env={}) == "model" and sd.detect_option(env={sd.ENV: ""}) == "model" and sd.detect_option(env={sd.ENV: "model"}) == "model"
    assert sd.detect_option(env={sd.ENV: "strokes"}) == "strokes" and sd.detect_option("strokes", env={}) == "strokes"
    assert sd.detect_option("model", env={sd.ENV: "strokes"}) == "model", "an argument wins over the environment"
    for bad in ("1", "stroke", "ocr", "none"):
        with pytest.raises(ValueError, match="text detector"):
            sd.detect_option(env={sd.ENV: bad})
    monkeypatch.setenv(sd.ENV, "strokes")
    assert sd.detect_option() == "strokes"
    monkeypatch.delenv(sd.ENV)
    assert sd.detect_option() == "model"
    assert parse_args(["-i", "x.y4m"]).text_detect is None
    assert parse_args(["-i", "x.y4m", "--text-detect", "strokes", "--inpaint-mode", "opencv"]).text_detect == "strokes"
    assert parse_args(["-i", "x.y4m", "--text-detect", "model"]).text_detect == "model"
    with pytest.raises(SystemExit):
        parse_args(["-i", "x.y4m", "--text-detect", "paddle"])


def test_flag_sets_the_environment_variable(monkeypatch):
    import os

    from vsr_amd.backend import main as m

    seen = {}

    class Stop(Exception):
        pass

    def fake_remover(path):
        seen["env"] = os.environ.get("VSR_TEXT_DETECT")
        raise Stop

    assert ("text_detect", "VSR_TEXT_DETECT", str) in m.FLAG_ENV
    monkeypatch.setenv("VSR_TEXT_DETECT", "model")
    monkeypatch.setattr(m, "SubtitleRemover", fake_remover)
    with pytest.raises(Stop):
        m.main(["-i", "x.y4m"])
    assert seen["env"] == "model", "without the flag the variable is left alone"
    with pytest.raises(Stop):
        m.main(["-i", "x.y4m", "--inpaint-mode", "opencv", "--text-detect", "strokes"])
    assert seen["env"] == "strokes"


class FakeDist:
    @staticmethod
    def get_world_size():
        return 2

    @staticmethod
    def get_rank():
        return 0


class Injected:
    def predict(self, img):
        return [{"dt_polys": np.zeros((0, 4, 2))}]


def test_refuse():
    from vsr_amd.backend.tools import stroke_det as sd

    assert sd.refuse(FakeDist, False, Injected(), "model") is False, "off: nothing is refused"
    assert sd.refuse(None, True, None, "strokes") is True
    with pytest.raises(RuntimeError, match="sttn-auto runs no text detector"):
        sd.refuse(None, False, None, "strokes")
    with pytest.raises(RuntimeError, match="contradicts the text detector .*Injected"):
        sd.refuse(None, True, Injected(), "strokes")
    with pytest.raises(RuntimeError, match="one process .world size 2"):
        sd.refuse(FakeDist, True, None, "strokes")
    with pytest.raises(ValueError, match="text detector"):
        sd.refuse(None, True, None, "both")


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


def remover(monkeypatch, value):
    """a SubtitleRemover over an in-memory clip whose reader and sink raise when touched: a refusal comes before either"""
    from vsr_amd.backend import main as m
    from vsr_amd.backend.tools.video_io import ArrayVideo

    if value is None:
        monkeypatch.delenv("VSR_TEXT_DETECT", raising=False)
    else:
        monkeypatch.setenv("VSR_TEXT_DETECT", value)
    for name in ("VSR_LOGO_SCAN", "VSR_LOGO_UNBLEND", "VSR_DET_MODEL_DIR", "VSR_DET_WEIGHTS"):
        monkeypatch.delenv(name, raising=False)
    clip = np.zeros((20, 144, 256, 3), np.uint8)
    sr = m.SubtitleRemover(ArrayVideo(clip, fps=25.0), device="cpu", model_path="unused")
    sr.append_output = lambda *a: None

    def touched(*a, **k):
        raise AssertionError("the run went on behind a refusal")

    sr._run = touched
    return sr


def test_run_refuses_before_any_work(monkeypatch):
    from vsr_amd.backend import main as m
    from vsr_amd.backend.tools.constant import InpaintMode

    with Mode(InpaintMode.OPENCV):
        with pytest.raises(ValueError, match="text detector: 'paddle'"):
            remover(monkeypatch, "paddle").run()
        sr = remover(monkeypatch, "strokes")
        sr.text_detector = Injected()
        with pytest.raises(RuntimeError, match="contradicts the text detector"):
            sr.run()
        sr = remover(monkeypatch, "strokes")
        monkeypatch.setattr(m.SubtitleRemover, "_distributed", staticmethod(lambda: FakeDist))
        with pytest.raises(RuntimeError, match="world size 2"):
            sr.run()
        monkeypatch.setattr(m.SubtitleRemover, "_distributed", staticmethod(lambda: None))
    with Mode(InpaintMode.STTN_AUTO):
        with pytest.raises(RuntimeError, match="sttn-auto runs no text detector"):
            remover(monkeypatch, "strokes").run()


@pytest.mark.parametrize("value", (None, "", "model"))
def test_off_touches_nothing_but_the_option(monkeypatch, built_lib, value):
    """unset, empty or `model`: the run reaches _run() as ever, the default detector is today's (none without weights), and of the new
    module nothing is called but detect_option -- no class made, no symbol of the library looked up"""
    from vsr_amd.backend.tools import stroke_det as sd
    from vsr_amd.backend.tools.constant import InpaintMode

    def never(*a, **k):
        raise AssertionError("the stroke detector was touched with the option off")

    for name in ("refuse", "select_boxes", "scale", "result"):
        monkeypatch.setattr(sd, name, never)
    monkeypatch.setattr(sd.StrokeTextDetection, "__init__", never)
    bound, before = set(built_lib.lazy_bound), dict(sd.stats)
    sr = remover(monkeypatch, value)
    reached = []
    sr._run = lambda scan, unmix, start: reached.append((scan, unmix))
    sr.text_detector = Injected()                                  # (with the option off an injected detector is no contradiction)
    for mode in (InpaintMode.OPENCV, InpaintMode.STTN_AUTO):
        with Mode(mode):
            sr.run()
    assert reached == [(False, False)] * 2
    assert sr._default_detector() is sr.text_detector
    sr.text_detector = None
    assert sr._default_detector() is None, "today's code: no weights configured, no detector"
    assert built_lib.lazy_bound == bound and sd.stats == before
    assert {"vsr_strokes_cells", "vsr_strokes_text"} <= set(built_lib.LAZY) <= set(built_lib.SIGNATURES)


def test_strokes_gives_the_stroke_detector(monkeypatch):
    from vsr_amd.backend.tools import stroke_det as sd

    made = []
    monkeypatch.setattr(sd.StrokeTextDetection, "__init__", lambda self, device=0: made.append(device))
    sr = remover(monkeypatch, "strokes")
    det = sr._default_detector()
    assert isinstance(det, sd.StrokeTextDetection) and made == [0] and sr._default_detector() is det, "one detector per run"
    assert det.batch_size == 8 and not hasattr(det, "clone"), "one lane, as an injected detector"
    for name in ("predict", "predict_batch", "predict_batch_device"):
        assert callable(getattr(det, name))
    mine = Injected()
    sr.text_detector = mine
    assert sr._default_detector() is mine


# ---- the host's choice among the components ---------------------------------------------------------------------------------------------
def planes(hc=20, wc=40):
    return np.zeros((hc, wc), np.int64), np.zeros((hc, wc), np.int64)


def both(comps, cv, ch, F=1, H=80, W=160):
    from vsr_amd.backend.tools import stroke_det as sd

    want, want_scores = st.boxes(comps, cv, ch, F, H, W)
    got, scores = sd.select_boxes(np.asarray(comps, np.int32).reshape(-1, 6), cv.astype(np.uint8), ch.astype(np.uint8), F, H, W)
    assert got == want and scores.dtype == np.float32 and np.array_equal(scores, want_scores)
    return got, scores


def test_constants_are_the_statements():
    from vsr_amd.backend.tools import stroke_det as sd

    assert (sd.S, sd.CONTRAST, sd.CELL, sd.WX, sd.WY, sd.NV, sd.NH, sd.MINC, sd.MIN_H) == (st.S, st.C, st.CELL, st.WX, st.WY, st.NV, st.NH, st.MINC, st.MIN_H)
    for shape in ((144, 256), (720, 1280), (1080, 1920), (1088, 1920), (2160, 3840), (4320, 7680), (9000, 9000)):
        assert sd.scale(*shape) == st.scale(*shape)


def test_each_keep_rule_rejects_what_it_should():
    cv, ch = planes()
    cv[4:7, 5:20] = 3                                                 # 3 x 15 cells of ink: 12 x 60 analysis pixels
    comp = (4 * 40 + 5, 99, 2, 25, 2, 9)                              # the component's box is larger than its ink
    got, scores = both([comp], cv, ch)
    assert got == [(16, 28, 20, 80)] and scores.tolist() == [1.0], "the tight box of the inked cells, in source pixels"
    # MINC: cells with one stroke pixel are no ink; cv + ch counts
    weak_v, weak_h = planes()
    weak_v[4:7, 5:20] = 1
    assert both([comp], weak_v, weak_h)[0] == [], "no inked cell: dropped"
    weak_h[4:7, 5:20] = 1
    assert both([comp], weak_v, weak_h)[0] == [(16, 28, 20, 80)]
    # MIN_H: one row of cells is 4 analysis pixels high
    low_v, low_h = planes()
    low_v[4, 5:20] = 3
    assert both([comp], low_v, low_h)[0] == []
    low_v[5, 5:20] = 3
    assert both([comp], low_v, low_h)[0] == [(16, 24, 20, 80)], "two rows: 8 pixels, kept"
    # ww >= 2 hh: 3 x 5 cells is 12 x 20
    short_v, short_h = planes()
    short_v[4:7, 5:10] = 3
    assert both([comp], short_v, short_h)[0] == []
    short_v[4:7, 5:11] = 3
    assert both([comp], short_v, short_h)[0] == [(16, 28, 20, 44)], "12 x 24: kept"
    # 4 inked >= cells: the corners span 4 x 16 = 64 cells
    thin_v, thin_h = planes()
    thin_v[2, 4] = thin_v[5, 19] = 3
    thin_v[3, 5:18] = 3                                               # 15 of 64
    assert both([comp], thin_v, thin_h)[0] == []
    thin_v[4, 5] = 3                                                  # 16 of 64
    got, scores = both([comp], thin_v, thin_h)
    assert got == [(8, 24, 16, 80)] and scores.tolist() == [0.25]


def test_boxes_scale_clip_and_sort():
    cv, ch = planes()
    cv[16:20, 28:40] = 2
    cv[16:20, 2:12] = 2
    cv[2:4, 10:30] = 2
    comps = [(7, 48, 28, 39, 16, 19), (5, 40, 2, 11, 16, 19), (3, 40, 10, 29, 2, 3)]
    got, _ = both(comps, cv, ch, F=2, H=157, W=317)
    assert got == [(16, 32, 80, 240), (128, 157, 16, 96), (128, 157, 224, 317)], "times CELL F, clipped to H, W, sorted by (ymin, xmin)"
    assert both(np.zeros((0, 6), np.int32), cv, ch)[0] == []


# ---- the result format ---------------------------------------------------------------------------------------------------------------------
def test_get_coordinates_gives_the_boxes_back():
    from vsr_amd.backend.tools import stroke_det as sd
    from vsr_amd.backend.tools.ocr import get_coordinates

    frame, _ = st.picture("desk", 3)
    found, scores = st.detect(frame)
    res = sd.result(found, scores)
    want = st.result(found, scores)[0]
    assert res["dt_polys"].dtype == np.int32 and res["dt_polys"].shape == (1, 4, 2) and res["dt_scores"].dtype == np.float32
    assert np.array_equal(res["dt_polys"], want["dt_polys"]) and np.array_equal(res["dt_scores"], want["dt_scores"])
    assert get_coordinates(res["dt_polys"].tolist()) == [(x0, x1, y0, y1) for y0, y1, x0, x1 in found]
    empty = sd.result([], np.zeros(0, np.float32))
    assert empty["dt_polys"].shape == (0, 4, 2) and empty["dt_scores"].shape == (0,)
