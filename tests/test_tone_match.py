"""--tone-match without a GPU: the statement (tests/_tone_statement.py) does what it is for on synthetic pictures, the option is parsed
in one place, several ranks are refused before any frame is read, and a plugin call runs its four passes in the stated order."""
import numpy as np
import pytest

from tests import _tone_statement as ts

SIZES = [(45, 75), (120, 200), (270, 480)]
STEP = np.array([7, -5, 12])


def box_mask(H, W):
    """one box whose long side exceeds 64 px, clear of the borders"""
    C = np.zeros((H, W), np.uint8)
    C[H * 2 // 3:H - 3, 4:4 + max(66, W // 2)] = 255
    assert C[:, -1].sum() == 0 and (C != 0).any(axis=0).sum() > 64
    return C


def constant(H, W):
    return np.broadcast_to(np.array([100, 120, 90], np.uint8), (1, H, W, 3)).copy()


def stepped(pic, C, step):
    fill = pic.copy()
    fill[:, C != 0] = (pic[:, C != 0].astype(np.int64) - step).astype(np.uint8)
    return fill


def test_constants():
    assert ts.BAND == 2 and ts.FINEST == 3 and ts.CLAMP == 24 * 64 and ts.DEN == 100 * 64 * 256 and ts.MAX_TONE == 100
    assert ts.top_level(45, 75) == 7 and ts.top_level(130, 260) == 9 and ts.top_level(8, 8) == 3 and ts.top_level(9, 8) == 4
    assert ts.top_level(1080, 1920) == 11 and ts.grid(1080, 1920, 3) == (135, 240) and ts.grid(1080, 1920, 11) == (1, 1)
    # the largest numerator of a pixel stays in 32 bits
    assert ts.MAX_TONE * 256 * ts.CLAMP + ts.DEN // 2 < 2 ** 31


def test_the_separable_bands_are_the_brute_force_bands():
    rng = np.random.default_rng(0)
    for k in range(24):
        H, W = (int(v) for v in rng.integers(5, 40, 2))
        C = ((rng.random((H, W)) < rng.choice([0.02, 0.3, 0.7, 0.98])) * rng.integers(1, 256)).astype(np.uint8)
        r0 = int(rng.integers(0, H))
        R = (r0, int(rng.integers(r0, H + 1))) if k % 3 else (0, H)
        for a, b in zip(ts.bands_brute(C, R), ts.bands(C, R)):
            assert np.array_equal(a, b), (H, W, R)
    # the frame border is no zero of C
    C = np.zeros((12, 12), np.uint8)
    C[6:] = 1
    E, M = ts.bands(C, (0, 12))
    assert E[4:6].all() and not E[:4].any() and M[6:8].all() and not M[8:].any()
    assert not any(s.any() for s in ts.bands(np.ones((9, 9), np.uint8), (0, 9)))
    assert np.array_equal(ts.cells(C, (0, 12)), [0, 1, 2, 3]) and np.array_equal(ts.cells(C, (0, 0)), [0, 1, 2, 3]), "cells of C count"
    assert np.array_equal(ts.cells(C[::-1], (0, 5)), [0, 1])


@pytest.mark.parametrize("size", SIZES)
def test_a_step_on_a_constant_picture_is_levelled_exactly(size):
    H, W = size
    C, pic = box_mask(H, W), constant(H, W)
    fill = stepped(pic, C, STEP)
    assert np.array_equal(ts.tone(fill, pic, C, (0, H), 100), pic), "every mean is exact: the picture comes back"
    half = ts.tone(fill, pic, C, (0, H), 50).astype(np.int64) - fill
    want = (50 * 64 * 256 * STEP + ts.DEN // 2) // ts.DEN                             # (4, -2, 6): halves round up
    assert want.tolist() == [4, -2, 6] and (half[:, C != 0] == want).all() and not half[:, C == 0].any()
    assert np.array_equal(ts.tone(pic, pic, C, (0, H), 100), pic), "a fill that matches is unchanged"
    # a fill that matches the picture but was inpainted (one byte differs deep inside): still nothing to level at the seam
    fill = pic.copy()
    ys, xs = np.nonzero(C)
    fill[0, ys[len(ys) // 2], xs[len(xs) // 2], 0] += 1
    info = []
    assert np.array_equal(ts.tone(fill, pic, C, (0, H), 100, info=info), fill) and info[0][3], "touched, and the field is zero"


@pytest.mark.parametrize("size", SIZES)
def test_a_ramp_is_followed_within_two_levels(size):
    """1/16 level per pixel along both axes, the fill 9 levels under it: the slope times the bands' 2 px centroid gap, plus the zero-order
    placement inside an 8-pixel cell (1/2 level), plus one rounding"""
    H, W = size
    C = box_mask(H, W)
    y, x = np.mgrid[0:H, 0:W]
    pic = np.repeat(((y + x) // 16 + 60)[None, :, :, None], 3, axis=3).astype(np.uint8)
    fill = stepped(pic, C, 9)
    out = ts.tone(fill, pic, C, (0, H), 100)
    err = int(np.abs(out.astype(np.int64) - pic)[:, C != 0].max())
    print(size, "largest error on the ramp:", err)
    assert err <= 2


@pytest.mark.parametrize("size", SIZES)
def test_what_is_left_alone(size):
    H, W = size
    C = box_mask(H, W)
    rng = np.random.default_rng(H)
    src = rng.integers(0, 256, (3, H, W, 3), dtype=np.uint8)
    fill = rng.integers(0, 256, (3, H, W, 3), dtype=np.uint8)                         # the body may write anywhere
    fill[1][C != 0] = src[1][C != 0]                                                  # a frame the call did not inpaint
    info = []
    out = ts.tone(fill, src, C, (0, H), 100, info=info)
    assert np.array_equal(out[:, C == 0], fill[:, C == 0]), "outside C every byte is the fill's"
    assert np.array_equal(out[1], fill[1]) and [i[3] for i in info] == [True, False, True]
    assert (out[0] != fill[0]).any() and (out[2] != fill[2]).any()
    assert np.array_equal(ts.tone(fill, src, C, (0, H), 0), fill), "S = 0 is the identity"
    # E or M empty: C covers all the rows held
    rows = (H * 2 // 3 + 2, H - 5)
    cover = np.zeros((H, W), np.uint8)
    cover[rows[0] - 6:rows[1] + 2] = 255
    info = []
    got = ts.tone(fill[:, rows[0]:rows[1]], src[:, rows[0]:rows[1]], cover, rows, 100, y0=rows[0], info=info)
    assert np.array_equal(got, fill[:, rows[0]:rows[1]]) and info[0][:2] == (0, 0)
    full = np.full((H, W), 255, np.uint8)
    assert np.array_equal(ts.tone(fill, src, full, (0, H), 100), fill)
    thin = np.zeros((H, W), np.uint8)                                                 # one row more than the rows held on either side:
    thin[rows[0] - 1:rows[1] + 1] = 255                                              # M reaches into them, E does not
    got = ts.tone(fill[:, rows[0]:rows[1]], src[:, rows[0]:rows[1]], thin, (0, H), 100, y0=rows[0], info=info)
    assert np.array_equal(got, fill[:, rows[0]:rows[1]]) and info[-1][0] == 0 and info[-1][1] > 0


@pytest.mark.parametrize("size", SIZES)
def test_strip_rows_state_the_rows_of_the_full_frame(size):
    H, W = size
    C = box_mask(H, W)
    rows = (H * 2 // 3 - 6, H)                                                        # C and its bands lie inside the strip
    E, M = ts.bands(C, (0, H))
    assert not (E | M)[:rows[0]].any() and np.array_equal(ts.bands(C, rows)[0], E)
    rng = np.random.default_rng(W)
    src = rng.integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    fill = src.copy()
    fill[:, C != 0] = rng.integers(0, 256, (2, int((C != 0).sum()), 3), dtype=np.uint8)
    full = ts.tone(fill, src, C, rows, 100)
    strip = ts.tone(fill[:, rows[0]:rows[1]], src[:, rows[0]:rows[1]], C, rows, 100, y0=rows[0])
    assert np.array_equal(strip, full[:, rows[0]:rows[1]]) and np.array_equal(full[:, :rows[0]], fill[:, :rows[0]])
    assert not np.array_equal(full, fill)


def test_a_step_beyond_the_clamp_is_levelled_by_24():
    H, W = SIZES[0]
    C, pic = box_mask(H, W), constant(H, W)
    fill = stepped(pic, C, np.array([40, -40, 24]))
    out = ts.tone(fill, pic, C, (0, H), 100).astype(np.int64) - fill
    assert (out[:, C != 0] == np.array([24, -24, 24])).all()


# ---- options and ranks ------------------------------------------------------------------------------------------------------------------
def test_option_parsing(monkeypatch):
    from vsr_amd.backend.tools import tone_match as tm
    from vsr_amd.backend.tools.args_handler import parse_args

    assert tm.tone_option(env={}) == 0 and tm.tone_option(env={"VSR_TONE_MATCH": ""}) == 0
    assert tm.tone_option(env={"VSR_TONE_MATCH": "37"}) == 37 and tm.tone_option(100, env={}) == 100
    assert tm.tone_option(3, env={"VSR_TONE_MATCH": "5"}) == 3, "an argument wins over the environment"
    for bad in ("-1", "101", "x", "1.5"):
        with pytest.raises(ValueError, match="tone match"):
            tm.tone_option(env={"VSR_TONE_MATCH": bad})
    for bad in (-1, 101, 1.5):
        with pytest.raises(ValueError, match="tone match"):
            tm.tone_option(bad)
    monkeypatch.setenv("VSR_TONE_MATCH", "4")
    assert tm.tone_option() == 4
    assert parse_args(["-i", "x.y4m"]).tone_match is None
    assert parse_args(["-i", "x.y4m", "--tone-match", "80"]).tone_match == 80
    for bad in ("101", "-1"):
        with pytest.raises(SystemExit):
            parse_args(["-i", "x.y4m", "--tone-match", bad])


def test_options_and_refusals_name_four(monkeypatch):
    from vsr_amd.backend.tools import seam_feather as sf

    for name, value in (("VSR_SEAM_FEATHER", "3"), ("VSR_REGRAIN", "150"), ("VSR_DEFLICKER", "2"), ("VSR_TONE_MATCH", "60")):
        monkeypatch.setenv(name, value)
    assert sf.options() == (3, 150, 2, 60) and sf.refuse_ranks_all(None) == (3, 150, 2, 60)
    for name in ("VSR_SEAM_FEATHER", "VSR_REGRAIN", "VSR_DEFLICKER", "VSR_TONE_MATCH"):
        monkeypatch.delenv(name)
    assert sf.options() == (0, 0, 0, 0)


def test_flag_sets_the_environment_variable(monkeypatch):
    from vsr_amd.backend import main as m

    seen = {}

    class Stop(Exception):
        pass

    def fake_remover(path):
        import os

        seen["env"] = os.environ.get("VSR_TONE_MATCH")
        raise Stop

    monkeypatch.setenv("VSR_TONE_MATCH", "0")
    monkeypatch.setattr(m, "SubtitleRemover", fake_remover)
    with pytest.raises(Stop):
        m.main(["-i", "x.y4m", "--tone-match", "80"])
    assert seen["env"] == "80"


class FakeDist:
    @staticmethod
    def get_world_size():
        return 2

    @staticmethod
    def get_rank():
        return 0


def others_off(monkeypatch):
    for name in ("VSR_SEAM_FEATHER", "VSR_REGRAIN", "VSR_DEFLICKER"):
        monkeypatch.delenv(name, raising=False)


@pytest.mark.parametrize("entry", ["run", "video_inpaint", "propainter_mode"])
def test_several_ranks_are_refused_before_a_frame_is_read(monkeypatch, entry):
    from vsr_amd.backend import main as m
    from vsr_amd.backend.tools import tone_match as tm
    from vsr_amd.backend.tools.subtitle_detect import SubtitleDetect
    from vsr_amd.backend.tools.video_io import ArrayVideo

    class Source(ArrayVideo):
        def read(self):
            raise AssertionError("a frame was read")

    def no_work(*a, **kw):
        raise AssertionError("work was started")

    sr = m.SubtitleRemover(Source(np.zeros((4, 48, 64, 3), np.uint8)))
    monkeypatch.setattr(sr, "_distributed", lambda: FakeDist)
    monkeypatch.setattr(SubtitleDetect, "find_subtitle_frame_no", no_work)
    monkeypatch.setattr(m, "STTNAutoInpaint", no_work)
    call = {"run": sr.run, "video_inpaint": lambda: sr.video_inpaint(None, no_work, text_detector=no_work),
            "propainter_mode": lambda: sr.propainter_mode(None, propainter_inpaint=no_work, text_detector=no_work)}[entry]
    others_off(monkeypatch)
    monkeypatch.setenv("VSR_TONE_MATCH", "80")
    with pytest.raises(RuntimeError, match="--tone-match .* one process"):
        call()
    monkeypatch.setenv("VSR_TONE_MATCH", "101")
    with pytest.raises(ValueError, match="tone match"):
        call()
    # off, or one rank: nothing is refused
    assert tm.refuse_ranks(FakeDist, 0) == 0 and tm.refuse_ranks(None, 80) == 80


def test_sttn_auto_refuses_several_ranks_before_the_source_is_opened(monkeypatch):
    from vsr_amd.backend.inpaint import sttn_auto_inpaint as sa

    def no_work(*a, **kw):
        raise AssertionError("the source was opened")

    monkeypatch.setattr(sa, "open_video", no_work)
    auto = object.__new__(sa.STTNAutoInpaint)
    auto.context = auto.scene_split = auto.lookahead = None
    auto.clip_gap = 50
    others_off(monkeypatch)
    monkeypatch.setenv("VSR_TONE_MATCH", "80")
    with pytest.raises(RuntimeError, match="--tone-match .* one process"):
        auto._run(FakeDist, None, None, None)


# ---- the order of the chain -----------------------------------------------------------------------------------------------------------
class Plugin:
    """a plugin whose body works on host arrays (the opencv kind) or on a device tensor in place"""
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
    """the four passes and their per-mask caches replaced by stand-ins that write down their names"""
    from vsr_amd.backend.tools import deflicker, regrain, seam_feather, tone_match

    log = []
    monkeypatch.setattr(tone_match, "sets", lambda cm, rows, device: ("bands", tuple(rows)))
    monkeypatch.setattr(regrain, "sets", lambda cm, rows, device: ("sets", tuple(rows)))
    monkeypatch.setattr(seam_feather, "alpha", lambda cm, feather, device: np.zeros(cm.shape, np.uint8))
    monkeypatch.setattr(tone_match, "apply", lambda frames, src, s, percent, y0=0: log.append(("tone", s, percent, y0)))
    monkeypatch.setattr(deflicker, "apply", lambda frames, src, s, radius, y0=0: log.append(("deflicker", s, radius, y0)))
    monkeypatch.setattr(regrain, "apply", lambda frames, src, s, percent, y0=0: log.append(("regrain", s, percent, y0)))
    monkeypatch.setattr(seam_feather, "composite", lambda frames, src, d, feather: log.append(("feather", feather)))
    return log


@pytest.mark.parametrize("form", ["device tensor", "list, device body", "list, host body"])
def test_a_plugin_call_runs_the_four_passes_in_order(monkeypatch, recorded, form):
    import torch

    from vsr_amd.backend.tools import seam_feather

    H, W = 24, 40
    mask = np.zeros((H, W), np.uint8)
    mask[10:16, 5:30] = 255
    frames = [np.full((H, W, 3), i, np.uint8) for i in range(3)]
    plugin = Plugin(recorded, accepts_device_frames=form != "list, host body")
    given = torch.from_numpy(np.stack(frames)) if form == "device tensor" else frames

    def call():
        del recorded[:]
        seam_feather.plugin_call(plugin, plugin.body, given, mask, "cpu")
        return list(recorded)

    for name in ("VSR_SEAM_FEATHER", "VSR_REGRAIN", "VSR_DEFLICKER", "VSR_TONE_MATCH"):
        monkeypatch.delenv(name, raising=False)
    assert call() == ["body"], "every option off: the body alone"
    monkeypatch.setenv("VSR_TONE_MATCH", "80")
    assert call() == ["body", ("tone", ("bands", (0, H)), 80, 0)]
    monkeypatch.setenv("VSR_SEAM_FEATHER", "4")
    monkeypatch.setenv("VSR_REGRAIN", "100")
    monkeypatch.setenv("VSR_DEFLICKER", "2")
    assert call() == ["body", ("tone", ("bands", (0, H)), 80, 0), ("deflicker", ("sets", (0, H)), 2, 0),
                      ("regrain", ("sets", (0, H)), 100, 0), ("feather", 4)]
    monkeypatch.setenv("VSR_TONE_MATCH", "0")
    assert call() == ["body", ("deflicker", ("sets", (0, H)), 2, 0), ("regrain", ("sets", (0, H)), 100, 0), ("feather", 4)]


def test_strip_rows_reach_the_pass_as_picture_rows(recorded):
    import torch

    from vsr_amd.backend.tools import seam_feather

    cm = np.zeros((48, 40), np.uint8)
    cm[20:30, 4:30] = 255
    strip = torch.zeros((2, 22, 40, 3), dtype=torch.uint8)
    seam_feather.device_call(strip, cm, lambda t: recorded.append("body"), 0, rows=(14, 36), sample_rows=(14, 36), tone=55)
    assert recorded == ["body", ("tone", ("bands", (14, 36)), 55, 14)]
