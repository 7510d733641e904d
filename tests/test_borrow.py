"""--borrow without a GPU: the statement (tests/_borrow_statement.py) does what it is for on a worked clip and keeps the properties that
follow from its definition, its bit-parallel N is its brute-force N, the option is parsed in one place, T = 0 and several ranks are
refused before any frame is read, a plugin call runs its passes in the stated order, and the entry points refuse bad arguments.

Grain heavier than T allows is the key's known limit, not this pass's: at sigma = 6 with independent grain in the fill, T = 12 seeds
everywhere and nothing lends.  The clips here use sigma = 2, at which the statement alone keeps every "every pixel" claim below."""
import ctypes as C

import numpy as np
import pytest

from tests import _borrow_statement as bs
from tests import _key_statement as ks

T = 12
H, W, BOX = 64, 150, (20, 48, 10, 140)
ROWS = (0, H)


def worked(seed=0, n=6, sigma=2.0):
    """6 frames of 64 x 150: a ramp with grain; the fill is the ramp with another draw of the grain inside the box mask; a 5 x 7 block
    of +120 at rows 30..34, columns 40..46 on frames 0-2 and at columns 90..96 on frames 3-5"""
    rng = np.random.default_rng(seed)
    Cm = np.zeros((H, W), np.uint8)
    Cm[BOX[0]:BOX[1], BOX[2]:BOX[3]] = 255
    y, x = np.mgrid[0:H, 0:W]
    ramp = (40 + 0.5 * x + 0.25 * y)[None, :, :, None] + np.zeros((n, 1, 1, 3))
    src = np.rint(ramp + rng.normal(0, sigma, ramp.shape))
    other = np.clip(np.rint(ramp + rng.normal(0, sigma, ramp.shape)), 0, 255).astype(np.uint8)
    src[:n // 2, 30:35, 40:47] += 120
    src[n // 2:, 30:35, 90:97] += 120
    src = np.clip(src, 0, 255).astype(np.uint8)
    fill = src.copy()
    fill[:, Cm != 0] = other[:, Cm != 0]
    return fill, src, Cm


def test_constants():
    assert bs.MAX_BORROW == 8 and bs.TH == 24 and bs.FULL == 16
    assert [bs.threshold(b) for b in (0, 1, 8, 16)] == [0, 1, 12, 24]
    assert bs.lenders(3, 6, 3) == [2, 4, 1, 5, 0] and bs.lenders(0, 6, 2) == [1, 2] and bs.lenders(5, 6, 8) == [4, 3, 2, 1, 0]
    assert bs.workspace_bytes(1080, 1920, 50) == 2 * 50 * 1080 * 30 * 8
    assert bs.pair_weight(0, 0, 0, 0) == 0 and bs.pair_weight(0, 0, 0, 30) == 16 and bs.pair_weight(120, 0, 0, 30) == 0
    assert bs.pair_weight(75, 0, 0, 30) == 8


@pytest.mark.parametrize("Wd", [63, 64, 65, 130])
def test_the_bit_parallel_reach_is_the_brute_force_reach(Wd):
    rng = np.random.default_rng(Wd)
    for h in (1, 7, 20, 33):
        Z = rng.random((2, h, Wd)) < 0.004
        Z[0, 0, 0] = Z[1, -1, -1] = True
        if Wd > 64:
            Z[0, h // 2, 56] = Z[1, h // 2, min(72, Wd - 1)] = True
        assert np.array_equal(ks.unpack_words(bs.near_words(ks.pack_words(Z)), Wd), bs.near(Z)), (h, Wd)


@pytest.mark.parametrize("seed", [0, 1])
def test_the_worked_clip(seed):
    fill, src, Cm = worked(seed)
    info = {}
    out = bs.borrow(fill, src, Cm, ROWS, T, 3, info=info)
    assert set(info["b"].values()) == {16}, "a still scene: every pair is open"
    assert [int(v) for v in info["borrowers"].sum(axis=(1, 2))] == [483] * 6
    assert (info["lender"][info["borrowers"]] >= 0).all(), "all 483 borrowers of every frame take a real pixel"
    for t in range(6):
        cols = slice(40, 47) if t < 3 else slice(90, 97)
        lender = info["lender"][t, 30:35, cols]
        assert lender.size == 35 and ((lender >= 3) if t < 3 else (lender < 3) & (lender >= 0)).all()
        for yy in range(5):
            for xx in range(7):
                assert np.array_equal(out[t, 30 + yy, cols][xx], src[lender[yy, xx], 30 + yy, cols][xx])
    assert np.array_equal(out[:, Cm == 0], fill[:, Cm == 0]), "nothing outside C is written"
    assert np.abs(out.astype(int) - fill).max() < 24
    keyed = ks.key(out, src, Cm, T)
    assert not np.array_equal(keyed, ks.key(fill, src, Cm, T))
    info1 = {}
    bs.borrow(fill, src, Cm, ROWS, T, 1, info=info1)
    taken = [int(v) for v in (info1["lender"] >= 0).sum(axis=(1, 2))]
    assert taken == [0, 0, 483, 483, 0, 0], "B = 1: only frames 2 and 3 borrow"


def test_a_lender_24_levels_off_is_passed_over():
    fill, src, Cm = worked(2)
    y, x = 32, 43
    src[3, y, x] = np.clip(fill[2, y, x].astype(int) + [24, 0, 0], 0, 255)      # one pixel: no seed on frame 3
    info = {}
    out = bs.borrow(fill, src, Cm, ROWS, T, 3, info=info)
    assert not info["N"][3, y, x] and info["lender"][2, y, x] == 4 and np.array_equal(out[2, y, x], src[4, y, x])
    src[3, y, x, 0] = int(fill[2, y, x, 0]) + 23
    assert bs.borrow(fill, src, Cm, ROWS, T, 3, info=info) is not None and info["lender"][2, y, x] == 3


def test_a_lender_with_its_own_glyph_is_passed_over():
    fill, src, Cm = worked(3)
    info = {}
    bs.borrow(fill, src, Cm, ROWS, T, 3, info=info)
    assert (info["lender"][1, 30:35, 40:47] == 3).all(), "frames 0 and 2 show the block there: frame 3, two away, lends"
    assert info["refused_near"] > 0 and info["N"][0, 32, 43] and info["N"][2, 32, 43]


def test_an_uninpainted_frame_lends_though_deflicker_closes_the_pair():
    from tests import _deflicker_statement as ds

    fill, src, Cm = worked(4)
    src[3, 30:35, 90:97] = src[2, 30:35, 90:97]                                   # frame 3 carries no glyph and is not inpainted
    fill[3] = src[3]
    info, dinfo = {}, {}
    out = bs.borrow(fill, src, Cm, ROWS, T, 1, info=info)
    ds.deflicker(fill, src, Cm, ROWS, 1, info=dinfo)
    assert dinfo["a"][(2, 1)] == 0 and info["b"][(2, 1)] == 16
    assert not info["Z"][3].any() and np.array_equal(out[3], fill[3]), "it borrows nothing"
    assert (info["lender"][2][info["borrowers"][2]] == 3).all() and (info["lender"][4][info["borrowers"][4]] == 3).all(), "and lends everywhere"


def test_properties():
    fill, src, Cm = worked(5)
    keep = src.copy()
    assert np.array_equal(bs.borrow(src.copy(), src, Cm, ROWS, T, 3), src), "fill == src is a fixed point"
    assert np.array_equal(src, keep), "src is never written"
    assert np.array_equal(bs.borrow(fill, src, Cm, ROWS, T, 0), fill) and np.array_equal(bs.borrow(fill[:1], src[:1], Cm, ROWS, T, 3), fill[:1])
    # a cut between frames 2 and 3: the two sides equal the statement run on each alone
    cut_src, cut_fill = src.copy(), fill.copy()
    cut_src[3:] = 255 - cut_src[3:]
    cut_fill[3:] = 255 - cut_fill[3:]
    info = {}
    out = bs.borrow(cut_fill, cut_src, Cm, ROWS, T, 3, info=info)
    assert all(v == 0 for (t, k), v in info["b"].items() if t < 3 <= t + k)
    assert np.array_equal(out[:3], bs.borrow(cut_fill[:3], cut_src[:3], Cm, ROWS, T, 3))
    assert np.array_equal(out[3:], bs.borrow(cut_fill[3:], cut_src[3:], Cm, ROWS, T, 3))
    # a batch and its halves differ only within B frames of the split; the window is one-sided at the ends
    whole = bs.borrow(fill, src, Cm, ROWS, T, 1)
    halves = np.concatenate([bs.borrow(fill[:3], src[:3], Cm, ROWS, T, 1), bs.borrow(fill[3:], src[3:], Cm, ROWS, T, 1)])
    differ = [t for t in range(6) if not np.array_equal(whole[t], halves[t])]
    assert differ == [2, 3]


def test_strip_rows_state_the_rows_of_the_full_frame():
    fill, src, Cm = worked(6)
    rows = (15, 55)
    full = bs.borrow(fill, src, Cm, rows, T, 3)
    strip = bs.borrow(fill[:, 15:55], src[:, 15:55], Cm, rows, T, 3, y0=15)
    assert np.array_equal(strip, full[:, 15:55]) and not np.array_equal(full, fill)


# ---- options and ranks ------------------------------------------------------------------------------------------------------------------
FOUR = ("VSR_SEAM_FEATHER", "VSR_REGRAIN", "VSR_DEFLICKER", "VSR_TONE_MATCH")


def test_option_parsing(monkeypatch):
    from vsr_amd.backend import main as m
    from vsr_amd.backend.tools import borrow as bw
    from vsr_amd.backend.tools.args_handler import parse_args

    assert bw.MAX_BORROW == bs.MAX_BORROW and bw.ENV == "VSR_BORROW"
    assert bw.borrow_option(env={}) == 0 and bw.borrow_option(env={"VSR_BORROW": ""}) == 0
    assert bw.borrow_option(env={"VSR_BORROW": "3"}) == 3 and bw.borrow_option(8, env={}) == 8
    assert bw.borrow_option(2, env={"VSR_BORROW": "5"}) == 2, "an argument wins over the environment"
    for bad in ("-1", "9", "x", "1.5"):
        with pytest.raises(ValueError, match="borrow"):
            bw.borrow_option(env={"VSR_BORROW": bad})
    for bad in (-1, 9, 1.5):
        with pytest.raises(ValueError, match="borrow"):
            bw.borrow_option(bad)
    assert parse_args(["-i", "x.y4m"]).borrow is None
    assert parse_args(["-i", "x.y4m", "--glyph-key", "12", "--borrow", "2"]).borrow == 2
    for bad in (["--borrow", "2"], ["--glyph-key", "12", "--borrow", "9"], ["--glyph-key", "12", "--borrow", "-1"]):
        with pytest.raises(SystemExit):
            parse_args(["-i", "x.y4m"] + bad)
    assert ("borrow", "VSR_BORROW", str) in m.FLAG_ENV


def test_flag_sets_the_environment_variable(monkeypatch):
    import os

    from vsr_amd.backend import main as m

    seen = {}

    class Stop(Exception):
        pass

    def fake_remover(path):
        seen["env"] = os.environ.get("VSR_BORROW")
        raise Stop

    monkeypatch.setenv("VSR_BORROW", "0")
    monkeypatch.setenv("VSR_GLYPH_KEY", "0")
    monkeypatch.setattr(m, "SubtitleRemover", fake_remover)
    with pytest.raises(Stop):
        m.main(["-i", "x.y4m", "--glyph-key", "12", "--borrow", "2"])
    assert seen["env"] == "2"


def test_options_and_refusals_still_name_four(monkeypatch):
    from vsr_amd.backend.tools import seam_feather as sf

    for name, value in zip(FOUR + ("VSR_GLYPH_KEY", "VSR_BORROW"), ("3", "150", "2", "60", "12", "2")):
        monkeypatch.setenv(name, value)
    assert sf.options() == (3, 150, 2, 60) and sf.refuse_ranks_all(None) == (3, 150, 2, 60)
    monkeypatch.setenv("VSR_GLYPH_KEY", "0")
    assert sf.options() == (3, 150, 2, 60)
    with pytest.raises(ValueError, match="--borrow .* --glyph-key"):
        sf.refuse_ranks_all(None)
    monkeypatch.setenv("VSR_GLYPH_KEY", "12")
    monkeypatch.setenv("VSR_BORROW", "9")
    with pytest.raises(ValueError, match="borrow"):
        sf.refuse_ranks_all(None)


class FakeDist:
    @staticmethod
    def get_world_size():
        return 2

    @staticmethod
    def get_rank():
        return 0


def others_off(monkeypatch):
    for name in FOUR + ("VSR_GLYPH_HOLD",):
        monkeypatch.delenv(name, raising=False)


@pytest.mark.parametrize("entry", ["run", "video_inpaint", "propainter_mode"])
def test_refusals_before_a_frame_is_read(monkeypatch, entry):
    from vsr_amd.backend import main as m
    from vsr_amd.backend.tools import borrow as bw
    from vsr_amd.backend.tools.subtitle_detect import SubtitleDetect
    from vsr_amd.backend.tools.video_io import ArrayVideo

    class Source(ArrayVideo):
        def read(self):
            raise AssertionError("a frame was read")

    def no_work(*a, **kw):
        raise AssertionError("work was started")

    sr = m.SubtitleRemover(Source(np.zeros((4, 48, 64, 3), np.uint8)))
    monkeypatch.setattr(SubtitleDetect, "find_subtitle_frame_no", no_work)
    monkeypatch.setattr(m, "STTNAutoInpaint", no_work)
    call = {"run": sr.run, "video_inpaint": lambda: sr.video_inpaint(None, no_work, text_detector=no_work),
            "propainter_mode": lambda: sr.propainter_mode(None, propainter_inpaint=no_work, text_detector=no_work)}[entry]
    others_off(monkeypatch)
    monkeypatch.setenv("VSR_BORROW", "2")
    monkeypatch.setenv("VSR_GLYPH_KEY", "0")
    with pytest.raises(ValueError, match="--borrow .* --glyph-key"):
        call()
    monkeypatch.setenv("VSR_GLYPH_KEY", "12")
    monkeypatch.setenv("VSR_BORROW", "9")
    with pytest.raises(ValueError, match="borrow"):
        call()
    monkeypatch.setenv("VSR_BORROW", "2")
    monkeypatch.setattr(sr, "_distributed", lambda: FakeDist)
    with pytest.raises(RuntimeError, match="one process"):
        call()
    # the pass's own refusal, with a stand-in for the ranks
    with pytest.raises(RuntimeError, match="--borrow .* one process"):
        bw.refuse_ranks(FakeDist, 2, 12)
    assert bw.refuse_ranks(FakeDist, 0, 0) == 0 and bw.refuse_ranks(None, 2, 12) == 2


def test_sttn_auto_refuses_before_the_source_is_opened(monkeypatch):
    from vsr_amd.backend.inpaint import sttn_auto_inpaint as sa

    def no_work(*a, **kw):
        raise AssertionError("the source was opened")

    monkeypatch.setattr(sa, "open_video", no_work)
    auto = object.__new__(sa.STTNAutoInpaint)
    auto.context = auto.scene_split = auto.lookahead = None
    auto.clip_gap = 50
    others_off(monkeypatch)
    monkeypatch.setenv("VSR_BORROW", "2")
    monkeypatch.setenv("VSR_GLYPH_KEY", "0")
    with pytest.raises(ValueError, match="--borrow .* --glyph-key"):
        auto._run(None, None, None, None)
    monkeypatch.setenv("VSR_GLYPH_KEY", "12")
    with pytest.raises(RuntimeError, match="one process"):
        auto._run(FakeDist, None, None, None)
    monkeypatch.setenv("VSR_BORROW", "x")
    with pytest.raises(ValueError, match="borrow"):
        auto._run(None, None, None, None)


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
    from vsr_amd.backend.tools import borrow, deflicker, glyph_key, regrain, seam_feather, tone_match

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
    return log


@pytest.mark.parametrize("form", ["device tensor", "list, device body", "list, host body"])
def test_a_plugin_call_runs_the_six_passes_in_order(monkeypatch, recorded, form):
    import torch

    from vsr_amd.backend.tools import seam_feather

    Hh, Ww = 24, 40
    mask = np.zeros((Hh, Ww), np.uint8)
    mask[10:16, 5:30] = 255
    frames = [np.full((Hh, Ww, 3), i, np.uint8) for i in range(3)]
    plugin = Plugin(recorded, accepts_device_frames=form != "list, host body")
    given = torch.from_numpy(np.stack(frames)) if form == "device tensor" else frames

    def call(these=given):
        del recorded[:]
        seam_feather.plugin_call(plugin, plugin.body, these, mask, "cpu")
        return list(recorded)

    for name in FOUR + ("VSR_GLYPH_KEY", "VSR_BORROW"):
        monkeypatch.delenv(name, raising=False)
    assert call() == ["body"]
    monkeypatch.setenv("VSR_BORROW", "2")
    assert call() == ["body"], "without a key the pass does not run (the entry points refuse the pair)"
    monkeypatch.setenv("VSR_GLYPH_KEY", "12")
    key = ("key", ("mask", 6 * 25), 12, 0)
    lend = ("borrow", ("sets", (0, Hh)), ("mask", 6 * 25), 12, 2, 0)
    assert call() == ["body", lend, key]
    assert call(given[:1]) == ["body", key], "a call of fewer than two frames reads B as 0"
    monkeypatch.setenv("VSR_BORROW", "0")
    assert call() == ["body", key], "B = 0: the calls of before"
    monkeypatch.setenv("VSR_BORROW", "2")
    monkeypatch.setenv("VSR_SEAM_FEATHER", "4")
    monkeypatch.setenv("VSR_REGRAIN", "100")
    monkeypatch.setenv("VSR_DEFLICKER", "2")
    monkeypatch.setenv("VSR_TONE_MATCH", "80")
    assert call() == ["body", ("tone", ("bands", (0, Hh)), 80, 0), ("deflicker", ("sets", (0, Hh)), 2, 0),
                      ("regrain", ("sets", (0, Hh)), 100, 0), lend, key, ("feather", 4)]


def test_strip_rows_reach_the_pass_as_picture_rows(monkeypatch, recorded):
    import torch

    from vsr_amd.backend.inpaint import sttn_auto_inpaint as sa
    from vsr_amd.backend.tools import seam_feather

    cm = np.zeros((48, 40), np.uint8)
    cm[20:30, 4:30] = 255
    strip = torch.zeros((2, 22, 40, 3), dtype=torch.uint8)
    seam_feather.device_call(strip, cm, lambda t: recorded.append("body"), 0, rows=(14, 36), sample_rows=(14, 36), key=55, borrow=3)
    assert recorded == ["body", ("borrow", ("sets", (14, 36)), ("mask", 260), 55, 3, 14), ("key", ("mask", 260), 55, 14)]

    class Engine:
        def auto_chunk(self, frames, mask, areas, **kw):
            recorded.append("body")

    plugin = object.__new__(sa.STTNInpaint)
    plugin.engine = Engine()
    for name in FOUR:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("VSR_GLYPH_KEY", "12")
    monkeypatch.setenv("VSR_BORROW", "2")
    del recorded[:]
    plugin.auto_chunk(strip, None, [(6, 16, 0, 40)], cmask=cm, rows=(14, 36))
    assert recorded == ["body", ("borrow", ("sets", (20, 30)), ("mask", 260), 12, 2, 14), ("key", ("mask", 260), 12, 14)]


@pytest.mark.parametrize("form", ["list, device body", "list, host body"])
def test_context_and_lookahead_frames_take_no_part(monkeypatch, recorded, form):
    """the pass sees the n frames of the call and their clone; the context frames in front and the look-ahead frames behind reach the
    body alone"""
    from vsr_amd.backend.tools import borrow, seam_feather

    seen = []
    monkeypatch.setattr(borrow, "apply", lambda frames, src, s, m, t, b, y0=0: seen.append((tuple(frames.shape), tuple(src.shape), b)))
    for name in FOUR:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("VSR_GLYPH_KEY", "12")
    monkeypatch.setenv("VSR_BORROW", "2")
    Hh, Ww = 24, 40
    mask = np.zeros((Hh, Ww), np.uint8)
    mask[10:16, 5:30] = 255
    frames = [np.full((Hh, Ww, 3), i, np.uint8) for i in range(3)]
    context = [np.full((Hh, Ww, 3), 100 + i, np.uint8) for i in range(2)]
    ahead = [np.full((Hh, Ww, 3), 200, np.uint8)]
    plugin = Plugin(recorded, accepts_device_frames=form == "list, device body")
    got = {}

    def body(given, m, **kw):
        got.update(n=len(given), context=len(kw["context"]), lookahead=len(kw["lookahead"]))
        return plugin.body(given, m)

    out = seam_feather.plugin_call(plugin, body, frames, mask, "cpu", context=context, lookahead=ahead)
    assert got == dict(n=3, context=2, lookahead=1) and len(out) == 3
    assert seen == [((3, Hh, Ww, 3), (3, Hh, Ww, 3), 2)], "the three frames of the call, and nothing of its context"


# ---- the entry points without a device ------------------------------------------------------------------------------------------------
def test_argument_errors_then_no_gpu(built_lib):
    lib = built_lib.lib
    buf = (C.c_uint8 * 4096)()
    words = (C.c_uint64 * 512)()
    p, q = C.cast(buf, C.c_void_p), C.cast(words, C.c_void_p)
    size = 8 * 8 * 3
    ok = dict(frames=p, fs=size, src=p, ss=size, cm=p, counts=q, stats=q, pairs=q, n=2, H=8, W=8, y0=0, rows=8, c0=2, c1=6, T=T, B=2, work=q)

    def apply(**kw):
        a = dict(ok, **kw)
        return lib.vsr_borrow_apply(a["frames"], a["fs"], a["src"], a["ss"], a["cm"], a["counts"], a["stats"], a["pairs"], a["n"], a["H"],
                                    a["W"], a["y0"], a["rows"], a["c0"], a["c1"], a["T"], a["B"], a["work"], None)

    for kw in (dict(frames=None), dict(counts=None), dict(pairs=None), dict(H=0), dict(n=-1), dict(fs=size - 1), dict(rows=9), dict(c1=9),
               dict(H=32768, W=32768, rows=1), dict(T=0), dict(T=129), dict(B=0), dict(B=9)):
        assert apply(**kw) == built_lib.VSR_ERR_ARG, kw
        assert "borrow" in built_lib.last_error(), kw
    assert lib.vsr_borrow_workspace_bytes(0, 8, 1) == built_lib.VSR_ERR_ARG and lib.vsr_borrow_workspace_bytes(8, 8, -1) == built_lib.VSR_ERR_ARG
    assert lib.vsr_borrow_workspace_bytes(9, 65, 3) == 2 * 3 * 9 * 2 * 8
    assert apply(n=1) == 0 and apply(c0=3, c1=3) == 0, "nothing to do is success without a launch"
    if lib.vsr_device_count() <= 0:
        assert apply() == built_lib.VSR_ERR_NOGPU
