"""--glyph-key without a GPU: the statement (tests/_key_statement.py) does what it is for on synthetic pictures, its bit-parallel form
is its brute-force form, the option is parsed in one place, several ranks are refused before any frame is read, and a plugin call runs
its five passes in the stated order."""
import numpy as np
import pytest

from tests import _key_statement as ks

T = 12


def test_constants():
    assert ks.G == 4 and ks.R == 4 and ks.MAX_KEY == 128 and ks.A_MAX == 2295
    assert 9 * ks.MAX_KEY <= ks.A_MAX, "the largest threshold can be reached"
    assert ks.workspace_bytes(1080, 1920, 50) == 50 * 1080 * 30 * 8 and ks.workspace_bytes(9, 65, 1) == 9 * 2 * 8


@pytest.mark.parametrize("W", [63, 64, 65, 130, 8])
def test_the_bit_parallel_distance_is_the_brute_force_distance(W):
    rng = np.random.default_rng(W)
    for h, density in ((1, 0.1), (5, 0.02), (7, 0.01), (20, 0.004), (33, 0.0015), (12, 0.0)):
        Z = rng.random((3, h, W)) < density
        if density:
            Z[0, 0, 0] = Z[0, -1, -1] = Z[1, 0, -1] = Z[1, -1, 0] = True        # the corners
            if W > 64:
                Z[2, h // 2, 63] = True                                      # either side of a word boundary, one at a time
                Z[2, :, 64] = False
                Z[1, h // 2, 64] = True
                Z[1, h // 2, 63] = False
        words = ks.pack_words(Z)
        assert words.shape == (3, h, -(-W // 64)) and np.array_equal(ks.unpack_words(words, W), Z)
        e = ks.distance(Z)
        assert np.array_equal(ks.distance_words(words, W), e), (h, W, density)
        assert (e[Z] == 0).all() and (e[~Z] > 0).all() and e.max() <= ks.G + ks.R
        if not density:
            assert (e == ks.G + ks.R).all(), "the frame border is no seed"


def test_dilation_carries_across_words():
    Z = np.zeros((1, 1, 200), bool)
    Z[0, 0, 64] = Z[0, 0, 127] = True
    for k in range(ks.G + ks.R):
        got = ks.unpack_words(ks.dilate_words(ks.pack_words(Z), k), 200)[0, 0]
        want = np.zeros(200, bool)
        want[64 - k:64 + k + 1] = want[127 - k:127 + k + 1] = True
        assert np.array_equal(got, want), k


def flat(n, H, W, value=100):
    return np.full((n, H, W, 3), value, np.uint8)


def test_the_threshold_is_met_at_nine_t():
    """one pixel off by 9 T - 1 in one channel: A = 9 T - 1 in its 3 x 3 neighbourhood, no seed; by 9 T: nine seeds"""
    H, W = 20, 30
    C = np.full((H, W), 255, np.uint8)
    for t in (1, 12, 28):
        src = flat(1, H, W, 0)
        fill = src.copy()
        fill[0, 9, 14, 1] = 9 * t - 1
        assert ks.box_sum(ks.difference(fill, src, C)).max() == 9 * t - 1 and not ks.seeds(fill, src, C, t).any()
        assert np.array_equal(ks.key(fill, src, C, t), src), "no seed: the source everywhere"
        fill[0, 9, 14, 1] = 9 * t
        Z = ks.seeds(fill, src, C, t)
        assert Z.sum() == 9 and Z[0, 8:11, 13:16].all()
        out = ks.key(fill, src, C, t)
        assert out[0, 9, 14, 1] == 9 * t, "within G of a seed: the fill"
    # the stated examples: a one-pixel stroke 100 levels off is a seed at T = 12 (3 x 100 >= 108), two grains of 18 are not
    src = flat(1, H, W)
    fill = src.copy()
    fill[0, 5:15, 10] -= 100
    assert ks.seeds(fill, src, C, T)[0, 6:14, 9:12].all()
    fill = src.copy()
    fill[0, 5, 10, 0] += 18
    fill[0, 6, 11, 2] -= 18
    assert not ks.seeds(fill, src, C, T).any()


def test_the_weight():
    e = np.arange(0, 12)
    assert ks.weight(e).tolist() == [4, 4, 4, 4, 4, 3, 2, 1, 0, 0, 0, 0]
    # the mix at every weight: src and fill 90 levels apart (A = 810 < 900 = 9 T), seeds at the left edge
    H, W = 5, 40
    C = np.full((H, W), 1, np.uint8)
    src, fill = flat(1, H, W, 0), flat(1, H, W, 0)
    fill[0, :, :, 0], src[0, :, :, 1] = 90, 90
    fill[0, :, 0, 2] = 255                                                # column 0, and column 1, whose sum holds column 0
    info = []
    out = ks.key(fill, src, C, 100, info=info)
    Z, a = info[0]
    assert Z[0, 1:4, :2].all() and not Z[0, :, 2:].any()
    assert a[0, 2, 1:11].tolist() == [4, 4, 4, 4, 4, 3, 2, 1, 0, 0]
    assert out[0, 2, 6:9, 0].tolist() == [68, 45, 23] and out[0, 2, 6:9, 1].tolist() == [23, 45, 68], "(a f + (R - a) s + R / 2) // R"
    assert np.array_equal(out[0, :, 9:], src[0, :, 9:]) and np.array_equal(out[0, :, :6], fill[0, :, :6])


def test_a_fill_that_equals_the_source_comes_back():
    rng = np.random.default_rng(1)
    src = rng.integers(0, 256, (2, 30, 70, 3), dtype=np.uint8)
    C = np.zeros((30, 70), np.uint8)
    C[10:25, 3:69] = 255
    for t in (1, 12, 128):
        assert np.array_equal(ks.key(src.copy(), src, C, t), src)


# ---- the synthetic clip ---------------------------------------------------------------------------------------------------------------
H, W, BOX, BLOCK = 64, 150, (20, 56, 10, 140), (34, 39, 70, 77)             # rows and columns: the mask, the 5 x 7 block


def synthetic(seed):
    """src: a ramp with noise of sigma 2; fill: the same ramp with another draw of the noise inside the box mask, src outside it;
    frames 0 and 2 carry a block of +120 in the source only"""
    rng = np.random.default_rng(seed)
    C = np.zeros((H, W), np.uint8)
    C[BOX[0]:BOX[1], BOX[2]:BOX[3]] = 255
    y, x = np.mgrid[0:H, 0:W]
    ramp = (40 + 0.5 * x + 0.25 * y)[None, :, :, None] + np.zeros((3, 1, 1, 3))
    src = np.rint(ramp + rng.normal(0, 2, ramp.shape))
    src[0::2, BLOCK[0]:BLOCK[1], BLOCK[2]:BLOCK[3]] += 120
    src = np.clip(src, 0, 255).astype(np.uint8)
    other = np.clip(np.rint(ramp + rng.normal(0, 2, ramp.shape)), 0, 255).astype(np.uint8)
    fill = src.copy()
    fill[:, C != 0] = other[:, C != 0]
    return fill, src, C


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_block_is_filled_and_the_rest_is_the_source(seed):
    fill, src, C = synthetic(seed)
    info = []
    out = ks.key(fill, src, C, T, info=info)
    Z, a = info[0]
    hull = np.zeros((H, W), bool)
    hull[BLOCK[0] - 1:BLOCK[1] + 1, BLOCK[2] - 1:BLOCK[3] + 1] = True
    assert not Z[1].any() and not Z[0][~hull].any() and not Z[2][~hull].any(), "the noise alone makes no seed"
    quiet = ks.box_sum(ks.difference(fill, src, C))[1].max()
    print("seed", seed, "largest 3 x 3 sum of the noise:", int(quiet), "of", 9 * T)
    assert Z[0][BLOCK[0]:BLOCK[1], BLOCK[2]:BLOCK[3]].all() and Z[2][BLOCK[0]:BLOCK[1], BLOCK[2]:BLOCK[3]].all()
    assert np.array_equal(out[1], src[1]), "the frame without a block is its source"
    reach = ks.G + ks.R
    far = np.ones((H, W), bool)
    far[BLOCK[0] - 1 - reach:BLOCK[1] + 1 + reach, BLOCK[2] - 1 - reach:BLOCK[3] + 1 + reach] = False
    inside = C != 0
    for f in (0, 2):
        assert np.array_equal(out[f][far & inside], src[f][far & inside]), "farther than G + R from the block's hull: the source"
        near = ks.distance(Z[f:f + 1])[0] <= ks.G
        assert near[BLOCK[0] - 4:BLOCK[1] + 4, BLOCK[2] - 4:BLOCK[3] + 4].all()
        assert np.array_equal(out[f][near & inside], fill[f][near & inside]), "within G of a seed: the fill"
        assert (out[f] != src[f]).any() and (out[f] != fill[f]).any()
    assert np.array_equal(out[:, ~inside], fill[:, ~inside])


def test_outside_the_mask_every_byte_is_the_fills():
    rng = np.random.default_rng(5)
    src = rng.integers(0, 256, (2, 40, 90, 3), dtype=np.uint8)
    fill = rng.integers(0, 256, (2, 40, 90, 3), dtype=np.uint8)                       # the body may write anywhere
    C = np.zeros((40, 90), np.uint8)
    C[12:30, 20:80] = 7
    fill[1][C != 0] = src[1][C != 0]                                                  # a frame the call did not inpaint
    out = ks.key(fill, src, C, T)
    assert np.array_equal(out[:, C == 0], fill[:, C == 0])
    assert np.array_equal(out[1], fill[1]) and np.array_equal(out[0][C != 0], fill[0][C != 0]), "noise everywhere: seeds everywhere"


@pytest.mark.parametrize("rows", [(20, 56), (15, 60), (5, 38)])
def test_strip_rows_state_the_rows_of_the_full_frame(rows):
    """whenever the strip holds the rows of C (a seed on the row above C has a seed under it that is nearer to every pixel of C); and
    a strip that cuts C states its own rows, the rows beyond it counting 0"""
    fill, src, C = synthetic(3)
    full = ks.key(fill, src, C, T)
    strip = ks.key(fill[:, rows[0]:rows[1]], src[:, rows[0]:rows[1]], C, T, y0=rows[0])
    if rows[0] <= BOX[0] and rows[1] >= BOX[1]:
        assert np.array_equal(strip, full[:, rows[0]:rows[1]])
    else:
        cut = np.zeros_like(C)
        cut[rows[0]:rows[1]] = C[rows[0]:rows[1]]
        assert np.array_equal(strip, ks.key(fill, src, cut, T)[:, rows[0]:rows[1]])
    assert not np.array_equal(full, fill)


# ---- options and ranks ------------------------------------------------------------------------------------------------------------------
def test_option_parsing(monkeypatch):
    from vsr_amd.backend.tools import glyph_key as gk
    from vsr_amd.backend.tools.args_handler import parse_args

    assert gk.MAX_KEY == ks.MAX_KEY
    assert gk.key_option(env={}) == 0 and gk.key_option(env={"VSR_GLYPH_KEY": ""}) == 0
    assert gk.key_option(env={"VSR_GLYPH_KEY": "37"}) == 37 and gk.key_option(128, env={}) == 128
    assert gk.key_option(3, env={"VSR_GLYPH_KEY": "5"}) == 3, "an argument wins over the environment"
    for bad in ("-1", "129", "x", "1.5"):
        with pytest.raises(ValueError, match="glyph key"):
            gk.key_option(env={"VSR_GLYPH_KEY": bad})
    for bad in (-1, 129, 1.5):
        with pytest.raises(ValueError, match="glyph key"):
            gk.key_option(bad)
    monkeypatch.setenv("VSR_GLYPH_KEY", "4")
    assert gk.key_option() == 4
    assert parse_args(["-i", "x.y4m"]).glyph_key is None
    assert parse_args(["-i", "x.y4m", "--glyph-key", "12"]).glyph_key == 12
    for bad in ("129", "-1"):
        with pytest.raises(SystemExit):
            parse_args(["-i", "x.y4m", "--glyph-key", bad])


FOUR = ("VSR_SEAM_FEATHER", "VSR_REGRAIN", "VSR_DEFLICKER", "VSR_TONE_MATCH")


def test_options_and_refusals_still_name_four(monkeypatch):
    from vsr_amd.backend.tools import seam_feather as sf

    for name, value in zip(FOUR + ("VSR_GLYPH_KEY",), ("3", "150", "2", "60", "12")):
        monkeypatch.setenv(name, value)
    assert sf.options() == (3, 150, 2, 60) and sf.refuse_ranks_all(None) == (3, 150, 2, 60)
    for name in FOUR:
        monkeypatch.delenv(name)
    assert sf.options() == (0, 0, 0, 0) and sf.refuse_ranks_all(None) == (0, 0, 0, 0)
    monkeypatch.setenv("VSR_GLYPH_KEY", "129")
    assert sf.options() == (0, 0, 0, 0)
    with pytest.raises(ValueError, match="glyph key"):
        sf.refuse_ranks_all(None)


def test_flag_sets_the_environment_variable(monkeypatch):
    from vsr_amd.backend import main as m

    seen = {}

    class Stop(Exception):
        pass

    def fake_remover(path):
        import os

        seen["env"] = os.environ.get("VSR_GLYPH_KEY")
        raise Stop

    monkeypatch.setenv("VSR_GLYPH_KEY", "0")
    monkeypatch.setattr(m, "SubtitleRemover", fake_remover)
    with pytest.raises(Stop):
        m.main(["-i", "x.y4m", "--glyph-key", "12"])
    assert seen["env"] == "12"


class FakeDist:
    @staticmethod
    def get_world_size():
        return 2

    @staticmethod
    def get_rank():
        return 0


def others_off(monkeypatch):
    for name in FOUR:
        monkeypatch.delenv(name, raising=False)


@pytest.mark.parametrize("entry", ["run", "video_inpaint", "propainter_mode"])
def test_several_ranks_are_refused_before_a_frame_is_read(monkeypatch, entry):
    from vsr_amd.backend import main as m
    from vsr_amd.backend.tools import glyph_key as gk
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
    monkeypatch.setenv("VSR_GLYPH_KEY", "12")
    with pytest.raises(RuntimeError, match="--glyph-key .* one process"):
        call()
    monkeypatch.setenv("VSR_GLYPH_KEY", "129")
    with pytest.raises(ValueError, match="glyph key"):
        call()
    # off, or one rank: nothing is refused
    assert gk.refuse_ranks(FakeDist, 0) == 0 and gk.refuse_ranks(None, 12) == 12


def test_sttn_auto_refuses_several_ranks_before_the_source_is_opened(monkeypatch):
    from vsr_amd.backend.inpaint import sttn_auto_inpaint as sa

    def no_work(*a, **kw):
        raise AssertionError("the source was opened")

    monkeypatch.setattr(sa, "open_video", no_work)
    auto = object.__new__(sa.STTNAutoInpaint)
    auto.context = auto.scene_split = auto.lookahead = None
    auto.clip_gap = 50
    others_off(monkeypatch)
    monkeypatch.setenv("VSR_GLYPH_KEY", "12")
    with pytest.raises(RuntimeError, match="--glyph-key .* one process"):
        auto._run(FakeDist, None, None, None)
    monkeypatch.setenv("VSR_GLYPH_KEY", "x")
    with pytest.raises(ValueError, match="glyph key"):
        auto._run(None, None, None, None)


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
    """the five passes and their per-mask caches replaced by stand-ins that write down their names"""
    from vsr_amd.backend.tools import deflicker, glyph_key, regrain, seam_feather, tone_match

    log = []
    monkeypatch.setattr(tone_match, "sets", lambda cm, rows, device: ("bands", tuple(rows)))
    monkeypatch.setattr(regrain, "sets", lambda cm, rows, device: ("sets", tuple(rows)))
    monkeypatch.setattr(glyph_key, "mask", lambda cm, device: ("mask", int((cm != 0).sum())))
    monkeypatch.setattr(seam_feather, "alpha", lambda cm, feather, device: np.zeros(cm.shape, np.uint8))
    monkeypatch.setattr(tone_match, "apply", lambda frames, src, s, percent, y0=0: log.append(("tone", s, percent, y0)))
    monkeypatch.setattr(deflicker, "apply", lambda frames, src, s, radius, y0=0: log.append(("deflicker", s, radius, y0)))
    monkeypatch.setattr(regrain, "apply", lambda frames, src, s, percent, y0=0: log.append(("regrain", s, percent, y0)))
    monkeypatch.setattr(glyph_key, "apply", lambda frames, src, m, t, y0=0: log.append(("key", m, t, y0)))
    monkeypatch.setattr(seam_feather, "composite", lambda frames, src, d, feather: log.append(("feather", feather)))
    return log


@pytest.mark.parametrize("form", ["device tensor", "list, device body", "list, host body"])
def test_a_plugin_call_runs_the_five_passes_in_order(monkeypatch, recorded, form):
    import torch

    from vsr_amd.backend.tools import seam_feather

    Hh, Ww = 24, 40
    mask = np.zeros((Hh, Ww), np.uint8)
    mask[10:16, 5:30] = 255
    frames = [np.full((Hh, Ww, 3), i, np.uint8) for i in range(3)]
    plugin = Plugin(recorded, accepts_device_frames=form != "list, host body")
    given = torch.from_numpy(np.stack(frames)) if form == "device tensor" else frames

    def call():
        del recorded[:]
        seam_feather.plugin_call(plugin, plugin.body, given, mask, "cpu")
        return list(recorded)

    for name in FOUR + ("VSR_GLYPH_KEY",):
        monkeypatch.delenv(name, raising=False)
    assert call() == ["body"], "every option off: the body alone"
    monkeypatch.setenv("VSR_GLYPH_KEY", "0")
    assert call() == ["body"], "T = 0 is off"
    monkeypatch.setenv("VSR_GLYPH_KEY", "12")
    key = ("key", ("mask", 6 * 25), 12, 0)
    assert call() == ["body", key]
    monkeypatch.setenv("VSR_SEAM_FEATHER", "4")
    monkeypatch.setenv("VSR_REGRAIN", "100")
    monkeypatch.setenv("VSR_DEFLICKER", "2")
    monkeypatch.setenv("VSR_TONE_MATCH", "80")
    assert call() == ["body", ("tone", ("bands", (0, Hh)), 80, 0), ("deflicker", ("sets", (0, Hh)), 2, 0),
                      ("regrain", ("sets", (0, Hh)), 100, 0), key, ("feather", 4)]
    monkeypatch.setenv("VSR_GLYPH_KEY", "0")
    assert call() == ["body", ("tone", ("bands", (0, Hh)), 80, 0), ("deflicker", ("sets", (0, Hh)), 2, 0),
                      ("regrain", ("sets", (0, Hh)), 100, 0), ("feather", 4)]
    # an empty composite mask: the body alone, whatever is on
    monkeypatch.setenv("VSR_GLYPH_KEY", "12")
    del recorded[:]
    seam_feather.plugin_call(plugin, plugin.body, given, np.zeros((Hh, Ww), np.uint8), "cpu")
    assert recorded == ["body"]


def test_one_frame_is_keyed_too(monkeypatch, recorded):
    """deflicker needs a neighbour; the key judges every frame by itself"""
    import torch

    from vsr_amd.backend.tools import seam_feather

    for name in FOUR:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("VSR_GLYPH_KEY", "12")
    monkeypatch.setenv("VSR_DEFLICKER", "2")
    mask = np.zeros((24, 40), np.uint8)
    mask[3, 3] = 1
    plugin = Plugin(recorded, accepts_device_frames=True)
    seam_feather.plugin_call(plugin, plugin.body, torch.zeros((1, 24, 40, 3), dtype=torch.uint8), mask, "cpu")
    assert recorded == ["body", ("key", ("mask", 1), 12, 0)]


def test_strip_rows_reach_the_pass_as_picture_rows(recorded):
    import torch

    from vsr_amd.backend.tools import seam_feather

    cm = np.zeros((48, 40), np.uint8)
    cm[20:30, 4:30] = 255
    strip = torch.zeros((2, 22, 40, 3), dtype=torch.uint8)
    seam_feather.device_call(strip, cm, lambda t: recorded.append("body"), 0, rows=(14, 36), sample_rows=(14, 36), key=55)
    assert recorded == ["body", ("key", ("mask", 260), 55, 14)]


def test_sttn_auto_hands_the_option_through(monkeypatch, recorded):
    """STTNInpaint.auto_chunk, where sttn-auto's loops end: the strip rows and T reach device_call"""
    import torch

    from vsr_amd.backend.inpaint import sttn_auto_inpaint as sa

    class Engine:
        def auto_chunk(self, frames, mask, areas, **kw):
            recorded.append("body")

    plugin = object.__new__(sa.STTNInpaint)
    plugin.engine = Engine()
    for name in FOUR:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("VSR_GLYPH_KEY", "12")
    cm = np.zeros((48, 40), np.uint8)
    cm[20:30, 4:30] = 255
    strip = torch.zeros((2, 22, 40, 3), dtype=torch.uint8)
    plugin.auto_chunk(strip, None, [(6, 16, 0, 40)], cmask=cm, rows=(14, 36))
    assert recorded == ["body", ("key", ("mask", 260), 12, 14)]
