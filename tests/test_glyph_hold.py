"""--glyph-hold without a GPU: the statement (tests/_hold_statement.py) is the plain key wherever the definition says so, only ever
keeps more fill, steadies a glyph that hovers about T, reaches K frames and one pixel and no further; its bit-parallel form is its
boolean form; the option is parsed in one place; a bad K, K without T and several ranks are refused before a frame is read; and the
plugin call's chain calls glyph_key.apply exactly as it did."""
import inspect

import numpy as np
import pytest

from tests import _hold_statement as hs
from tests import _key_statement as ks

T = 12
FIVE = ("VSR_SEAM_FEATHER", "VSR_REGRAIN", "VSR_DEFLICKER", "VSR_TONE_MATCH", "VSR_GLYPH_KEY")


def test_constants():
    assert hs.MAX_HOLD == 8 and (hs.G, hs.R) == (ks.G, ks.R)
    assert [hs.low(t) for t in (1, 2, 3, 12, 127, 128)] == [1, 1, 2, 6, 64, 64]
    assert hs.workspace_bytes(1080, 1920, 50) == 3 * 50 * 1080 * 30 * 8


def random_clip(seed, n=5, H=30, W=70):
    """src: noise; fill: src off by up to 40 levels in a third of the pixels of a box mask, frame 1 not inpainted"""
    rng = np.random.default_rng(seed)
    src = rng.integers(40, 200, (n, H, W, 3), dtype=np.uint8)
    C = np.zeros((H, W), np.uint8)
    C[6:25, 3:66] = 255
    off = rng.integers(0, 41, (n, H, W, 1)) * (rng.random((n, H, W, 1)) < 0.3)
    fill = (src + off).astype(np.uint8)
    if n > 1:
        fill[1] = src[1]
    return fill, src, C


# ---- equality with the plain key, set relations ----------------------------------------------------------------------------------------
def test_k0_one_frame_and_t1_are_the_plain_key():
    fill, src, C = random_clip(0)
    for t in (1, 12, 16):
        assert np.array_equal(hs.hold(fill, src, C, t, 0), ks.key(fill, src, C, t)), "K = 0"
        assert np.array_equal(hs.seeds(fill, src, C, t, 0), ks.seeds(fill, src, C, t))
    for k in (1, 8):
        assert np.array_equal(hs.hold(fill[:1], src[:1], C, T, k), ks.key(fill[:1], src[:1], C, T)), "n = 1"
        assert np.array_equal(hs.hold(fill, src, C, 1, k), ks.key(fill, src, C, 1)), "T = 1: T_lo = T"
    assert not np.array_equal(hs.hold(fill, src, C, 16, 2), ks.key(fill, src, C, 16)), "(the clip is one the hold changes)"


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_hold_only_keeps_more_fill(seed):
    fill, src, C = random_clip(seed, n=6)
    for t in (8, 12, 16):
        S, Wk = hs.strong_weak(fill, src, C, t)
        assert np.array_equal(S, ks.seeds(fill, src, C, t)) and (Wk | ~S).all(), "S is the plain key's Z, and S <= Wk"
        before = S
        grew = False
        for k in range(hs.MAX_HOLD + 1):
            Z = hs.seeds(fill, src, C, t, k)
            assert (Z | ~before).all() and (Wk | ~Z).all(), "Z'(K - 1) <= Z'(K) <= Wk"
            grew |= bool((Z & ~before).any())
            before = Z
            a_plain, a_held = ks.weight(ks.distance(S)), ks.weight(ks.distance(Z))
            assert (a_held >= a_plain).all(), "no pixel gets less of the fill"
        assert not Z[1].any() and not Wk[1].any(), "the frame that was not inpainted has no seed"
        assert grew


# ---- the hovering glyph ----------------------------------------------------------------------------------------------------------------
H, W, BOX, BLOCK = 64, 150, (20, 56, 10, 140), (34, 39, 70, 77)             # rows and columns: the mask, the 5 x 7 block


def hovering(seed, n=6):
    """src: a ramp with noise; fill: src but for the block, 14 levels off on even frames and 10 on odd ones: about T = 12"""
    rng = np.random.default_rng(seed)
    C = np.zeros((H, W), np.uint8)
    C[BOX[0]:BOX[1], BOX[2]:BOX[3]] = 255
    y, x = np.mgrid[0:H, 0:W]
    ramp = (40 + 0.5 * x + 0.25 * y)[None, :, :, None] + np.zeros((n, 1, 1, 3))
    src = np.clip(np.rint(ramp + rng.normal(0, 2, ramp.shape)), 0, 255).astype(np.uint8)
    fill = src.copy()
    fill[0::2, BLOCK[0]:BLOCK[1], BLOCK[2]:BLOCK[3]] += 14
    fill[1::2, BLOCK[0]:BLOCK[1], BLOCK[2]:BLOCK[3]] += 10
    return fill, src, C


def test_a_glyph_that_hovers_about_t_is_held():
    fill, src, C = hovering(0)
    n = fill.shape[0]
    block = np.zeros((H, W), bool)
    block[BLOCK[0]:BLOCK[1], BLOCK[2]:BLOCK[3]] = True
    info = []
    plain = hs.hold(fill, src, C, T, 0, info=info)
    S, Wk, Z, a = info[0]
    assert np.array_equal(plain, ks.key(fill, src, C, T)) and np.array_equal(Z, S)
    for f in range(n):
        if f % 2:
            assert not S[f].any() and Wk[f][BLOCK[0] + 1:BLOCK[1] - 1, BLOCK[2] + 1:BLOCK[3] - 1].all()
            assert np.array_equal(plain[f], src[f]) and (a[f] == 0).all(), "K = 0: the odd frames are their source, the block included"
        else:
            assert S[f][BLOCK[0] + 1:BLOCK[1] - 1, BLOCK[2] + 1:BLOCK[3] - 1].all()
            assert np.array_equal(plain[f][block], fill[f][block])
    changes = lambda w: int((w[1:] != w[:-1]).sum())
    assert changes(a) > 0
    info = []
    out = hs.hold(fill, src, C, T, 1, info=info)
    S1, Wk1, Z1, a1 = info[0]
    reach = ks.G + ks.R
    far = np.ones((H, W), bool)
    far[BLOCK[0] - 1 - reach:BLOCK[1] + 1 + reach, BLOCK[2] - 1 - reach:BLOCK[3] + 1 + reach] = False
    inside = C != 0
    for f in range(n):
        assert Z1[f].any() and not Z1[f][~block].any()
        near = ks.distance(block[None])[0] <= ks.G
        assert np.array_equal(out[f][near & inside], fill[f][near & inside]), "K = 1: the fill within G of the block on every frame"
        assert (a1[f][block] == ks.R).all(), "and at full weight in the block"
        assert np.array_equal(out[f][far & inside], src[f][far & inside]) and (a1[f][far] == 0).all(), "farther than G + R: the source"
    assert np.array_equal(out[:, ~inside], fill[:, ~inside])
    assert changes(a1 > 0) < changes(a > 0), "the patch stops switching on and off"


# ---- the edge cases of the definition --------------------------------------------------------------------------------------------------
def test_weak_only_differences_change_nothing():
    rng = np.random.default_rng(4)
    src = rng.integers(0, 200, (4, 24, 40, 3), dtype=np.uint8)
    C = np.full((24, 40), 255, np.uint8)
    fill = src + rng.integers(6, 12, (4, 24, 40, 1)).astype(np.uint8)         # A in [54, 99] inside: weak everywhere, strong nowhere
    S, Wk = hs.strong_weak(fill, src, C, T)
    assert not S.any() and Wk[:, 1:-1, 1:-1].all()
    for k in (1, 8):
        assert not hs.seeds(fill, src, C, T, k).any()
        assert np.array_equal(hs.hold(fill, src, C, T, k), ks.key(fill, src, C, T))
    assert np.array_equal(hs.hold(fill, src, C, T, 8), src)


def test_an_untouched_frame_between_two_strong_ones_is_its_source():
    fill, src, C = hovering(2, n=3)
    fill[0::2, BLOCK[0]:BLOCK[1], BLOCK[2]:BLOCK[3]] += 100
    fill[1] = src[1]
    info = []
    out = hs.hold(fill, src, C, T, 2, info=info)
    S, Wk, Z, a = info[0]
    assert S[0].any() and S[2].any() and not Wk[1].any() and not Z[1].any() and np.array_equal(out[1], src[1])


def maps(n, h, w, strong=(), weak=()):
    S, Wk = np.zeros((n, h, w), bool), np.zeros((n, h, w), bool)
    for at in strong:
        S[at] = True
    for at in weak:
        Wk[at] = True
    return S, Wk | S


def test_the_reach_in_space_is_one_pixel():
    S, Wk = maps(2, 12, 12, strong=[(0, 5, 5)], weak=[(1, 6, 6), (1, 4, 4), (1, 5, 7), (1, 7, 5), (1, 5, 5), (0, 9, 9)])
    Z = hs.held(S, Wk, 1)
    assert Z[1, 6, 6] and Z[1, 4, 4] and Z[1, 5, 5], "a weak pixel at or one pixel off a neighbour frame's strong seed is held"
    assert not Z[1, 5, 7] and not Z[1, 7, 5], "two pixels off: not"
    assert Z[0, 5, 5] and not Z[0, 9, 9] and Z.sum() == 4
    # a frame's own strong seed holds nothing of its own weak pixels
    S, Wk = maps(2, 12, 12, strong=[(0, 5, 5)], weak=[(0, 5, 6)])
    assert hs.held(S, Wk, 8).sum() == 1


def test_the_reach_in_time_is_k_frames():
    n = 12
    S, Wk = maps(n, 4, 4, strong=[(5, 2, 2)], weak=[(f, 2, 2) for f in range(n)])
    for k in range(hs.MAX_HOLD + 1):
        Z = hs.held(S, Wk, k)
        assert [f for f in range(n) if Z[f, 2, 2]] == list(range(max(5 - k, 0), min(5 + k, n - 1) + 1)), k
        assert Z.sum() == len(range(max(5 - k, 0), min(5 + k, n - 1) + 1))


def test_one_sided_windows_and_a_window_longer_than_the_call():
    S, Wk = maps(3, 4, 4, strong=[(0, 1, 1), (2, 2, 2)], weak=[(f, y, y) for f in range(3) for y in (1, 2)])
    Z = hs.held(S, Wk, 1)
    assert Z[0, 1, 1] and not Z[0, 2, 2], "frame 0 looks ahead only, and one frame"
    assert Z[1, 1, 1] and Z[1, 2, 2] and Z[2, 2, 2] and not Z[2, 1, 1]
    for k in (2, 3, 8):
        assert hs.held(S, Wk, k)[:, [1, 2], [1, 2]].all(), "K >= n - 1: every frame sees every other"
    assert np.array_equal(hs.held(S[:1], Wk[:1], 8), S[:1])


# ---- the bit-parallel form ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [8, 63, 64, 65, 130])
def test_the_bit_parallel_hold_is_the_boolean_hold(w):
    rng = np.random.default_rng(w)
    for h, n, k in ((1, 2, 1), (2, 3, 1), (7, 5, 2), (34, 4, 8), (33, 9, 3)):
        S = rng.random((n, h, w)) < 0.03
        Wk = S | (rng.random((n, h, w)) < 0.4)
        S[0, 0, 0] = S[1, -1, -1] = S[0, 0, -1] = S[1, -1, 0] = True            # the corners, the first and the last row
        Wk[1, 0, :2] = Wk[0, -1, -2:] = True
        Wk |= S
        want = hs.held(S, Wk, k)
        got = ks.unpack_words(hs.hold_words(ks.pack_words(S), ks.pack_words(Wk), k), w)
        assert np.array_equal(got, want), (h, n, k)
        assert want[1, 0, 0] and want[1, 0, 1] and want[0, -1, -1] and want[0, -1, -2]


@pytest.mark.parametrize("strong_at,weak_at", [(63, 64), (64, 63)])
def test_the_carry_across_a_word_boundary(strong_at, weak_at):
    for row in (0, 3, 6):                                                       # the first row, one inside, the last
        S, Wk = maps(2, 7, 130, strong=[(0, row, strong_at)], weak=[(1, row, weak_at), (1, row, 2 * weak_at - strong_at)])
        want = hs.held(S, Wk, 1)
        assert want[1, row, weak_at] and not want[1, row, 2 * weak_at - strong_at] and want.sum() == 2
        got = ks.unpack_words(hs.hold_words(ks.pack_words(S), ks.pack_words(Wk), 1), 130)
        assert np.array_equal(got, want)


# ---- strip rows ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [(20, 56), (15, 60), (5, 38), (30, 64)])
def test_strip_rows_state_the_rows_of_the_full_frame(rows):
    """whenever the strip holds the rows of C; a strip that cuts C, or that C's box lies in front of, states its own rows"""
    fill, src, C = hovering(3)
    rng = np.random.default_rng(9)
    for f in range(fill.shape[0]):                                          # strokes about T on C's first and last rows too
        for y in (BOX[0], BOX[1] - 1, 40):
            x = int(rng.integers(BOX[2], BOX[3] - 8))
            fill[f, y:y + 1, x:x + 8] += 30 if (f + y) % 2 else 60
    C[2:4, 20:60] = 255                                                     # a second box, in front of some of the strips
    fill[:, 2:4, 30:50] += 25
    full = hs.hold(fill, src, C, T, 2)
    assert not np.array_equal(full, ks.key(fill, src, C, T)), "(the hold matters on this clip)"
    strip = hs.hold(fill[:, rows[0]:rows[1]], src[:, rows[0]:rows[1]], C, T, 2, y0=rows[0])
    cut = np.zeros_like(C)
    cut[rows[0]:rows[1]] = C[rows[0]:rows[1]]
    assert np.array_equal(strip, hs.hold(fill, src, cut, T, 2)[:, rows[0]:rows[1]])
    if rows[0] <= BOX[0] and rows[1] >= BOX[1]:
        only = np.zeros_like(C)
        only[BOX[0]:BOX[1]] = C[BOX[0]:BOX[1]]
        assert np.array_equal(strip, hs.hold(fill, src, only, T, 2)[:, rows[0]:rows[1]])
    fill, src, C = hovering(3)                                              # C inside the rows: the full-frame result sliced
    for f in range(fill.shape[0]):
        fill[f, BOX[0], 30:38] += 30 if f % 2 else 60
        fill[f, BOX[1] - 1, 90:98] += 60 if f % 2 else 30
    if rows[0] <= BOX[0] and rows[1] >= BOX[1]:
        full = hs.hold(fill, src, C, T, 2)
        assert np.array_equal(hs.hold(fill[:, rows[0]:rows[1]], src[:, rows[0]:rows[1]], C, T, 2, y0=rows[0]), full[:, rows[0]:rows[1]])
        assert not np.array_equal(full, ks.key(fill, src, C, T))


# ---- options and refusals --------------------------------------------------------------------------------------------------------------
def test_option_parsing(monkeypatch):
    from vsr_amd.backend.tools import glyph_key as gk
    from vsr_amd.backend.tools.args_handler import parse_args

    assert gk.MAX_HOLD == hs.MAX_HOLD == 8
    assert gk.hold_option(env={}) == 0 and gk.hold_option(env={"VSR_GLYPH_HOLD": ""}) == 0
    assert gk.hold_option(env={"VSR_GLYPH_HOLD": "3"}) == 3 and gk.hold_option(8, env={}) == 8
    assert gk.hold_option(2, env={"VSR_GLYPH_HOLD": "5"}) == 2, "an argument wins over the environment"
    for bad in ("-1", "9", "x", "1.5"):
        with pytest.raises(ValueError, match="glyph hold"):
            gk.hold_option(env={"VSR_GLYPH_HOLD": bad})
    for bad in (-1, 9, 1.5):
        with pytest.raises(ValueError, match="glyph hold"):
            gk.hold_option(bad)
    monkeypatch.setenv("VSR_GLYPH_HOLD", "4")
    assert gk.hold_option() == 4
    monkeypatch.delenv("VSR_GLYPH_HOLD")
    monkeypatch.delenv("VSR_GLYPH_KEY", raising=False)
    assert parse_args(["-i", "x.y4m"]).glyph_hold is None
    args = parse_args(["-i", "x.y4m", "--glyph-key", "12", "--glyph-hold", "2"])
    assert (args.glyph_key, args.glyph_hold) == (12, 2)
    assert parse_args(["-i", "x.y4m", "--glyph-hold", "0"]).glyph_hold == 0, "K = 0 needs no T"
    for bad in (["--glyph-key", "12", "--glyph-hold", "9"], ["--glyph-key", "12", "--glyph-hold", "-1"], ["--glyph-hold", "2"],
                ["--glyph-key", "0", "--glyph-hold", "2"]):
        with pytest.raises(SystemExit):
            parse_args(["-i", "x.y4m"] + bad)
    monkeypatch.setenv("VSR_GLYPH_KEY", "12")
    assert parse_args(["-i", "x.y4m", "--glyph-hold", "2"]).glyph_hold == 2, "T from the environment"


def test_flag_sets_the_environment_variable(monkeypatch):
    from vsr_amd.backend import main as m

    seen = {}

    class Stop(Exception):
        pass

    def fake_remover(path):
        import os

        seen["env"] = os.environ.get("VSR_GLYPH_KEY"), os.environ.get("VSR_GLYPH_HOLD")
        raise Stop

    assert ("glyph_hold", "VSR_GLYPH_HOLD", str) in m.FLAG_ENV
    monkeypatch.setenv("VSR_GLYPH_KEY", "0")
    monkeypatch.setenv("VSR_GLYPH_HOLD", "0")
    monkeypatch.setattr(m, "SubtitleRemover", fake_remover)
    with pytest.raises(Stop):
        m.main(["-i", "x.y4m", "--glyph-key", "12", "--glyph-hold", "3"])
    assert seen["env"] == ("12", "3")


class FakeDist:
    @staticmethod
    def get_world_size():
        return 2

    @staticmethod
    def get_rank():
        return 0


def others_off(monkeypatch):
    for name in FIVE:
        monkeypatch.delenv(name, raising=False)


def test_refuse_ranks(monkeypatch):
    from vsr_amd.backend.tools import glyph_key as gk
    from vsr_amd.backend.tools import seam_feather as sf

    others_off(monkeypatch)
    monkeypatch.delenv("VSR_GLYPH_HOLD", raising=False)
    assert gk.refuse_ranks(None) == 0 and gk.refuse_ranks(None, 12, 2) == 12 and gk.refuse_ranks(FakeDist, 0, 0) == 0
    with pytest.raises(ValueError, match=r"--glyph-hold .*--glyph-key"):
        gk.refuse_ranks(None, 0, 2)
    with pytest.raises(ValueError, match="glyph hold"):
        gk.refuse_ranks(None, 12, 9)
    with pytest.raises(RuntimeError, match="--glyph-key .* one process"):
        gk.refuse_ranks(FakeDist, 12, 2)
    monkeypatch.setenv("VSR_GLYPH_KEY", "12")
    monkeypatch.setenv("VSR_GLYPH_HOLD", "2")
    assert sf.options() == (0, 0, 0, 0) and sf.refuse_ranks_all(None) == (0, 0, 0, 0), "still four values"
    monkeypatch.setenv("VSR_GLYPH_KEY", "0")
    with pytest.raises(ValueError, match=r"VSR_GLYPH_HOLD.*VSR_GLYPH_KEY"):
        sf.refuse_ranks_all(None)


@pytest.mark.parametrize("entry", ["run", "video_inpaint", "propainter_mode"])
def test_refusals_come_before_a_frame_is_read(monkeypatch, entry):
    from vsr_amd.backend import main as m
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
    monkeypatch.setattr(sr, "_distributed", lambda: None)
    monkeypatch.setenv("VSR_GLYPH_KEY", "12")
    monkeypatch.setenv("VSR_GLYPH_HOLD", "9")
    with pytest.raises(ValueError, match="glyph hold"):
        call()
    monkeypatch.setenv("VSR_GLYPH_HOLD", "2")
    monkeypatch.setenv("VSR_GLYPH_KEY", "0")
    with pytest.raises(ValueError, match=r"--glyph-hold .*--glyph-key"):
        call()
    monkeypatch.setenv("VSR_GLYPH_KEY", "12")
    monkeypatch.setattr(sr, "_distributed", lambda: FakeDist)
    with pytest.raises(RuntimeError, match="--glyph-key .* one process"):
        call()


def test_sttn_auto_refuses_before_the_source_is_opened(monkeypatch):
    from vsr_amd.backend.inpaint import sttn_auto_inpaint as sa

    def no_work(*a, **kw):
        raise AssertionError("the source was opened")

    monkeypatch.setattr(sa, "open_video", no_work)
    auto = object.__new__(sa.STTNAutoInpaint)
    auto.context = auto.scene_split = auto.lookahead = None
    auto.clip_gap = 50
    others_off(monkeypatch)
    monkeypatch.setenv("VSR_GLYPH_HOLD", "2")
    with pytest.raises(ValueError, match=r"--glyph-hold .*--glyph-key"):
        auto._run(None, None, None, None)
    monkeypatch.setenv("VSR_GLYPH_KEY", "12")
    monkeypatch.setenv("VSR_GLYPH_HOLD", "x")
    with pytest.raises(ValueError, match="glyph hold"):
        auto._run(None, None, None, None)
    monkeypatch.setenv("VSR_GLYPH_HOLD", "2")
    with pytest.raises(RuntimeError, match="--glyph-key .* one process"):
        auto._run(FakeDist, None, None, None)


# ---- the chain ---------------------------------------------------------------------------------------------------------------------------
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
    """the five passes replaced by stand-ins of the signatures they had before --glyph-hold: a call site that handed glyph_key.apply a
    sixth argument would fail here"""
    from vsr_amd.backend.tools import deflicker, glyph_key, regrain, seam_feather, tone_match

    log = []
    monkeypatch.setattr(tone_match, "sets", lambda cm, rows, device: "bands")
    monkeypatch.setattr(regrain, "sets", lambda cm, rows, device: "sets")
    monkeypatch.setattr(glyph_key, "mask", lambda cm, device: "mask")
    monkeypatch.setattr(seam_feather, "alpha", lambda cm, feather, device: np.zeros(cm.shape, np.uint8))
    monkeypatch.setattr(tone_match, "apply", lambda frames, src, s, percent, y0=0: log.append(("tone", percent, y0)))
    monkeypatch.setattr(deflicker, "apply", lambda frames, src, s, radius, y0=0: log.append(("deflicker", radius, y0)))
    monkeypatch.setattr(regrain, "apply", lambda frames, src, s, percent, y0=0: log.append(("regrain", percent, y0)))
    monkeypatch.setattr(glyph_key, "apply", lambda frames, src, m, t, y0=0: log.append(("key", t, y0, glyph_key.hold_option())))
    monkeypatch.setattr(seam_feather, "composite", lambda frames, src, d, feather: log.append(("feather", feather)))
    return log


@pytest.mark.parametrize("form", ["device tensor", "list, device body", "list, host body"])
def test_the_chain_is_unchanged(monkeypatch, recorded, form):
    import torch

    from vsr_amd.backend.tools import seam_feather

    mask = np.zeros((24, 40), np.uint8)
    mask[10:16, 5:30] = 255
    frames = [np.full((24, 40, 3), i, np.uint8) for i in range(3)]
    plugin = Plugin(recorded, accepts_device_frames=form != "list, host body")
    given = torch.from_numpy(np.stack(frames)) if form == "device tensor" else frames

    def call():
        del recorded[:]
        seam_feather.plugin_call(plugin, plugin.body, given, mask, "cpu")
        return list(recorded)

    others_off(monkeypatch)
    monkeypatch.setenv("VSR_GLYPH_HOLD", "0")
    assert call() == ["body"]
    monkeypatch.setenv("VSR_GLYPH_KEY", "12")
    assert call() == ["body", ("key", 12, 0, 0)]
    monkeypatch.setenv("VSR_GLYPH_HOLD", "2")
    assert call() == ["body", ("key", 12, 0, 2)], "the same call; K is read inside apply"
    monkeypatch.setenv("VSR_SEAM_FEATHER", "4")
    monkeypatch.setenv("VSR_REGRAIN", "100")
    monkeypatch.setenv("VSR_DEFLICKER", "2")
    monkeypatch.setenv("VSR_TONE_MATCH", "80")
    assert call() == ["body", ("tone", 80, 0), ("deflicker", 2, 0), ("regrain", 100, 0), ("key", 12, 0, 2), ("feather", 4)]


def test_sttn_auto_calls_apply_as_before(monkeypatch, recorded):
    import torch

    from vsr_amd.backend.inpaint import sttn_auto_inpaint as sa

    class Engine:
        def auto_chunk(self, frames, mask, areas, **kw):
            recorded.append("body")

    plugin = object.__new__(sa.STTNInpaint)
    plugin.engine = Engine()
    others_off(monkeypatch)
    monkeypatch.setenv("VSR_GLYPH_KEY", "12")
    monkeypatch.setenv("VSR_GLYPH_HOLD", "3")
    cm = np.zeros((48, 40), np.uint8)
    cm[20:30, 4:30] = 255
    plugin.auto_chunk(torch.zeros((2, 22, 40, 3), dtype=torch.uint8), None, [(6, 16, 0, 40)], cmask=cm, rows=(14, 36))
    assert recorded == ["body", ("key", 12, 14, 3)]


def test_apply_reads_the_option_when_it_is_given_none(monkeypatch):
    """apply(..., hold=None) asks hold_option(), apply(..., hold=K) does not; without a GPU the call ends at the first check after it"""
    import torch

    from vsr_amd.backend.tools import glyph_key as gk

    sig = inspect.signature(gk.apply)
    assert list(sig.parameters) == ["frames", "src", "m", "T", "y0", "hold"] and sig.parameters["hold"].default is None

    class Asked(Exception):
        pass

    def asked(*a, **kw):
        raise Asked

    monkeypatch.setattr(gk, "hold_option", asked)
    frames = torch.zeros((2, 8, 8, 3), dtype=torch.uint8)
    m = gk.Mask(torch.zeros((8, 8), dtype=torch.uint8), 2, 6)
    with pytest.raises(Asked):
        gk.apply(frames, frames.clone(), m, 12)
    for k in (0, 2):
        with pytest.raises(AssertionError):                                 # frames on the host: refused, and the option was not asked
            gk.apply(frames, frames.clone(), m, 12, hold=k)
    assert gk.apply(frames, frames.clone(), m, 0) is frames, "T = 0: nothing is read, nothing runs"
