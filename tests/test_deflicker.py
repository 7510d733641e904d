"""--deflicker without a GPU: the statement (tests/_deflicker_statement.py) does what it is for on synthetic clips, the option is parsed
in one place, and several ranks are refused before any frame is read."""
import numpy as np
import pytest

from tests import _deflicker_statement as ds
from tests import _regrain_statement as rs

H, W = 72, 160
BAND = (32, 52)
TH = ds.TH


def clip(sigma, seed, n, offsets=None):
    """src: a plane with independent Gaussian noise per sample and frame (a still scene with grain); fill: one smooth picture under the
    band in every frame, plus offsets[t]"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    plane = (90 + 0.11 * x + 0.23 * y)[None, :, :, None] + np.zeros((n, 1, 1, 3))
    src = np.clip(np.rint(plane + rng.normal(0.0, sigma, plane.shape)), 0, 255).astype(np.uint8)
    C = np.zeros((H, W), np.uint8)
    C[BAND[0]:BAND[1]] = 255
    smooth = np.rint(plane[0] + 20 * np.sin(x / 9.0)[..., None] + np.array([0, 3, -2])).astype(np.int64)
    fill = src.copy()
    for t in range(n):
        fill[t][C != 0] = np.clip(smooth + (0 if offsets is None else int(offsets[t])), 0, 255).astype(np.uint8)[C != 0]
    return src, fill, C


def flicker(n, seed):
    return np.random.default_rng(seed).integers(-TH + 1, TH, n)                  # every integer of (-TH, TH)


def test_constants():
    assert ds.GRAIN == 15447 and ds.TH == 24 and ds.FULL == 16 and ds.MAX_DEFLICKER == 8
    # the largest numerator of a pixel: 16 TH + 16 neighbours of weight 16 TH, times 255, stays in 32 bits
    assert (16 * TH + 2 * ds.MAX_DEFLICKER * 16 * TH) * 255 + 16 * TH * 17 < 2 ** 31
    # the gate: full up to one level per sample, none from four
    m = 3 * 1000
    assert ds.pair_weight(m, 0, 0, True, True, m) == 16 and ds.pair_weight(m + 200, 0, 0, True, True, m) == 15
    assert ds.pair_weight(4 * m, 0, 0, True, True, m) == 0 and ds.pair_weight(4 * m - 1, 0, 0, True, True, m) == 0
    assert ds.pair_weight(4 * m - 600, 0, 0, True, True, m) == 1 and ds.pair_weight(100 * m, 0, 0, True, True, m) == 0
    assert ds.pair_weight(0, 0, 0, False, True, m) == ds.pair_weight(0, 0, 0, True, False, m) == ds.pair_weight(0, 0, 0, True, True, 0) == 0
    # the grain floor: (15447 (A + A')) >> 17 = sqrt(2) / 6 of the mean of the two sums
    assert ds.pair_weight(m + 4242, 18000, 18000, True, True, m) == 16 and (15447 * 36000) >> 17 == 4242


def test_identical_fills_are_a_fixed_point():
    src, fill, C = clip(6, seed=1, n=5)
    info = {}
    out = ds.deflicker(fill, src, C, (0, H), 2, info=info)
    assert set(info["a"].values()) == {16}, "the pairs were open"
    assert np.array_equal(out, fill)


def test_r_zero_and_one_frame_are_the_identity():
    src, fill, C = clip(6, seed=2, n=4, offsets=[5, -5, 9, 0])
    assert np.array_equal(ds.deflicker(fill, src, C, (0, H), 0), fill)
    assert not np.array_equal(ds.deflicker(fill, src, C, (0, H), 1), fill)
    for R in (1, 8):
        assert np.array_equal(ds.deflicker(fill[:1], src[:1], C, (0, H), R), fill[:1])
    # a mask without a ring: the identity
    full = np.full((H, W), 255, np.uint8)
    assert np.array_equal(ds.deflicker(fill, src, full, (0, H), 2), fill)


def test_an_uninpainted_frame_stays_and_lends_nothing():
    src, fill, C = clip(6, seed=3, n=5, offsets=[5, -5, 0, 7, -3])
    fill[2] = src[2]                                               # a frame the call did not inpaint
    info = {}
    out = ds.deflicker(fill, src, C, (0, H), 2, info=info)
    assert info["changed"] == [True, True, False, True, True]
    assert np.array_equal(out[2], src[2])
    for (t, k), a in info["a"].items():
        assert (a == 0) == (2 in (t, t + k)), (t, k, a)
    # whatever that frame shows under the mask, its neighbours come out the same
    src2, fill2 = src.copy(), fill.copy()
    src2[2][C != 0] = 255 - src2[2][C != 0]
    fill2[2] = src2[2]
    out2 = ds.deflicker(fill2, src2, C, (0, H), 2)
    assert np.array_equal(out2[[0, 1, 3, 4]], out[[0, 1, 3, 4]]) and not np.array_equal(out[[0, 1, 3, 4]], fill[[0, 1, 3, 4]])
    # and they are what the definition gives with that frame's weights at zero: frame 1 sees frames 0 and 3 only
    f = fill.astype(np.int64)
    num, den = 16 * TH * f[1], np.full((H, W), 16 * TH, np.int64)
    for s in (0, 3):
        D = np.abs(f[s] - f[1]).max(axis=-1)
        w = np.where(D < TH, 16 * (TH - D), 0)
        num, den = num + w[..., None] * f[s], den + w
    want = ((num + (den // 2)[..., None]) // den[..., None]).astype(np.uint8)
    assert np.array_equal(out[1][C != 0], want[C != 0])


@pytest.mark.parametrize("sigma", [2, 6, 12])
def test_a_still_scene_with_grain_keeps_every_pair_open(sigma):
    """the ring's frame differences are the source's grain and nothing else: the floor takes them away, every weight is 16, and the
    flicker (a per-frame offset in (-TH, TH)) shrinks at every pixel while the temporal mean stays within a level"""
    n, R = 8, 2
    offsets = flicker(n, seed=sigma)
    assert offsets.max() - offsets.min() >= TH, "some frames are too far apart to be mixed with each other"
    src, fill, C = clip(sigma, seed=100 + sigma, n=n, offsets=offsets)
    info = {}
    out = ds.deflicker(fill, src, C, (0, H), R, info=info)
    m = info["m"]
    for (t, k), a in info["a"].items():
        moved = int(info["S"][t, k - 1]) - ((ds.GRAIN * (info["A"][t] + info["A"][t + k])) >> 17)
        print(f"sigma {sigma} pair ({t}, {k}): S/m {info['S'][t, k - 1] / m:.3f} moved/m {moved / m:+.4f} a {a}")
        assert a == 16, (t, k)
    assert info["S"].max() / m > 0.55 * sigma, "the grain alone is worth more than a level per sample"
    inside = C != 0
    f, o = fill[:, inside].astype(np.int64), out[:, inside].astype(np.int64)
    assert ((o.max(axis=0) - o.min(axis=0)) < (f.max(axis=0) - f.min(axis=0))).all()
    assert np.abs(o.mean(axis=0) - f.mean(axis=0)).max() <= 1.0
    assert np.array_equal(out[:, ~inside], fill[:, ~inside]), "pixels outside C are never changed"


def test_a_cut_closes_every_pair_across_it():
    n, R, j = 7, 2, 3
    src, fill, C = clip(6, seed=7, n=n, offsets=flicker(n, seed=7))
    rng = np.random.default_rng(8)
    other = np.clip(np.rint(170 - 0.2 * np.mgrid[0:H, 0:W][1][None, :, :, None] + rng.normal(0, 6, src[j:].shape)), 0, 255).astype(np.uint8)
    src[j:][:, C == 0] = other[:, C == 0]                           # the picture around the band is another one from frame j on
    fill[j:][:, C == 0] = other[:, C == 0]
    info = {}
    out = ds.deflicker(fill, src, C, (0, H), R, info=info)
    for (t, k), a in info["a"].items():
        assert a == (0 if t < j <= t + k else 16), (t, k, a)
    assert np.array_equal(out[:j], ds.deflicker(fill[:j], src[:j], C, (0, H), R))
    assert np.array_equal(out[j:], ds.deflicker(fill[j:], src[j:], C, (0, H), R))
    assert not np.array_equal(out[:j], fill[:j]) and not np.array_equal(out[j:], fill[j:])


def test_a_fill_that_differs_by_th_is_not_mixed_there():
    src, fill, C = clip(6, seed=9, n=2)
    half = W // 2
    f1 = fill[1].astype(np.int64)
    f1[BAND[0]:BAND[1], :half, 1] += TH                              # one channel TH away: other content
    f1[BAND[0]:BAND[1], half:] += TH - 1
    fill[1] = np.clip(f1, 0, 255).astype(np.uint8)
    assert fill.max() < 255
    out = ds.deflicker(fill, src, C, (0, H), 1)
    assert np.array_equal(out[:, :, :half], fill[:, :, :half])
    band = out[:, BAND[0]:BAND[1], half:].astype(np.int64) - fill[:, BAND[0]:BAND[1], half:]
    # D = TH - 1: w = 16 against 16 TH: TH - 1 levels * 16 / (16 TH + 16) rounds to one level, towards the other frame
    assert (band[0] == 1).all() and (band[1] == -1).all()


def test_batching_matters_within_r_frames_of_the_split():
    """the window is the call: a batch and its two halves agree except within R frames of the split, where the halves' windows are
    one-sided"""
    n, R, cut = 10, 2, 5
    src, fill, C = clip(6, seed=11, n=n, offsets=flicker(n, seed=11))
    whole = ds.deflicker(fill, src, C, (0, H), R)
    halves = np.concatenate([ds.deflicker(fill[:cut], src[:cut], C, (0, H), R), ds.deflicker(fill[cut:], src[cut:], C, (0, H), R)])
    differ = [t for t in range(n) if not np.array_equal(whole[t], halves[t])]
    assert differ and set(differ) <= set(range(cut - R, cut + R)), differ


def test_strip_rows_state_the_rows_of_the_full_frame():
    n = 4
    src, fill, C = clip(6, seed=13, n=n, offsets=flicker(n, seed=13))
    rows = (24, 64)
    E = rs.sets(C, rows)[0]
    assert E[25:31].any() and not E[:25].any() and not E[63:].any() and E.sum() < rs.sets(C, (0, H))[0].sum()
    full = ds.deflicker(fill, src, C, rows, 2)
    strip = ds.deflicker(fill[:, rows[0]:rows[1]], src[:, rows[0]:rows[1]], C, rows, 2, y0=rows[0])
    assert np.array_equal(strip, full[:, rows[0]:rows[1]]) and np.array_equal(full[:, :rows[0]], fill[:, :rows[0]])
    assert not np.array_equal(full, fill)


def test_option_parsing(monkeypatch):
    from vsr_amd.backend.tools import deflicker as df
    from vsr_amd.backend.tools.args_handler import parse_args

    assert df.deflicker_option(env={}) == 0 and df.deflicker_option(env={"VSR_DEFLICKER": ""}) == 0
    assert df.deflicker_option(env={"VSR_DEFLICKER": "2"}) == 2 and df.deflicker_option(8, env={}) == 8
    assert df.deflicker_option(3, env={"VSR_DEFLICKER": "5"}) == 3, "an argument wins over the environment"
    for bad in ("-1", "9", "x", "1.5"):
        with pytest.raises(ValueError, match="deflicker"):
            df.deflicker_option(env={"VSR_DEFLICKER": bad})
    for bad in (-1, 9, 1.5):
        with pytest.raises(ValueError, match="deflicker"):
            df.deflicker_option(bad)
    monkeypatch.setenv("VSR_DEFLICKER", "4")
    assert df.deflicker_option() == 4
    assert parse_args(["-i", "x.y4m"]).deflicker is None
    assert parse_args(["-i", "x.y4m", "--deflicker", "2"]).deflicker == 2
    for bad in ("9", "-1"):
        with pytest.raises(SystemExit):
            parse_args(["-i", "x.y4m", "--deflicker", bad])


def test_flag_sets_the_environment_variable(monkeypatch):
    from vsr_amd.backend import main as m

    seen = {}

    class Stop(Exception):
        pass

    def fake_remover(path):
        import os

        seen["env"] = os.environ.get("VSR_DEFLICKER")
        raise Stop

    monkeypatch.setenv("VSR_DEFLICKER", "0")
    monkeypatch.setattr(m, "SubtitleRemover", fake_remover)
    with pytest.raises(Stop):
        m.main(["-i", "x.y4m", "--deflicker", "2"])
    assert seen["env"] == "2"


class FakeDist:
    @staticmethod
    def get_world_size():
        return 2

    @staticmethod
    def get_rank():
        return 0


@pytest.mark.parametrize("entry", ["run", "video_inpaint", "propainter_mode"])
def test_several_ranks_are_refused_before_a_frame_is_read(monkeypatch, entry):
    from vsr_amd.backend import main as m
    from vsr_amd.backend.tools import deflicker as df
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
    monkeypatch.delenv("VSR_SEAM_FEATHER", raising=False)
    monkeypatch.delenv("VSR_REGRAIN", raising=False)
    monkeypatch.setenv("VSR_DEFLICKER", "2")
    with pytest.raises(RuntimeError, match="one process"):
        call()
    monkeypatch.setenv("VSR_DEFLICKER", "9")
    with pytest.raises(ValueError, match="deflicker"):
        call()
    # off, or one rank: nothing is refused
    assert df.refuse_ranks(FakeDist, 0) == 0 and df.refuse_ranks(None, 2) == 2


def test_sttn_auto_refuses_several_ranks_before_the_source_is_opened(monkeypatch):
    from vsr_amd.backend.inpaint import sttn_auto_inpaint as sa

    def no_work(*a, **kw):
        raise AssertionError("the source was opened")

    monkeypatch.setattr(sa, "open_video", no_work)
    auto = object.__new__(sa.STTNAutoInpaint)
    auto.context = auto.scene_split = auto.lookahead = None
    auto.clip_gap = 50
    monkeypatch.delenv("VSR_SEAM_FEATHER", raising=False)
    monkeypatch.delenv("VSR_REGRAIN", raising=False)
    monkeypatch.setenv("VSR_DEFLICKER", "2")
    with pytest.raises(RuntimeError, match="one process"):
        auto._run(FakeDist, None, None, None)
