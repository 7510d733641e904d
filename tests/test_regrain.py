"""--regrain without a GPU: the statement checks itself (tests/_regrain_statement.py) and does what it is for on a synthetic clip, the
option is parsed in one place, and several ranks are refused before any frame is read."""
import numpy as np
import pytest

from tests import _regrain_statement as rs

H, W = 120, 320
BAND = (60, 100)


def _masks(h, w, seed):
    rng = np.random.default_rng(seed)
    out = {"empty": np.zeros((h, w), np.uint8), "full": np.full((h, w), 255, np.uint8)}
    band = np.zeros((h, w), np.uint8)
    band[h // 2:, :] = 255                                         # touches the bottom, left and right frame edges
    out["bottom band"] = band
    two = np.zeros((h, w), np.uint8)
    two[3:h // 3, 2:w // 2] = 255
    two[h // 2:h - 4, w // 2 + 3:w - 1] = 7                        # any non-zero value is inside
    out["two rectangles"] = two
    line = np.zeros((h, w), np.uint8)
    line[2:h - 2, w // 2] = 255
    out["line"] = line
    out["random blob"] = (rng.random((h, w)) < 0.9).astype(np.uint8) * 255
    out["sparse"] = (rng.random((h, w)) < 0.003).astype(np.uint8)
    return out


@pytest.mark.parametrize("shape,R", [((37, 53), (0, 37)), ((37, 53), (5, 30)), ((3, 9), (0, 3)), ((40, 3), (0, 40)), ((2, 9), (0, 2)),
                                     ((37, 53), (7, 7))])
def test_separable_sets_are_the_brute_force_sets(shape, R):
    for name, C in _masks(*shape, seed=shape[0]).items():
        E, I = rs.sets(C, R)
        Eb, Ib = rs.sets_brute(C, R)
        assert np.array_equal(E, Eb) and np.array_equal(I, Ib), name
        assert not (E & I).any() and not E[C != 0].any() and I[C == 0].sum() == 0, name
        m = rs.sets_map(C, R)
        assert np.array_equal(m & 1, E) and np.array_equal((m >> 1) & 1, I) and np.array_equal(m >> 2, C != 0), name


def test_sets_of_the_edge_cases():
    m = _masks(37, 53, 1)
    assert not rs.sets(m["line"], (0, 37))[1].any(), "a one-pixel line has no interior sample"
    assert rs.sets(m["line"], (0, 37))[0].any()
    assert not rs.sets(m["full"], (0, 37))[0].any(), "a mask that covers the frame has no ring"
    assert rs.sets(m["full"], (0, 37))[1].sum() == 35 * 51
    E, I = rs.sets(m["bottom band"], (0, 37))
    ys = np.flatnonzero(E.any(axis=1))
    assert ys.min() == 18 - 1 - 16 + 1 and ys.max() == 16, "the ring: 16 rows, none closer than two rows to the band (rows 18..)"
    assert np.flatnonzero(I.any(axis=1)).tolist() == list(range(19, 36))


def test_the_noise_operator_is_blind_to_planes_and_straight_edges():
    y, x = np.mgrid[0:20, 0:30]
    plane = np.repeat((3 * x + 2 * y + 7)[..., None], 3, axis=2)
    assert not rs.noise_level(plane).any()
    step = np.repeat(np.where(x < 15, 10, 200)[..., None], 3, axis=2)
    assert not rs.noise_level(step).any()
    dot = np.zeros((5, 5, 3), np.int64)
    dot[2, 2] = 1
    assert rs.noise_level(dot)[1:4, 1:4].tolist() == [[3, 6, 3], [6, 12, 6], [3, 6, 3]]
    assert rs.noise_level(np.full((5, 5, 3), 255) * (np.indices((5, 5)).sum(axis=0) % 2)[..., None]).max() == 3 * 8 * 255      # the most there is


def test_integer_square_root_and_constant():
    for v in (0, 1, 2, 3, 4, 15, 16, 17, 2 ** 40 - 1, 2 ** 40, (16 * 255 * 256) ** 2, (16 * 255 * 256) ** 2 - 1):
        r = rs.isqrt(v)
        assert r * r <= v < (r + 1) * (r + 1)
    assert rs.GAIN == 60701
    # r <= 16 * 255 * 256, P <= 200, |z| <= 510: the product stays below 2^63
    assert 16 * 255 * 256 * 200 * rs.GAIN * 510 + 2 ** 39 < 2 ** 63


def test_the_hash_is_32_bit_and_the_grain_is_centred():
    assert int(rs.mix(np.array([0], np.uint32))[0]) == 0
    h = 1
    h ^= h >> 16
    h = (h * 0x7feb352d) & 0xffffffff
    h ^= h >> 15
    h = (h * 0x846ca68b) & 0xffffffff
    h ^= h >> 16
    assert int(rs.mix(np.array([1], np.uint32))[0]) == h
    # g with r * P * GAIN = 2^40 is z itself: Irwin-Hall of four bytes, mean 0, standard deviation sqrt(65535 / 3) = 147.8
    k = 2 ** 40 // rs.GAIN
    g = rs.grain(200, 300, 12345, k, 1).astype(np.float64) * (2 ** 40 / (k * rs.GAIN))
    assert g.shape == (200, 300) and abs(g.mean()) < 2.0 and abs(g.std() - 147.8) < 1.5 and np.abs(g).max() <= 512
    assert np.array_equal(rs.grain(200, 300, 7, 1000, 100)[50:80], rs.grain(200, 300, 7, 1000, 100, y0=50, rows=30)), "full-frame coordinates"
    assert not np.array_equal(rs.grain(200, 300, 7, 1000, 100), rs.grain(200, 300, 8, 1000, 100))


def clip(sigma, seed, n=2):
    """a plane with independent Gaussian noise per sample; the fill: the noise-free plane, five levels up, under the band"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    plane = (90 + 0.11 * x + 0.23 * y)[None, :, :, None] + np.zeros((n, 1, 1, 3))
    src = np.clip(np.rint(plane + rng.normal(0.0, sigma, plane.shape)), 0, 255).astype(np.uint8)
    C = np.zeros((H, W), np.uint8)
    C[BAND[0]:BAND[1]] = 255
    fill = src.copy()
    fill[:, C != 0] = (np.rint(plane) + 5).astype(np.uint8)[:, C != 0]
    return src, fill, C


@pytest.mark.parametrize("sigma", [2, 6, 12])
def test_the_band_gets_the_rings_noise_level(sigma):
    """P = 100: mean L(out) over I / mean L(src) over E in [0.95, 1.06].  The bound: about 10^4 ring samples give a sampling error of
    about 1 %, rounding the grain to integers adds 1/12 to its variance (2 % at sigma = 2).  The statement's own values on these clips
    are recorded in DESIGN 4.12."""
    src, fill, C = clip(sigma, seed=100 + sigma)
    R = (0, H)
    info = []
    out = rs.regrain(fill, src, C, R, 100, info=info)
    E, I = rs.sets(C, R)
    assert E.sum() > 9000 and I.sum() > 9000
    for t in range(src.shape[0]):
        ratio = rs.noise_level(out[t])[I].mean() / rs.noise_level(src[t])[E].mean()
        print(f"sigma {sigma} frame {t}: r {info[t][3]} ratio {ratio:.4f}")
        assert info[t][5] and 0.95 <= ratio <= 1.06, ratio
        assert rs.noise_level(fill[t])[I].mean() < 0.2 * rs.noise_level(src[t])[E].mean(), "the fill was flat"
    assert np.array_equal(out[:, C == 0], fill[:, C == 0]), "pixels outside C are never changed"
    assert (out[:, C != 0] != fill[:, C != 0]).any()
    # achromatic: the same value on the three channels (no clamp is reached on this clip)
    delta = out.astype(np.int64) - fill
    assert np.array_equal(delta[..., 0], delta[..., 1]) and np.array_equal(delta[..., 0], delta[..., 2])
    # P scales the grain
    half = rs.regrain(fill, src, C, R, 50).astype(np.int64) - fill
    assert 0.4 < np.abs(half).mean() / np.abs(delta).mean() < 0.6


def test_a_fill_as_noisy_as_the_ring_gets_nothing():
    src, fill, C = clip(2, seed=3)
    rng = np.random.default_rng(4)
    noisy = fill.copy()
    noisy[:, C != 0] = np.clip(fill[:, C != 0].astype(np.int64) + np.rint(rng.normal(0, 6, fill[:, C != 0].shape)), 0, 255).astype(np.uint8)
    info = []
    out = rs.regrain(noisy, src, C, (0, H), 100, info=info)
    assert all(i[3] == 0 for i in info) and np.array_equal(out, noisy)


def test_p_zero_is_the_identity_and_an_untouched_frame_stays():
    src, fill, C = clip(6, seed=5, n=3)
    assert np.array_equal(rs.regrain(fill, src, C, (0, H), 0), fill)
    fill[1] = src[1]                                               # a frame the call did not inpaint
    info = []
    out = rs.regrain(fill, src, C, (0, H), 100, info=info)
    assert [i[5] for i in info] == [True, False, True] and np.array_equal(out[1], src[1])
    # E or I empty: untouched
    full = np.full((H, W), 255, np.uint8)
    assert np.array_equal(rs.regrain(fill, src, full, (0, H), 100), fill)
    line = np.zeros((H, W), np.uint8)
    line[70, :] = 255
    assert np.array_equal(rs.regrain(fill, src, line, (0, H), 100), fill)


def test_identical_frames_get_identical_grain_and_batching_does_not_matter():
    src, fill, C = clip(6, seed=6, n=1)
    src3, fill3 = np.concatenate([src] * 3), np.concatenate([fill] * 3)
    out = rs.regrain(fill3, src3, C, (0, H), 100)
    assert np.array_equal(out[0], out[1]) and np.array_equal(out[0], out[2])
    assert np.array_equal(out[:1], rs.regrain(fill, src, C, (0, H), 100))


def test_strip_rows_state_the_rows_of_the_full_frame():
    """R a proper sub-range: the frames of the full form and the rows of the strip form agree, and the samples stay inside R"""
    src, fill, C = clip(6, seed=7)
    R = (50, 112)
    E, I = rs.sets(C, R)
    assert E[51:60].any() and not E[:51].any() and not E[111:].any()
    full = rs.regrain(fill, src, C, R, 100)
    rows = rs.regrain(fill[:, R[0]:R[1]], src[:, R[0]:R[1]], C, R, 100, y0=R[0])
    assert np.array_equal(rows, full[:, R[0]:R[1]]) and np.array_equal(full[:, :R[0]], fill[:, :R[0]])
    assert not np.array_equal(full, rs.regrain(fill, src, C, (0, H), 100)), "other samples, another seed"


def test_sample_rows_mirror_the_plugins():
    from vsr_amd.backend.inpaint.lama_inpaint import LamaInpaint
    from vsr_amd.backend.inpaint.opencv_inpaint import OpenCVInpaint
    from vsr_amd.backend.inpaint.propainter_inpaint import PropainterInpaint
    from vsr_amd.backend.inpaint.sttn_auto_inpaint import STTNInpaint
    from vsr_amd.backend.inpaint.sttn_det_inpaint import STTNDetInpaint

    M = np.zeros((480, 852), np.uint8)
    M[300:340, 100:700] = 255
    M[89:91, 10:60] = 255
    for cls, mode in ((STTNDetInpaint, "sttn-det"), (LamaInpaint, "lama"), (OpenCVInpaint, "opencv"), (PropainterInpaint, "propainter")):
        assert cls.sample_rows(object.__new__(cls), M) == rs.sample_rows(mode, M) == (0, 480), mode
    r0, r1 = STTNInpaint.sample_rows(object.__new__(STTNInpaint), M)
    assert (r0, r1) == rs.sample_rows("sttn-auto", M) and 0 < r0 <= 89 and 340 <= r1 < 480
    C = STTNInpaint.composite_mask(object.__new__(STTNInpaint), M)
    assert not C[:r0].any() and not C[r1:].any(), "sttn-auto's C lies inside its sample rows"
    assert STTNInpaint.sample_rows(object.__new__(STTNInpaint), np.zeros((480, 852), np.uint8)) == (0, 0)


def test_option_parsing(monkeypatch):
    from vsr_amd.backend.tools import regrain as rg
    from vsr_amd.backend.tools.args_handler import parse_args

    assert rg.regrain_option(env={}) == 0 and rg.regrain_option(env={"VSR_REGRAIN": ""}) == 0
    assert rg.regrain_option(env={"VSR_REGRAIN": "100"}) == 100 and rg.regrain_option(200, env={}) == 200
    assert rg.regrain_option(30, env={"VSR_REGRAIN": "90"}) == 30, "an argument wins over the environment"
    for bad in ("-1", "201", "x", "1.5"):
        with pytest.raises(ValueError, match="regrain"):
            rg.regrain_option(env={"VSR_REGRAIN": bad})
    for bad in (-1, 201, 1.5):
        with pytest.raises(ValueError, match="regrain"):
            rg.regrain_option(bad)
    monkeypatch.setenv("VSR_REGRAIN", "50")
    assert rg.regrain_option() == 50
    assert parse_args(["-i", "x.y4m"]).regrain is None
    assert parse_args(["-i", "x.y4m", "--regrain", "100"]).regrain == 100
    for bad in ("201", "-1"):
        with pytest.raises(SystemExit):
            parse_args(["-i", "x.y4m", "--regrain", bad])


def test_flag_sets_the_environment_variable(monkeypatch):
    from vsr_amd.backend import main as m

    seen = {}

    class Stop(Exception):
        pass

    def fake_remover(path):
        import os

        seen["env"] = os.environ.get("VSR_REGRAIN")
        raise Stop

    monkeypatch.setenv("VSR_REGRAIN", "0")
    monkeypatch.setattr(m, "SubtitleRemover", fake_remover)
    with pytest.raises(Stop):
        m.main(["-i", "x.y4m", "--regrain", "100"])
    assert seen["env"] == "100"


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
    from vsr_amd.backend.tools import regrain as rg
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
    monkeypatch.setenv("VSR_REGRAIN", "100")
    with pytest.raises(RuntimeError, match="one process"):
        call()
    monkeypatch.setenv("VSR_REGRAIN", "201")
    with pytest.raises(ValueError, match="regrain"):
        call()
    # off, or one rank: nothing is refused
    assert rg.refuse_ranks(FakeDist, 0) == 0 and rg.refuse_ranks(None, 100) == 100


def test_sttn_auto_refuses_several_ranks_before_the_source_is_opened(monkeypatch):
    from vsr_amd.backend.inpaint import sttn_auto_inpaint as sa

    def no_work(*a, **kw):
        raise AssertionError("the source was opened")

    monkeypatch.setattr(sa, "open_video", no_work)
    auto = object.__new__(sa.STTNAutoInpaint)
    auto.context = auto.scene_split = auto.lookahead = None
    auto.clip_gap = 50
    monkeypatch.delenv("VSR_SEAM_FEATHER", raising=False)
    monkeypatch.setenv("VSR_REGRAIN", "100")
    with pytest.raises(RuntimeError, match="one process"):
        auto._run(FakeDist, None, None, None)
