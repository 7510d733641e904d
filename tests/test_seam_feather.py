"""--seam-feather without a GPU: the statement checks itself (tests/_feather_statement.py), the option is parsed in one place, and
several ranks are refused before any frame is read."""
import numpy as np
import pytest

from tests import _feather_statement as fs


def _masks(H, W, seed):
    rng = np.random.default_rng(seed)
    out = {"empty": np.zeros((H, W), np.uint8), "full": np.full((H, W), 255, np.uint8)}
    one = np.zeros((H, W), np.uint8)
    one[H // 2, W // 2] = 1
    out["one pixel"] = one
    edge = np.zeros((H, W), np.uint8)
    edge[H // 2:, W // 3:] = 255                                   # touches the bottom and the right frame edge
    out["edge rectangle"] = edge
    two = np.zeros((H, W), np.uint8)
    two[2:H - 2, 2:W // 2] = 255
    two[2:H - 2, W // 2 + 1:W - 1] = 255                           # one pixel apart
    out["two rectangles"] = two
    blob = (rng.random((H, W)) < 0.97).astype(np.uint8) * 255
    out["random blob"] = blob
    return out


@pytest.mark.parametrize("shape", [(37, 53), (1, 9), (9, 1)])
@pytest.mark.parametrize("F", [1, 2, 3, 8, 64])
def test_separable_distance_is_the_brute_force_distance(shape, F):
    for name, C in _masks(*shape, seed=F).items():
        brute = fs.distance_brute(C, F)
        assert np.array_equal(fs.distance_separable(C, F), brute), name
        assert brute.max() <= F and not brute[C == 0].any() and (brute[C != 0] >= 1).all(), name


def test_distance_has_no_ramp_along_the_frame_border():
    C = np.zeros((12, 10), np.uint8)
    C[6:, :] = 1                                                   # a band that touches the bottom, left and right edges
    d = fs.distance_brute(C, 4)
    assert np.array_equal(d[:, 0], d[:, 5]) and d[11].tolist() == [4] * 10 and d[6].tolist() == [1] * 10
    assert (fs.distance_brute(np.ones((5, 7), np.uint8), 3) == 3).all()      # no zero anywhere: the fill everywhere


@pytest.mark.parametrize("F", [1, 2, 7, 64])
def test_blend_identity_and_range(F):
    a, b = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    fill = np.repeat(a[..., None], 3, axis=2)                      # all 256^2 (fill, src) pairs, as a 256 x 256 "frame"
    src = np.repeat(b[..., None], 3, axis=2)
    for d in range(F + 1):
        dd = np.full((256, 256), d, np.uint8)
        out = fs.blend(fill, src, dd, F).astype(np.int64)          # (blend asserts 0..255 itself before the cast)
        assert (out >= np.minimum(fill, src)).all() and (out <= np.maximum(fill, src)).all()
        assert np.array_equal(fs.blend(src, src, dd, F), src), "fill == src gives src for every d"
        if d == 0:
            assert np.array_equal(out, src)
        if d == F:
            assert np.array_equal(out, fill)


def test_f1_is_the_hard_composite():
    rng = np.random.default_rng(5)
    fill, src = rng.integers(0, 256, (2, 9, 11, 3), dtype=np.uint8), rng.integers(0, 256, (2, 9, 11, 3), dtype=np.uint8)
    C = (rng.random((9, 11)) < 0.5).astype(np.uint8)
    assert np.array_equal(fs.composite(fill, src, C, 1), np.where(C[None, :, :, None] != 0, fill, src))


def test_composite_masks_mirror_the_plugins():
    """the statement's C against the arithmetic of each plugin's composite_mask, without building an engine"""
    from vsr_amd.backend.inpaint.lama_inpaint import LamaInpaint
    from vsr_amd.backend.inpaint.opencv_inpaint import OpenCVInpaint
    from vsr_amd.backend.inpaint.propainter_inpaint import PropainterInpaint
    from vsr_amd.backend.inpaint.sttn_auto_inpaint import STTNInpaint
    from vsr_amd.backend.inpaint.sttn_det_inpaint import STTNDetInpaint

    H, W = 480, 852
    M = np.zeros((H, W), np.uint8)
    M[300:340, 100:700] = 255
    M[89:91, 10:60] = 255              # the 4-fold dilation of this one reaches its strip's first row
    M[200:204, 30:50] = 100            # under sttn-auto's threshold
    for cls, mode in ((STTNDetInpaint, "sttn-det"), (LamaInpaint, "lama"), (OpenCVInpaint, "opencv"), (STTNInpaint, "sttn-auto")):
        assert np.array_equal(cls.composite_mask(object.__new__(cls), M), fs.composite_mask(mode, M)), mode
    pp = object.__new__(PropainterInpaint)
    pp.mask_dilation = 4
    got = PropainterInpaint.composite_mask(pp, M)
    assert np.array_equal(got, fs.composite_mask("propainter", M))
    assert got[M != 0].all() and got.sum() > (M != 0).sum()
    assert not fs.composite_mask("sttn-auto", M)[200:204].any() and fs.composite_mask("sttn-det", M)[200:204, 30:50].all()


def test_option_parsing(monkeypatch):
    from vsr_amd.backend.tools import seam_feather as sf
    from vsr_amd.backend.tools.args_handler import parse_args

    assert sf.feather_option(env={}) == 0 and sf.feather_option(env={"VSR_SEAM_FEATHER": ""}) == 0
    assert sf.feather_option(env={"VSR_SEAM_FEATHER": "8"}) == 8 and sf.feather_option(64, env={}) == 64
    assert sf.feather_option(3, env={"VSR_SEAM_FEATHER": "9"}) == 3, "an argument wins over the environment"
    for bad in ("-1", "65", "x", "1.5"):
        with pytest.raises(ValueError, match="seam feather"):
            sf.feather_option(env={"VSR_SEAM_FEATHER": bad})
    for bad in (-1, 65, 1.5):
        with pytest.raises(ValueError, match="seam feather"):
            sf.feather_option(bad)
    monkeypatch.setenv("VSR_SEAM_FEATHER", "5")
    assert sf.feather_option() == 5
    assert parse_args(["-i", "x.y4m"]).seam_feather is None
    assert parse_args(["-i", "x.y4m", "--seam-feather", "8"]).seam_feather == 8
    for bad in ("65", "-1"):
        with pytest.raises(SystemExit):
            parse_args(["-i", "x.y4m", "--seam-feather", bad])


def test_flag_sets_the_environment_variable(monkeypatch):
    from vsr_amd.backend import main as m

    seen = {}

    class Stop(Exception):
        pass

    def fake_remover(path):
        import os

        seen["env"] = os.environ.get("VSR_SEAM_FEATHER")
        raise Stop

    monkeypatch.setenv("VSR_SEAM_FEATHER", "0")
    monkeypatch.setattr(m, "SubtitleRemover", fake_remover)
    with pytest.raises(Stop):
        m.main(["-i", "x.y4m", "--seam-feather", "8"])
    assert seen["env"] == "8"


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
    from vsr_amd.backend.tools import seam_feather as sf
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
    monkeypatch.setenv("VSR_SEAM_FEATHER", "8")
    with pytest.raises(RuntimeError, match="one process"):
        call()
    monkeypatch.setenv("VSR_SEAM_FEATHER", "65")
    with pytest.raises(ValueError, match="seam feather"):
        call()
    # off, or one rank: nothing is refused
    assert sf.refuse_ranks(FakeDist, 0) == 0 and sf.refuse_ranks(None, 8) == 8
