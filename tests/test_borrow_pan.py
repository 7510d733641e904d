"""--borrow-pan without a GPU: the statement (tests/_borrow_pan_statement.py) follows a pan on a worked clip where the plain pass
(tests/_borrow_statement.py) borrows nothing, refuses a pan that the ring cannot see, and keeps the properties that follow from its
definition; the option is parsed in one place; P > 0 without B, bad values and several ranks are refused before any frame is read;
borrow.apply takes the new entry points for P > 0 only; the entry points refuse bad arguments."""
import contextlib
import ctypes as C
import types

import numpy as np
import pytest

from tests import _borrow_pan_statement as ps
from tests import _borrow_statement as bs

T = 12
H, W, BOX = 64, 150, (20, 48, 12, 138)
ROWS = (0, H)


def canvas(h, w):
    """smooth and textured: a shift by a few pixels moves every sample by many levels, Immerkaer's operator sees next to nothing"""
    y, x = np.mgrid[0:h, 0:w]
    return 128 + 40 * np.sin(2 * np.pi * x / 23.0) + 30 * np.sin(2 * np.pi * y / 29.0 + x / 7.0)       # (periods beyond 2 P + 1)


def panned(seed=0, n=6, step=(0, 3), sigma=2.0, glyph=True):
    """n frames of 64 x 150 cut from a larger canvas: what frame t shows at p, frame t + k shows at p + k step; independent grain per
    frame; the fill is the picture behind with another draw of the grain inside the box mask; a 5 x 7 block of +100 at rows 30..34,
    columns 40..46 on the first half and at columns 100..106 on the second"""
    rng = np.random.default_rng(seed)
    Cm = np.zeros((H, W), np.uint8)
    Cm[BOX[0]:BOX[1], BOX[2]:BOX[3]] = 255
    big = canvas(H + 2 * 80, W + 2 * 80)
    clean = np.stack([big[80 - t * step[0]:80 - t * step[0] + H, 80 - t * step[1]:80 - t * step[1] + W] for t in range(n)])[..., None]
    clean = clean + np.zeros((1, 1, 1, 3))
    src = np.rint(clean + rng.normal(0, sigma, clean.shape))
    other = np.clip(np.rint(clean + rng.normal(0, sigma, clean.shape)), 0, 255).astype(np.uint8)
    if glyph:
        src[:n // 2, 30:35, 40:47] += 100
        src[n // 2:, 30:35, 100:107] += 100
    src = np.clip(src, 0, 255).astype(np.uint8)
    fill = src.copy()
    fill[:, Cm != 0] = other[:, Cm != 0]
    return fill, src, Cm


def glyph_of(t, n=6):
    block = np.zeros((H, W), bool)
    block[30:35, (slice(40, 47) if t < n // 2 else slice(100, 107))] = True
    return block


def test_constants():
    assert ps.MAX_PAN == 8 and ps.slots(1) == 10 and ps.slots(2) == 25 and ps.slots(8) == 289
    assert ps.candidates(1, 1) == [(-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 0), (0, 1), (1, -1), (1, 0), (1, 1)]
    assert ps.candidates(2, 4, (0, 6))[:3] == [(-1, 5), (-1, 6), (-1, 7)] and ps.candidates(2, 4, (0, 6))[9] == (0, 0)
    assert ps.candidates(2, 4, (0, 8))[2] is None, "beyond k P"
    assert ps.candidates(2, 4, (0, 1))[3] is None, "(0,0) stands once, in the last slot"
    assert sorted([(1, 1), (0, -1), (0, 0), (-1, 0), (0, 1), (1, 0), (0, 2)], key=ps.order) == \
        [(0, 0), (-1, 0), (0, -1), (0, 1), (1, 0), (1, 1), (0, 2)]
    # d beats e iff S_d cnt(e) < S_e cnt(d); a tie goes to the earlier
    assert ps.raw_best([(0, 0), (0, 1)], [10, 10], [5, 5], 6) == (0, 0) and ps.raw_best([(0, 0), (0, 1)], [10, 19], [5, 10], 6) == (0, 1)
    assert ps.raw_best([(0, 0), (0, 1)], [10, 0], [5, 2], 6) == (0, 0), "2 cnt < |E|: not eligible"
    assert ps.raw_best([(0, 0)], [0], [0], 0) == (0, 0)
    assert ps.weight(75, 10, 0, 0, 10) == bs.pair_weight(75, 0, 0, 30) == 8 and ps.weight(0, 0, 0, 0, 10) == 0
    assert ps.workspace_bytes(9, 65, 3, 2, 1) == 8 * (3 * 2 * 11 * 2 + 6) + 2 * 3 * 9 * 2 * 8


@pytest.mark.parametrize("seed", [0, 1])
def test_the_worked_clip(seed):
    fill, src, Cm = panned(seed)
    plain = {}
    assert np.array_equal(bs.borrow(fill, src, Cm, ROWS, T, 3, info=plain), fill), "the plain pass borrows nothing"
    assert set(plain["b"].values()) == {0}, "every pair is closed"
    info = {}
    out = ps.borrow_pan(fill, src, Cm, ROWS, T, 3, 4, info=info)
    assert all(info["R"][(t, k)] == (0, 3 * k) for (t, k) in info["R"]) and len(info["R"]) == 5 + 4 + 3
    assert info["D"] == info["R"] and min(info["w"].values()) >= 14 and set(info["b0"].values()) == {0}
    lender, q, borrowers = info["lender"], info["q"], info["borrowers"]
    assert borrowers.any(axis=(1, 2)).all() and (lender[borrowers] >= 0).all(), "the mask keeps every q inside the frame: all are borrowed"
    for t in range(6):
        assert (borrowers[t] & glyph_of(t)).sum() == 35
        for y, x in np.argwhere(lender[t] >= 0):
            s, (qy, qx) = lender[t, y, x], q[t, y, x]
            assert (qy, qx) == (y, x + 3 * (s - t)) and not glyph_of(s)[qy, qx] and not (info["N"][s, qy, qx] and Cm[qy, qx])
            assert np.array_equal(out[t, y, x], src[s, qy, qx])
    assert np.array_equal(out[:, Cm == 0], fill[:, Cm == 0]), "nothing outside C is written"
    assert np.abs(out.astype(int) - fill).max() < 24
    # the table: level 1 holds every shift within P, the later levels the centre's neighbours and (0,0)
    assert info["S"].shape == info["cnt"].shape == (6, 3, 81)
    assert info["cnt"][0, 0, 4 * 9 + 4] == info["m"] // 3 and info["cands"][(0, 3)][4] == (0, 9) and info["cands"][(0, 3)][9] == (0, 0)
    assert (info["cnt"][5] == 0).all() and (info["cnt"][4, 1:] == 0).all()


def test_a_pan_the_ring_cannot_see_closes_the_pair():
    """8 rows per frame downwards: at k = 2 the true shift (16, 0) moves the ring above the mask into it and the ring below off the
    frame; fewer than half of E's samples have a valid target, so the shift is not eligible and the pair stays closed"""
    fill, src, Cm = panned(3, n=4, step=(8, 0))
    info = {}
    out = ps.borrow_pan(fill, src, Cm, ROWS, T, 2, 8, info=info)
    n_e = info["m"] // 3
    for t in range(2):
        cs = info["cands"][(t, 2)]
        i = cs.index((16, 0))
        assert info["R"][(t, 1)] == (8, 0) and 0 < 2 * info["cnt"][t, 1, i] < n_e
        per = info["S"][t, 1, i] / (3 * info["cnt"][t, 1, i])
        assert per < 3, "the samples that are left agree: it is the rule that closes the pair, not the picture"
        assert info["R"][(t, 2)] == (0, 0) and info["D"][(t, 2)] == (0, 0) and info["w"][(t, 2)] == 0
    assert (np.abs(info["lender"] - np.arange(4)[:, None, None])[info["lender"] >= 0] == 1).all(), "nothing is lent two frames away"
    assert np.array_equal(out[:, Cm == 0], fill[:, Cm == 0])


def test_properties():
    fill, src, Cm = panned(5)
    keep = src.copy()
    assert np.array_equal(ps.borrow_pan(fill, src, Cm, ROWS, T, 3, 0), bs.borrow(fill, src, Cm, ROWS, T, 3)), "P = 0 is the plain pass"
    assert np.array_equal(ps.borrow_pan(src.copy(), src, Cm, ROWS, T, 3, 4), src), "fill == src is a fixed point"
    out = ps.borrow_pan(fill, src, Cm, ROWS, T, 3, 4)
    assert np.array_equal(src, keep), "src is never written"
    assert np.array_equal(out[:, Cm == 0], fill[:, Cm == 0]) and np.abs(out.astype(int) - fill).max() < 24 and (out != fill).any()
    assert np.array_equal(ps.borrow_pan(fill[:1], src[:1], Cm, ROWS, T, 3, 4), fill[:1])
    # a still clip: every pair has b_0 = 16 and any P gives the plain pass's bytes
    sfill, ssrc, _ = panned(6, step=(0, 0))
    plain, info = {}, {}
    want = bs.borrow(sfill, ssrc, Cm, ROWS, T, 3, info=plain)
    assert set(plain["b"].values()) == {16} and (want != sfill).any()
    for P in (1, 4, 8):
        assert np.array_equal(ps.borrow_pan(sfill, ssrc, Cm, ROWS, T, 3, P, info=info), want), P
        assert set(info["D"].values()) == {(0, 0)} and info["w"] == plain["b"]
    # a cut between frames 2 and 3 lends nothing across it: the two sides equal the statement run on each alone
    cut_src, cut_fill = src.copy(), fill.copy()
    cut_src[3:] = 255 - cut_src[3:, ::-1]
    cut_fill[3:] = 255 - cut_fill[3:, ::-1]
    info = {}
    out = ps.borrow_pan(cut_fill, cut_src, Cm, ROWS, T, 3, 4, info=info)
    assert all(v == 0 for (t, k), v in info["w"].items() if t < 3 <= t + k)
    lender = info["lender"]
    assert not (lender[:3] >= 3).any() and not ((lender[3:] >= 0) & (lender[3:] < 3)).any()
    assert np.array_equal(out[:3], ps.borrow_pan(cut_fill[:3], cut_src[:3], Cm, ROWS, T, 3, 4))
    assert np.array_equal(out[3:], ps.borrow_pan(cut_fill[3:], cut_src[3:], Cm, ROWS, T, 3, 4))


def test_strip_rows_state_their_own_rows():
    """the rows held bound V and q: a strip is its own picture, and a horizontal pan inside it borrows as the full frame does"""
    fill, src, Cm = panned(7)
    rows = (2, 62)
    full = ps.borrow_pan(fill, src, Cm, rows, T, 3, 4)
    strip = ps.borrow_pan(fill[:, 2:62], src[:, 2:62], Cm, rows, T, 3, 4, y0=2)
    assert np.array_equal(strip, full[:, 2:62]) and not np.array_equal(full, fill)


# ---- options and ranks ------------------------------------------------------------------------------------------------------------------
FOUR = ("VSR_SEAM_FEATHER", "VSR_REGRAIN", "VSR_DEFLICKER", "VSR_TONE_MATCH")


def test_option_parsing():
    from vsr_amd.backend import main as m
    from vsr_amd.backend.tools import borrow as bw
    from vsr_amd.backend.tools.args_handler import parse_args

    assert bw.MAX_PAN == ps.MAX_PAN and bw.PAN_ENV == "VSR_BORROW_PAN"
    assert bw.pan_option(env={}) == 0 and bw.pan_option(env={"VSR_BORROW_PAN": ""}) == 0
    assert bw.pan_option(env={"VSR_BORROW_PAN": "3"}) == 3 and bw.pan_option(8, env={}) == 8
    assert bw.pan_option(2, env={"VSR_BORROW_PAN": "5"}) == 2, "an argument wins over the environment"
    for bad in ("-1", "9", "x", "1.5"):
        with pytest.raises(ValueError, match="borrow-pan"):
            bw.pan_option(env={"VSR_BORROW_PAN": bad})
    for bad in (-1, 9, 1.5):
        with pytest.raises(ValueError, match="borrow-pan"):
            bw.pan_option(bad)
    assert parse_args(["-i", "x.y4m"]).borrow_pan is None
    assert parse_args(["-i", "x.y4m", "--glyph-key", "12", "--borrow", "2", "--borrow-pan", "4"]).borrow_pan == 4
    assert parse_args(["-i", "x.y4m", "--borrow-pan", "0"]).borrow_pan == 0
    for bad in (["--borrow-pan", "4"], ["--glyph-key", "12", "--borrow-pan", "4"], ["--glyph-key", "12", "--borrow", "2", "--borrow-pan", "9"],
                ["--glyph-key", "12", "--borrow", "2", "--borrow-pan", "-1"]):
        with pytest.raises(SystemExit):
            parse_args(["-i", "x.y4m"] + bad)
    assert ("borrow_pan", "VSR_BORROW_PAN", str) in m.FLAG_ENV


def test_flag_sets_the_environment_variable(monkeypatch):
    import os

    from vsr_amd.backend import main as m

    seen = {}

    class Stop(Exception):
        pass

    def fake_remover(path):
        seen["env"] = os.environ.get("VSR_BORROW_PAN")
        raise Stop

    for name in ("VSR_BORROW", "VSR_GLYPH_KEY", "VSR_BORROW_PAN"):
        monkeypatch.setenv(name, "0")
    monkeypatch.setattr(m, "SubtitleRemover", fake_remover)
    with pytest.raises(Stop):
        m.main(["-i", "x.y4m", "--glyph-key", "12", "--borrow", "2", "--borrow-pan", "4"])
    assert seen["env"] == "4"


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


def test_options_and_refusals_keep_their_signatures(monkeypatch):
    from vsr_amd.backend.tools import borrow as bw
    from vsr_amd.backend.tools import seam_feather as sf

    for name, value in zip(FOUR + ("VSR_GLYPH_KEY", "VSR_BORROW", "VSR_BORROW_PAN"), ("3", "150", "2", "60", "12", "2", "4")):
        monkeypatch.setenv(name, value)
    assert sf.options() == (3, 150, 2, 60) and sf.refuse_ranks_all(None) == (3, 150, 2, 60)
    monkeypatch.setenv("VSR_BORROW", "0")
    with pytest.raises(ValueError, match="--borrow-pan .* --borrow"):
        sf.refuse_ranks_all(None)
    monkeypatch.setenv("VSR_BORROW", "2")
    monkeypatch.setenv("VSR_BORROW_PAN", "9")
    with pytest.raises(ValueError, match="borrow-pan"):
        sf.refuse_ranks_all(None)
    with pytest.raises(RuntimeError, match="--borrow-pan .* one process"):
        bw.refuse_ranks(FakeDist, 2, 12, 4)
    assert bw.refuse_ranks(None, 2, 12, 4) == 2 and bw.refuse_ranks(FakeDist, 0, 0, 0) == 0


@pytest.mark.parametrize("entry", ["run", "video_inpaint", "propainter_mode"])
def test_refusals_before_a_frame_is_read(monkeypatch, entry):
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
    monkeypatch.setenv("VSR_GLYPH_KEY", "12")
    monkeypatch.setenv("VSR_BORROW", "0")
    monkeypatch.setenv("VSR_BORROW_PAN", "4")
    with pytest.raises(ValueError, match="--borrow-pan .* --borrow"):
        call()
    monkeypatch.setenv("VSR_BORROW", "2")
    monkeypatch.setenv("VSR_BORROW_PAN", "9")
    with pytest.raises(ValueError, match="borrow-pan"):
        call()
    monkeypatch.setenv("VSR_BORROW_PAN", "4")
    monkeypatch.setattr(sr, "_distributed", lambda: FakeDist)
    with pytest.raises(RuntimeError, match="one process"):            # (the key's own refusal comes first: it is on too)
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
    monkeypatch.setenv("VSR_GLYPH_KEY", "12")
    monkeypatch.setenv("VSR_BORROW", "0")
    monkeypatch.setenv("VSR_BORROW_PAN", "4")
    with pytest.raises(ValueError, match="--borrow-pan .* --borrow"):
        auto._run(None, None, None, None)
    monkeypatch.setenv("VSR_BORROW", "2")
    with pytest.raises(RuntimeError, match="one process"):
        auto._run(FakeDist, None, None, None)
    monkeypatch.setenv("VSR_BORROW_PAN", "x")
    with pytest.raises(ValueError, match="borrow-pan"):
        auto._run(None, None, None, None)


# ---- borrow.apply: which entry points a call reaches --------------------------------------------------------------------------------------
class Tensor:
    """what borrow.apply asks of a tensor"""
    is_cuda, device = True, "gpu"

    def __init__(self, shape, dtype):
        self.shape, self.dtype = tuple(shape), dtype

    def stride(self, i):
        return int(np.prod(self.shape[i + 1:]))

    def data_ptr(self):
        return 4096

    def record_stream(self, stream):
        pass


class Library:
    def __init__(self, log):
        self.log = log

    def __getattr__(self, name):
        def call(*args):
            self.log.append((name, args))
            return 1 << 12 if name.endswith("workspace_bytes") else 0
        return call


@pytest.mark.parametrize("pan", [None, "0", "4"])
def test_apply_takes_the_new_path_only_for_p_above_zero(monkeypatch, pan):
    import torch

    import vsr_amd._lib as _lib
    from vsr_amd.backend.tools import borrow as bw

    log = []
    monkeypatch.setattr(_lib, "lib", Library(log))
    monkeypatch.setattr(_lib, "check", lambda rc: rc)
    monkeypatch.setattr(torch.cuda, "device", lambda device: contextlib.nullcontext())
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: types.SimpleNamespace(cuda_stream=0))
    monkeypatch.setattr(torch, "empty", lambda shape, dtype=None, device=None: Tensor(shape if isinstance(shape, tuple) else (shape,), dtype))
    monkeypatch.delenv("VSR_BORROW_PAN", raising=False)
    if pan is not None:
        monkeypatch.setenv("VSR_BORROW_PAN", pan)
    n, h, Wd = 5, 20, 64
    frames, src = Tensor((n, h, Wd, 3), torch.uint8), Tensor((n, h, Wd, 3), torch.uint8)
    sets = types.SimpleNamespace(map=Tensor((h, Wd), torch.uint8), counts=Tensor((2,), torch.int64), c0=6, c1=14)
    mask = types.SimpleNamespace(c=Tensor((h, Wd), torch.uint8), c0=6, c1=14)
    calls = dict(bw.stats)
    assert bw.apply(frames, src, sets, mask, T, 3) is frames
    names = [name for name, _ in log]
    if pan == "4":
        assert names == ["vsr_borrow_pan_workspace_bytes", "vsr_regrain_measure", "vsr_borrow_pan_search", "vsr_borrow_pan_apply"]
        assert log[0][1] == (h, Wd, n, 3, 4)
        search, apply = log[2][1], log[3][1]
        assert search[4:13] == (n, h, Wd, 0, h, 6, 14, 3, 4) and apply[7:17] == (n, h, Wd, 0, h, 6, 14, T, 3, 4)
        assert bw.stats["pan_calls"] == calls["pan_calls"] + 1
    else:
        assert names == ["vsr_borrow_workspace_bytes", "vsr_regrain_measure", "vsr_deflicker_pairs", "vsr_borrow_apply"], \
            "P = 0: the calls of before"
        assert log[0][1] == (h, Wd, n) and bw.stats["pan_calls"] == calls["pan_calls"]
    assert bw.stats["calls"] == calls["calls"] + 1


# ---- the entry points without a device ------------------------------------------------------------------------------------------------
def test_argument_errors_then_no_gpu(built_lib):
    lib = built_lib.lib
    buf = (C.c_uint8 * 4096)()
    words = (C.c_uint64 * 4096)()
    p, q = C.cast(buf, C.c_void_p), C.cast(words, C.c_void_p)
    size = 8 * 8 * 3
    ok = dict(frames=p, fs=size, src=p, ss=size, cm=p, map=p, counts=q, stats=q, n=2, H=8, W=8, y0=0, rows=8, c0=2, c1=6, T=T, B=2, P=1, work=q)

    def apply(**kw):
        a = dict(ok, **kw)
        return lib.vsr_borrow_pan_apply(a["frames"], a["fs"], a["src"], a["ss"], a["cm"], a["counts"], a["stats"], a["n"], a["H"], a["W"],
                                        a["y0"], a["rows"], a["c0"], a["c1"], a["T"], a["B"], a["P"], a["work"], None)

    def search(**kw):
        a = dict(ok, **kw)
        return lib.vsr_borrow_pan_search(a["src"], a["ss"], a["map"], a["counts"], a["n"], a["H"], a["W"], a["y0"], a["rows"], a["c0"],
                                         a["c1"], a["B"], a["P"], a["work"], None)

    shared = (dict(src=None), dict(counts=None), dict(work=None), dict(H=0), dict(W=-1), dict(n=-1), dict(ss=size - 1), dict(y0=1),
              dict(rows=9), dict(rows=0), dict(c0=-1), dict(c0=7, c1=6), dict(c1=9), dict(H=32768, W=32768, rows=1), dict(B=0), dict(B=9),
              dict(P=0), dict(P=-1), dict(P=9), dict(work=C.c_void_p(q.value + 4)))
    for kw in shared + (dict(frames=None), dict(cm=None), dict(stats=None), dict(fs=size - 1), dict(T=0), dict(T=129)):
        assert apply(**kw) == built_lib.VSR_ERR_ARG, kw
        assert "borrow-pan" in built_lib.last_error(), kw
    for kw in shared + (dict(map=None),):
        assert search(**kw) == built_lib.VSR_ERR_ARG, kw
        assert "borrow-pan" in built_lib.last_error(), kw
    for args in ((0, 8, 1, 2, 1), (8, -1, 1, 2, 1), (8, 8, -1, 2, 1), (32768, 32768, 1, 2, 1), (8, 8, 1, 0, 1), (8, 8, 1, 9, 1),
                 (8, 8, 1, 2, 0), (8, 8, 1, 2, 9)):
        assert lib.vsr_borrow_pan_workspace_bytes(*args) == built_lib.VSR_ERR_ARG, args
        assert "borrow-pan" in built_lib.last_error(), args
    for args in ((9, 65, 3, 2, 1), (1080, 1920, 50, 8, 8), (45, 75, 17, 8, 3)):
        assert lib.vsr_borrow_pan_workspace_bytes(*args) == ps.workspace_bytes(*args), args
    assert apply(n=1) == 0 and apply(c0=3, c1=3) == 0 and search(n=1) == 0 and search(c0=3, c1=3) == 0, \
        "nothing to do is success without a launch"
    if lib.vsr_device_count() <= 0:
        assert apply() == built_lib.VSR_ERR_NOGPU and search() == built_lib.VSR_ERR_NOGPU
