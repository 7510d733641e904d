"""--logo-scan on the MI355X: the two kernels of csrc/static_kernels.hip against tests/_static_statement.py bit for
bit, find_areas over a resident clip and over its own reading pass, and a whole run that finds a logo no text detector sees."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from tests import _static_statement as ss

pytestmark = pytest.mark.gpu

SHAPES = [(37, 61), (64, 64), (70, 130), (33, 257)]       # no multiple of the 32 x 64 tile; a tile seam in each direction; all four borders
COUNTS = (1, 2, 17)
SLACK = 5                                                  # bytes between two frames: every frame at another alignment


def p(t):
    return C.c_void_p(t.data_ptr())


def random_frames(H, W, k, seed):
    """colour noise whose amplitude changes from frame to frame and from left to right: the gradient passes GE in some frames and not in
    others, so e takes many values, and lo and hi are spread over the whole range"""
    rng = np.random.default_rng(seed)
    amp = rng.integers(8, 256, size=(k, 1, 1, 1)) * np.linspace(0.05, 1.0, W)[None, None, :, None]
    base = rng.integers(0, 200, size=(1, 1, 1, 3))
    return np.clip(base + rng.random((k, H, W, 3)) * amp, 0, 255).astype(np.uint8)


class Case:
    """one shape: 19 frames on the device `SLACK` bytes apart, and per n of COUNTS the n frames a call takes and the statement's planes"""

    def __init__(self, H, W, device):
        self.H, self.W, self.K = H, W, 19
        self.host = random_frames(H, W, self.K, seed=H * 1000 + W)
        self.stride = H * W * 3 + SLACK
        flat = np.zeros(self.K * self.stride, np.uint8)
        for f in range(self.K):
            flat[f * self.stride:f * self.stride + H * W * 3] = self.host[f].ravel()
        self.dev = torch.from_numpy(flat).to(device)
        order = np.random.default_rng(7).permutation(self.K)
        self.idx = {n: [int(i) for i in order[:n]] for n in COUNTS}
        self.want = {n: ss.accumulate(self.host[i] for i in self.idx[n]) for n in COUNTS}


@pytest.fixture(scope="module")
def cases(built_lib, gpu_device):
    return {shape: Case(*shape, gpu_device) for shape in SHAPES}


def planes(H, W, device):
    return (torch.full((H, W), 7, dtype=torch.uint8, device=device), torch.full((H, W), 9, dtype=torch.uint8, device=device),
            torch.full((H, W), 11, dtype=torch.int16, device=device))


def accum(lib, case, idx, first, state):
    from vsr_amd._lib import check

    idx_dev = torch.tensor(idx, dtype=torch.int32, device=case.dev.device)
    check(lib.vsr_static_accum(p(case.dev), case.stride, p(idx_dev), len(idx), case.H, case.W, ss.GE, first, p(state[0]), p(state[1]), p(state[2]), None))
    torch.cuda.synchronize()


def host_planes(state):
    return (state[0].cpu().numpy().astype(np.int64), state[1].cpu().numpy().astype(np.int64),
            state[2].cpu().numpy().view(np.uint16).astype(np.int64))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_accumulate_equals_the_statement(built_lib, gpu_device, cases, shape):
    case = cases[shape]
    for n in COUNTS:
        state = planes(case.H, case.W, gpu_device)                       # (first = 1 overwrites whatever the planes held)
        accum(built_lib.lib, case, case.idx[n], 1, state)
        got, want = host_planes(state), case.want[n]
        for name, g, w in zip(("lo", "hi", "e"), got, want):
            assert np.array_equal(g, w), f"{name} at n = {n}: {np.argwhere(g != w)[:4].tolist()}"
    lo, hi, e = case.want[17]
    assert len(np.unique(e)) > 6 and e.min() < 17 and e.max() > 0 and (hi - lo).min() < ss.MV < (hi - lo).max(), "the frames exercise the planes"


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_classify_equals_the_statement(built_lib, gpu_device, cases, shape):
    from vsr_amd._lib import check

    case = cases[shape]
    H, W = case.H, case.W
    lo, hi, e = case.want[17]
    state = (torch.from_numpy(lo.astype(np.uint8)).to(gpu_device), torch.from_numpy(hi.astype(np.uint8)).to(gpu_device),
             torch.from_numpy(e.astype(np.uint16).view(np.int16)).to(gpu_device))
    occurs = int(np.median(e))
    assert (e == occurs).any() and (e == e.max()).any()
    seeds = []
    for need in (occurs, occurs + 1, int(e.max()), int(e.max()) + 1):    # an e that occurs and one more than it; the last seed and none
        grown = torch.full((H, W), 0.5, dtype=torch.float32, device=gpu_device)
        moving = torch.full((H, W), 3, dtype=torch.uint8, device=gpu_device)
        check(built_lib.lib.vsr_static_classify(p(state[0]), p(state[1]), p(state[2]), H, W, need, ss.MV, ss.D, p(grown), p(moving), None))
        torch.cuda.synchronize()
        want_grown, want_moving = ss.classify(lo, hi, e, need)
        g = grown.cpu().numpy()
        assert set(np.unique(g).tolist()) <= {0.0, 1.0} and np.array_equal(g == 1.0, want_grown), f"grown at need = {need}"
        assert np.array_equal(moving.cpu().numpy(), want_moving.astype(np.uint8)), f"moving at need = {need}"
        seeds.append(int((e >= need).sum()))
    assert seeds[0] > seeds[1] and seeds[2] > 0 and seeds[3] == 0
    assert not ss.classify(lo, hi, e, int(e.max()))[0].all(), "the sparse seeds leave pixels no dilation reaches"


def test_two_calls_equal_one(built_lib, gpu_device, cases):
    case = cases[(70, 130)]
    state = planes(case.H, case.W, gpu_device)
    accum(built_lib.lib, case, case.idx[17][:9], 1, state)
    accum(built_lib.lib, case, case.idx[17][9:], 0, state)
    for g, w in zip(host_planes(state), case.want[17]):
        assert np.array_equal(g, w)


# ---- find_areas ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def logo_clip():
    clip = ss.clip_logo()
    assert ss.areas(clip) == [ss.LOGO_AREA]
    return clip


def write_y4m(path, clip):
    from vsr_amd.backend.tools import video_io

    w = video_io.Y4mWriter(str(path), 25.0, (clip.shape[2], clip.shape[1]), chroma="444")
    for f in clip:
        w.write(f)
    w.release()
    return str(path)


def test_find_areas_on_a_resident_clip(built_lib, gpu_device, logo_clip):
    from vsr_amd.backend.tools import logo_scan as ls

    before = dict(ls.stats)
    resident = types.SimpleNamespace(frames=torch.from_numpy(logo_clip).to(gpu_device), windowed=False)
    assert ls.find_areas(None, clip=resident) == [ss.LOGO_AREA]
    assert ls.stats["accum_launches"] == before["accum_launches"] + 1, "the frames are read where they are, in one launch"
    assert ls.stats["frames"] == before["frames"] + len(logo_clip) and ls.stats["scans"] == before["scans"] + 1
    assert ls.stats["areas"] == before["areas"] + 1 and ls.stats["dropped"] == before["dropped"]
    # the still wave: the same component, nothing around it moves
    still = types.SimpleNamespace(frames=torch.from_numpy(ss.clip_still_logo()).to(gpu_device), windowed=False)
    assert ls.find_areas(None, clip=still) == []
    with pytest.raises(ValueError, match="at least 16"):
        ls.find_areas(None, clip=types.SimpleNamespace(frames=resident.frames[:15], windowed=False))


def test_find_areas_through_the_reading_pass(built_lib, gpu_device, logo_clip, tmp_path):
    from vsr_amd.backend.tools import logo_scan as ls
    from vsr_amd.backend.tools.video_io import ArrayVideo

    before = dict(ls.stats)
    path = write_y4m(tmp_path / "logo.y4m", logo_clip)
    assert ls.find_areas(path, device=0) == [ss.LOGO_AREA]
    batches = -(-len(logo_clip) // ls.BATCH_FRAMES)
    assert batches > 1 and ls.stats["accum_launches"] == before["accum_launches"] + batches, "uploaded in batches, continued with first = 0"
    assert ls.find_areas(ArrayVideo(logo_clip, fps=25.0), device=0) == [ss.LOGO_AREA], "host frames"


# ---- a whole run ----------------------------------------------------------------------------------------------------------------------------
class NoText:
    def predict(self, img):
        return [{"dt_polys": np.zeros((0, 4, 2), np.int32)}]


def records(path, n):
    """the stored samples of a 4:4:4 8-bit *.y4m: uint8 [n,3,H,W] (Y, U, V)"""
    from vsr_amd.backend.tools import video_io

    r = video_io.Y4mVideo(path)
    rec = np.empty((n, r._fsize), np.uint8)
    assert r.read_planes_into(rec) == n
    r.release()
    return rec.reshape(n, 3, r.h, r.w)


def test_a_run_removes_a_logo_no_detector_sees(built_lib, gpu_device, logo_clip, tmp_path, monkeypatch):
    """*.y4m in -> SubtitleRemover.run() in opencv mode (no weights) with a text detector that finds nothing.  With --logo-scan the run
    succeeds: the written file keeps every sample of the source outside the pixels the mode masks for the area (create_mask: the area
    grown by the mask margin of every mode, config.subtitleAreaDeviationPixel), and inside the area no pixel of any frame keeps the
    logo's white.  Without the flag the same run finds nothing to do, as it does today."""
    from vsr_amd.backend.config import config
    from vsr_amd.backend.inpaint.opencv_inpaint import OpenCVInpaint
    from vsr_amd.backend.main import SubtitleRemover
    from vsr_amd.backend.tools import logo_scan as ls
    from vsr_amd.backend.tools.constant import InpaintMode
    from vsr_amd.backend.tools.inpaint_tools import create_mask

    n, H, W = len(logo_clip), ss.CLIP_H, ss.CLIP_W
    src = write_y4m(tmp_path / "in.y4m", logo_clip)
    monkeypatch.setenv("VSR_Y4M_OUT", "source")
    monkeypatch.delenv("VSR_OPENCV_BACKEND", raising=False)
    for name in ("VSR_SEAM_FEATHER", "VSR_REGRAIN", "VSR_DEFLICKER", "VSR_TONE_MATCH", "VSR_GLYPH_KEY", "VSR_GLYPH_HOLD"):
        monkeypatch.delenv(name, raising=False)
    old_mode = config.inpaintMode.value
    plugin = OpenCVInpaint("cuda:0")
    try:
        config.inpaintMode.value = InpaintMode.OPENCV
        monkeypatch.setenv("VSR_LOGO_SCAN", "1")
        said = []
        sr = SubtitleRemover(src, device="cuda:0")
        sr.text_detector, sr.opencv_inpaint = NoText(), plugin
        sr.append_output = lambda *a: said.append(" ".join(str(x) for x in a))
        sr.video_out_path = str(tmp_path / "out.y4m")
        sr.run()
        assert sr.isFinished and sr.static_areas == [ss.LOGO_AREA] and sr.phase_seconds["logo scan"] > 0
        assert any("logo scan: 1 static area" in s and str(ss.LOGO_AREA) in s for s in said)
        # the same run without the flag
        monkeypatch.delenv("VSR_LOGO_SCAN")
        scans = ls.stats["scans"]
        sr2 = SubtitleRemover(src, device="cuda:0")
        sr2.text_detector, sr2.opencv_inpaint = NoText(), plugin
        sr2.append_output = lambda *a: None
        sr2.video_out_path = str(tmp_path / "out_off.y4m")
        with pytest.raises(Exception, match="No subtitle detected"):
            sr2.run()
        assert ls.stats["scans"] == scans and sr2.static_areas == []
    finally:
        config.inpaintMode.value = old_mode
        plugin.close()
    before, after = records(src, n), records(sr.video_out_path, n)
    ymin, ymax, xmin, xmax = ss.LOGO_AREA
    masked = create_mask((H, W), [(xmin, xmax, ymin, ymax)]) != 0
    assert masked[ymin:ymax, xmin:xmax].all() and not masked.all()
    assert np.array_equal(after[:, :, ~masked], before[:, :, ~masked]), "every sample outside the masked pixels is the source's"
    y0, y1, x0, x1 = ss.LOGO
    white = int(before[0, 0, y0, x0])
    assert (before[:, 0, y0:y1, x0:x1] == white).all() and white > int(before[:, 0][:, ~masked].max())
    assert (after[:, 0, ymin:ymax, xmin:xmax] < white).all(), "no pixel of any frame keeps the logo's white"
