"""--opencv-fill exemplar on the GPU against tests/_exemplar_statement.py, byte for byte: every launch of a call on its own, each fed the
statement's own input for that stage (vsr_exemplar_run_stage and the workspace layout); whole calls, strided frames and workspace
reuse; the plugin under VSR_OPENCV_FILL=exemplar in both forms, behind --seam-feather, and through a file-to-file run."""
import numpy as np
import pytest
import torch

from tests import _exemplar_statement as es
from tests import _feather_statement as fs

pytestmark = pytest.mark.gpu

STAGE_CASES = ("48x64", "37x53", "64x96_two")
NAMES = ("VSR_SEAM_FEATHER", "VSR_REGRAIN", "VSR_DEFLICKER", "VSR_TONE_MATCH", "VSR_GLYPH_KEY", "VSR_GLYPH_HOLD", "VSR_BORROW", "VSR_BORROW_PAN",
         "VSR_LOGO_SCAN", "VSR_LOGO_UNBLEND")
_traces = {}


@pytest.fixture(scope="module")
def engine(built_lib, gpu_device):
    from vsr_amd.engine import ExemplarEngine

    eng = ExemplarEngine(device=0, max_plans=8)
    yield eng
    eng.close()


def traced(name, seeds=(0, 3)):
    """per seed (input, mask, filled, trace of the statement), computed once and left unchanged"""
    if name not in _traces:
        runs = []
        for seed in seeds:
            _, img, mask = es.case(name, seed)
            trace = []
            out = es.fill(img, mask, trace)
            runs.append((img, mask, out, trace))
        _traces[name] = runs
    return _traces[name]


class Stage:
    """the workspace of one (mask, n) seen through the layout query"""

    def __init__(self, engine, mask, frames):
        self.eng, self.mask, self.frames, self.n = engine, mask, frames, frames.shape[0]
        self.levels = engine.plan_levels(mask)
        self.ws = engine.workspace(engine.plan(mask), self.n)

    def _img_view(self, level):
        if level == 0:
            return self.frames
        off, size, _, _, _ = self.eng.layout(self.mask, self.n, level)
        lv = self.levels[level]
        return self.ws[off:off + self.n * size].view(self.n, lv["H"], lv["W"], 3)

    def put_img(self, level, imgs):
        self._img_view(level).copy_(torch.from_numpy(np.stack(imgs)).to(self.frames.device))

    def get_img(self, level):
        return self._img_view(level).cpu().numpy()

    def _field_view(self, level, b):
        _, _, fa, fb, size = self.eng.layout(self.mask, self.n, level)
        off = fb if b else fa
        return self.ws[off:off + self.n * size]

    def put_field(self, level, b, fields):
        y0, x0, h, w = self.levels[level]["box"]
        raw = np.stack([f[y0:y0 + h, x0:x0 + w].astype(np.int16) for f in fields])
        self._field_view(level, b).copy_(torch.from_numpy(raw.view(np.uint8).reshape(-1)).to(self.frames.device))

    def get_field(self, level, b):
        """dense int32 [n,H,W,2] like the statement's"""
        lv = self.levels[level]
        y0, x0, h, w = lv["box"]
        raw = self._field_view(level, b).cpu().numpy().view(np.int16).reshape(self.n, h, w, 2)
        out = np.full((self.n, lv["H"], lv["W"], 2), -1, np.int32)
        out[:, y0:y0 + h, x0:x0 + w] = raw
        return out

    def run(self, stage, level, it=0, ps=0, from_b=False):
        self.eng.run_stage(self.frames, self.mask, stage, level, it, ps, from_b)
        torch.cuda.synchronize()


@pytest.mark.parametrize("stage", ["down", "init", "up", "search", "vote"])
@pytest.mark.parametrize("name", STAGE_CASES)
def test_every_launch_equals_the_statement(built_lib, gpu_device, engine, name, stage):
    """every launch of that kind that a call makes, two frames at once, from the statement's own state in front of it"""
    runs = traced(name)
    mask = runs[0][1]
    inputs = [r[0] for r in runs]
    frames = torch.from_numpy(np.stack(inputs)).to(gpu_device)
    st = Stage(engine, mask, frames)
    nl = len(st.levels)
    assert nl == len(es.plan(mask)[0]) >= 2
    traces = [r[3] for r in runs]
    checked = 0
    for i, entry in enumerate(traces[0]):
        kind, level, it, ps = entry[:4]
        if kind != stage:
            continue
        now = [t[i] for t in traces]
        prev = [t[i - 1] for t in traces] if i else None
        assert all(e[:4] == entry[:4] for e in now)
        # the image the launch finds at its level (for `down`: at the level it reads)
        if kind == "down":
            st.put_img(level - 1, [p[4] for p in prev] if level > 1 else inputs)
            st.run(built_lib.EX_DOWN, level)
            assert np.array_equal(st.get_img(level), np.stack([e[4] for e in now]))
        elif kind == "init":
            before = [p[4] for p in prev] if prev and prev[0][1] == level else inputs
            st.put_img(level, before)
            st.run(built_lib.EX_INIT, level)
            got, want = st.get_img(level), np.stack([e[4] for e in now])
            assert np.array_equal(got, want), f"{int((got != want).sum())} bytes differ"
            assert not np.array_equal(want, np.stack(before))
        elif kind == "up":
            if level < nl - 1:
                st.put_field(level + 1, False, [p[5] for p in prev])
            st.run(built_lib.EX_UP, level)
            want = np.stack([e[5] for e in now])
            assert np.array_equal(st.get_field(level, False), want) and np.array_equal(st.get_field(level, True), want)
        elif kind == "search":
            from_b = bool(ps & 1)
            st.put_img(level, [p[4] for p in prev])
            st.put_field(level, from_b, [p[5] for p in prev])
            st.put_field(level, not from_b, [np.where(p[5] >= 0, 0, -1) for p in prev])      # the pass must write every target
            st.run(built_lib.EX_SEARCH, level, it, ps, from_b)
            got, want = st.get_field(level, not from_b), np.stack([e[5] for e in now])
            assert np.array_equal(got, want), f"level {level} it {it} pass {ps}: {int((got != want).any(-1).sum())} matches differ"
            assert np.array_equal(st.get_field(level, from_b), np.stack([p[5] for p in prev])), "the field it reads stays"
        else:
            st.put_img(level, [p[4] for p in prev])
            st.put_field(level, True, [e[5] for e in now])
            st.run(built_lib.EX_VOTE, level, from_b=True)
            got, want = st.get_img(level), np.stack([e[4] for e in now])
            assert np.array_equal(got, want), f"level {level}: {int((got != want).sum())} bytes differ"
            if name == "37x53" and level == 0:
                hole = st.levels[0]["cls"] & 1
                assert hole[-1].any() and hole[:, -1].any(), "hole pixels on the edges: fewer than 49 contributors"
        checked += 1
    assert checked >= (1 if stage in ("down", "init") else 2)
    if stage == "search":
        assert checked == nl * es.ITERS * es.PASSES


@pytest.mark.parametrize("name", ["48x64", "37x53", "64x96_two", "96x160", "thin"])
def test_a_call_equals_the_statement(built_lib, gpu_device, engine, name):
    clean, img, mask = es.case(name)
    want = es.fill(img, mask)
    frames = torch.from_numpy(img[None].copy()).to(gpu_device)
    out = engine.inpaint(frames, mask)
    torch.cuda.synchronize()
    got = frames.cpu().numpy()[0]
    assert out.data_ptr() == frames.data_ptr()
    assert np.array_equal(got, want), f"{int((got != want).any(-1).sum())} pixels differ from the statement"
    assert np.array_equal(got[mask == 0], img[mask == 0])
    levels = len(engine.plan_levels(mask))
    assert levels == (1 if name == "thin" else levels) and (name != "96x160" or levels >= 3)


def test_strided_frames_and_workspace_reuse(built_lib, gpu_device, engine):
    """three frames with different seeds in a buffer whose frame stride exceeds a frame (and is odd); then another n on the same handle"""
    name = "37x53"
    cases = [es.case(name, seed) for seed in (0, 3, 9)]
    mask = cases[0][2]
    want = [es.fill(c[1], mask) for c in cases]
    H, W = mask.shape
    size, gap = H * W * 3, 61
    buf = torch.full((3 * (size + gap),), 7, dtype=torch.uint8, device=gpu_device)
    frames = torch.as_strided(buf, (3, H, W, 3), (size + gap, W * 3, 3, 1))
    frames.copy_(torch.from_numpy(np.stack([c[1] for c in cases])).to(gpu_device))
    engine.inpaint(frames, mask)
    torch.cuda.synchronize()
    raw = buf.cpu().numpy().reshape(3, size + gap)
    for f in range(3):
        assert np.array_equal(raw[f, :size].reshape(H, W, 3), want[f]), f"frame {f}"
    assert (raw[:, size:] == 7).all(), "the bytes between the frames stay"
    builds = engine.plan_builds
    two = torch.from_numpy(np.stack([cases[2][1], cases[0][1]])).to(gpu_device)
    engine.inpaint(two, mask)
    one = torch.from_numpy(cases[1][1][None].copy()).to(gpu_device)
    engine.inpaint(one, mask)
    torch.cuda.synchronize()
    assert engine.plan_builds == builds, "the same mask: the same plan"
    assert np.array_equal(two.cpu().numpy(), np.stack([want[2], want[0]])) and np.array_equal(one.cpu().numpy()[0], want[1])
    # out= : the frames stay, the copy is filled; an empty mask and an empty batch change nothing
    src = torch.from_numpy(cases[0][1][None].copy()).to(gpu_device)
    dst = torch.zeros_like(src)
    engine.inpaint(src, mask, out=dst)
    assert np.array_equal(src.cpu().numpy()[0], cases[0][1]) and np.array_equal(dst.cpu().numpy()[0], want[0])
    engine.inpaint(src, np.zeros_like(mask))
    engine.inpaint(src[:0], mask)
    assert np.array_equal(src.cpu().numpy()[0], cases[0][1])
    with pytest.raises(built_lib.VsrError, match="no 7x7 patch"):
        engine.inpaint(src, np.full_like(mask, 255))
    assert np.array_equal(src.cpu().numpy()[0], cases[0][1]), "refused before a frame is touched"


# ---- the plugin -----------------------------------------------------------------------------------------------------------------------------
def test_plugin_gives_the_statements_bytes(built_lib, gpu_device, monkeypatch):
    from tests.test_gpu_seam_feather import call_device, call_list
    from vsr_amd.backend.inpaint.opencv_inpaint import OpenCVInpaint
    from vsr_amd.engine import ExemplarEngine, TeleaEngine

    for name in NAMES:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.delenv("VSR_OPENCV_BACKEND", raising=False)
    cases = [es.case("48x64", seed) for seed in (0, 3)]
    mask = cases[0][2]
    clip = np.stack([c[1] for c in cases])
    want = es.exemplar(clip, mask)
    monkeypatch.setenv("VSR_OPENCV_FILL", "exemplar")
    plugin = OpenCVInpaint("cuda:0")
    monkeypatch.delenv("VSR_OPENCV_FILL")
    telea = OpenCVInpaint("cuda:0")
    try:
        assert type(plugin.engine) is ExemplarEngine and type(telea.engine) is TeleaEngine
        assert np.array_equal(call_device(plugin, clip, mask, gpu_device), want)
        assert plugin.engine.plan_builds == 1 and plugin.engine.plan_hits == 0
        assert np.array_equal(call_list(plugin, clip, mask), want)
        assert plugin.engine.plan_builds == 1 and plugin.engine.plan_hits == 1, "the second call with the same mask hits the plan cache"
        assert np.array_equal(call_list(plugin, clip, mask[:, :, None]), want)
        assert np.array_equal(plugin.inpaint(clip[0], mask), want[0])
        monkeypatch.setenv("VSR_SEAM_FEATHER", "4")
        C = plugin.composite_mask(mask)
        feathered = fs.composite(want, clip, C, 4)
        assert np.array_equal(call_device(plugin, clip, mask, gpu_device), feathered)
        assert np.array_equal(call_list(plugin, clip, mask), feathered) and not np.array_equal(feathered, want)
        monkeypatch.delenv("VSR_SEAM_FEATHER")
        other = call_device(telea, clip, mask, gpu_device)
        assert not np.array_equal(other, want) and np.array_equal(other[:, mask == 0], want[:, mask == 0])
        twin = plugin.clone()
        assert type(twin.engine) is ExemplarEngine and np.array_equal(call_device(twin, clip, mask, gpu_device), want)
        twin.close()
    finally:
        plugin.close()
        telea.close()


def test_a_file_to_file_run(built_lib, gpu_device, tmp_path, monkeypatch):
    """*.y4m in -> SubtitleRemover.run() in opencv mode (no weights), the area found by --logo-scan as in tests/test_gpu_seam_unmix.py:
    outside the masked pixels the written samples are the source's with and without the flag, inside them the two fills differ"""
    from tests import _static_statement as ss
    from tests.test_gpu_logo_scan import NoText, records, write_y4m
    from vsr_amd.backend import main as m
    from vsr_amd.backend.config import config
    from vsr_amd.backend.tools.inpaint_tools import create_mask

    clip = ss.clip_logo()
    n, H, W = clip.shape[:3]
    src = write_y4m(tmp_path / "in.y4m", clip)

    def run(out, flags):
        for name in NAMES:
            monkeypatch.setenv(name, "0")                              # (main() writes the flags into the environment: put back afterwards)
        monkeypatch.setenv("VSR_OPENCV_FILL", "")
        monkeypatch.setenv("VSR_Y4M_OUT", "source")
        monkeypatch.delenv("VSR_OPENCV_BACKEND", raising=False)
        monkeypatch.setattr(m.SubtitleRemover, "_default_detector", lambda self: NoText())
        old = config.inpaintMode.value
        try:
            m.main(["-i", src, "-o", str(out), "--inpaint-mode", "opencv", "--logo-scan"] + flags)
        finally:
            config.inpaintMode.value = old
        return records(str(out), n)

    telea = run(tmp_path / "telea.y4m", [])
    exemplar = run(tmp_path / "exemplar.y4m", ["--opencv-fill", "exemplar"])
    before = records(src, n)
    ymin, ymax, xmin, xmax = ss.LOGO_AREA
    masked = create_mask((H, W), [(xmin, xmax, ymin, ymax)]) != 0
    assert masked.any() and not masked.all()
    assert np.array_equal(exemplar[:, :, ~masked], before[:, :, ~masked]), "outside the box the written frames are the source"
    assert np.array_equal(telea[:, :, ~masked], before[:, :, ~masked])
    assert (exemplar[:, :, masked] != before[:, :, masked]).any()
    assert (exemplar[:, :, masked] != telea[:, :, masked]).any(), "inside it the exemplar fill is not Telea's"
