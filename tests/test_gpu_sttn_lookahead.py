"""Look-ahead context frames (--sttn-lookahead M) on the GPU: the engine's entry points with a read-only suffix against the
plain call on the extended list (bit for bit), one oracle anchor, and both drivers against the definition:

    before    the look-back context of a chunk / batch [a, b) (tests/test_gpu_sttn_context.py, tests/test_gpu_sttn_det_context.py)
    after     sttn-auto: the source frames [b, min(b + M, c')) of a piece in the scene [c, c'); sttn-det: [b, min(b + M, e)) of a batch
              of the piece [c, e)
    result    what the plain call gives at the positions of [a, b) when run on the list before ++ selected ++ after
"""
import numpy as np
import pytest
import torch

from vsr_amd import synth
from vsr_amd.backend.tools import video_io
from vsr_amd.backend.tools.chunk_parallel import context_span, lookahead_span, scene_chunk_ranges
from vsr_amd.backend.tools.det_lookback import det_jobs
from vsr_amd.backend.tools.inpaint_tools import is_frame_number_in_ab_sections
from oracle.sttn_auto import STTNInpaintOracle, calculate_psnr, create_mask, get_inpaint_area_by_mask
from oracle import cv2_restate as cv2r
from vsr_amd.synth import make_state_dict

pytestmark = pytest.mark.gpu

H, W = 480, 852
BOX = (150, 400, 50, 800)
PSNR_MIN_DB = 50.0      # the bar of tests/test_gpu_sttn.py::test_auto_chunk_vs_oracle


@pytest.fixture(scope="module")
def sd():
    return make_state_dict(0, "auto")


def _mask_and_areas(boxes=(BOX,)):
    mask = create_mask((H, W), [(b[2], b[3], b[0], b[1]) for b in boxes])
    mask01 = cv2r.threshold_binary(mask, 127, 1)
    return mask, mask01, get_inpaint_area_by_mask(W, H, int(W * 3 / 16), mask01[:, :, None])


@pytest.fixture(scope="module")
def engines(built_lib, gpu_device, sd):
    """one engine per arithmetic, default window schedule (stride 5, references every 10)"""
    from vsr_amd.engine import SttnEngine

    made = {}

    def get(mode):
        if mode not in made:
            made[mode] = SttnEngine(sd, "auto", device=0, precision=mode)
        return made[mode]

    yield get
    for e in made.values():
        e.close()


@pytest.fixture(scope="module")
def clip28():
    return synth.make_clip(28, H, W, BOX, seed=17)


def _dev(a, dev):
    return None if a is None or len(a) == 0 else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _run(eng, dev, frames, mask01, areas, sel=None, context=None, lookahead=None):
    d = torch.from_numpy(np.ascontiguousarray(frames)).to(dev)
    c, a = _dev(context, dev), _dev(lookahead, dev)
    keep = [None if t is None else t.clone() for t in (c, a)]
    eng.auto_chunk(d, torch.from_numpy(mask01).to(dev), areas, sel=sel, context=c, lookahead=a)
    torch.cuda.synchronize()
    for t, k in zip((c, a), keep):
        assert t is None or torch.equal(t, k), "the context tensors are read-only"
    return d.cpu().numpy()


def _split(clip, n_ctx, Ls, n_after):
    return clip[:n_ctx], clip[n_ctx:n_ctx + Ls], clip[n_ctx + Ls:n_ctx + Ls + n_after]


def _check_engine_case(eng, dev, clip, n_ctx, Ls, n_after):
    _, mask01, areas = _mask_and_areas()
    ctx, frames, after = _split(clip, n_ctx, Ls, n_after)
    got = _run(eng, dev, frames, mask01, areas, context=ctx, lookahead=after)
    want = _run(eng, dev, clip[:n_ctx + Ls + n_after], mask01, areas)[n_ctx:n_ctx + Ls]
    assert np.array_equal(got, want)
    m = mask01.astype(bool)
    assert np.array_equal(got[:, ~m], frames[:, ~m]), "pixels outside the mask are untouched"
    assert (got[:, m] != frames[:, m]).mean() > 0.5
    back_only = _run(eng, dev, frames, mask01, areas, context=ctx)
    assert not np.array_equal(back_only, got), "the look-ahead changes the fill"


@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("mode", ["f32", "f16"])
@pytest.mark.parametrize("shape", [(5, 6), (7, 9)], ids=["5+12+6", "7+12+9"])
def test_lookahead_call_equals_the_extended_list(built_lib, gpu_device, engines, clip28, shape, mode, lanes):
    """12 written frames between n_ctx frames in front and n_after behind: the frames written are frames [n_ctx, n_ctx + 12) of the plain
    call on the whole list, bit for bit.  7 + 12 + 9: the windows at f = 0 (neighbours 0..5, all prefix) and f = 25 (20..27, all
    suffix) are dropped, one on each side."""
    eng = engines(mode)
    eng.set_lanes(lanes)
    _check_engine_case(eng, gpu_device, clip28, shape[0], 12, shape[1])


@pytest.mark.parametrize("shape", [(0, 12, 4), (3, 12, 9), (5, 4, 5)], ids=["0+12+4", "3+12+9", "5+4+5"])
def test_lookahead_call_edge_lists(built_lib, gpu_device, engines, clip28, shape):
    """0 + 12 + 4: a suffix only, no window dropped.  3 + 12 + 9: the window at f = 20 has neighbours 15..23, all suffix, and is dropped.
    5 + 4 + 5: the written run 5..8 lies strictly inside the window at f = 5 (neighbours 0..10), so q0 > 0 and q1 < nn."""
    eng = engines("f32")
    eng.set_lanes(1)
    _check_engine_case(eng, gpu_device, clip28, *shape)


def test_lookahead_call_two_areas_and_selection(built_lib, gpu_device, engines, clip28):
    eng = engines("f32")
    eng.set_lanes(2)
    _, mask01, areas = _mask_and_areas((BOX, (20, 60, 200, 600)))
    assert len(areas) >= 2
    n_ctx, n_after = 5, 6
    ctx, frames, after = _split(clip28, n_ctx, 12, n_after)
    sel = [0, 1, 3, 4, 5, 8, 9, 11]
    got = _run(eng, gpu_device, frames, mask01, areas, sel=sel, context=ctx, lookahead=after)
    ext_sel = list(range(n_ctx)) + [n_ctx + s for s in sel] + list(range(n_ctx + 12, n_ctx + 12 + n_after))
    ext = _run(eng, gpu_device, clip28[:n_ctx + 12 + n_after], mask01, areas, sel=ext_sel)
    assert np.array_equal(got, ext[n_ctx:n_ctx + 12])
    drop = [i for i in range(12) if i not in sel]
    assert np.array_equal(got[drop], frames[drop]), "unselected frames pass through"
    assert (got[sel] != frames[sel]).any()


def test_empty_lookahead_is_the_call_of_today(built_lib, gpu_device, engines, clip28):
    eng = engines("f32")
    eng.set_lanes(2)
    _, mask01, areas = _mask_and_areas()
    ctx, frames, _ = _split(clip28, 5, 12, 0)
    empty = torch.zeros((0, H, W, 3), dtype=torch.uint8, device=gpu_device)
    d = torch.from_numpy(np.ascontiguousarray(frames)).to(gpu_device)
    eng.auto_chunk(d, torch.from_numpy(mask01).to(gpu_device), areas, context=_dev(ctx, gpu_device), lookahead=empty)
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy(), _run(eng, gpu_device, frames, mask01, areas, context=ctx))


def test_lookahead_call_vs_oracle(built_lib, gpu_device, sd):
    """the one anchor: 3 + 4 + 4 frames (stride 2, references every 3) against the reference's chunk on the 11-frame list"""
    from vsr_amd.engine import SttnEngine

    eng = SttnEngine(sd, "auto", device=0, neighbor_stride=2, ref_length=3)
    clip = synth.make_clip(11, H, W, BOX, seed=23)
    _, mask01, areas = _mask_and_areas()
    got = _run(eng, gpu_device, clip[3:7], mask01, areas, context=clip[:3], lookahead=clip[7:])
    ref = np.stack(STTNInpaintOracle(sd, "auto", 2, 3).chunk(list(clip), mask01[:, :, None], areas))[3:7]
    m = mask01.astype(bool)
    psnr = calculate_psnr(got[:, m], ref[:, m])
    dmax = np.abs(got.astype(int) - ref.astype(int)).max()
    print(f"3 + 4 + 4 frames vs oracle: PSNR masked pixels {psnr:.2f} dB, max |d| {dmax}")
    assert np.array_equal(got[:, ~m], clip[3:7][:, ~m])
    assert psnr >= PSNR_MIN_DB
    assert dmax <= 2
    eng.close()


# ------------------------------------------------------------------------------------------------
# the sttn-det handle
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def det_sd():
    return make_state_dict(0, "det")


def _det_mask_and_areas():
    from vsr_amd.backend.tools.inpaint_tools import create_mask as cm, get_inpaint_area_by_mask as areas_of

    mask = cm((H, W), [(BOX[2], BOX[3], BOX[0], BOX[1])])
    return mask, areas_of(W, H, int(W * 5 / 18), mask[:, :, None])


def _det_run(eng, dev, frames, mask, areas, context=None, lookahead=None):
    d = torch.from_numpy(np.ascontiguousarray(frames)).to(dev)
    c, a = _dev(context, dev), _dev(lookahead, dev)
    keep = [None if t is None else t.clone() for t in (c, a)]
    eng.det_batch(d, torch.from_numpy(np.ascontiguousarray(mask)).to(dev), areas, mask_host=mask, context=c, lookahead=a)
    torch.cuda.synchronize()
    for t, k in zip((c, a), keep):
        assert t is None or torch.equal(t, k), "the context tensors are read-only"
    return d.cpu().numpy()


@pytest.mark.parametrize("shape", [(5, 6), (7, 9)], ids=["5+12+6", "7+12+9"])
def test_det_lookahead_call_equals_the_extended_list(built_lib, gpu_device, det_sd, clip28, shape):
    from vsr_amd.engine import SttnEngine

    eng = SttnEngine(det_sd, "det", device=0)
    try:
        mask, areas = _det_mask_and_areas()
        n_ctx, n_after = shape
        ctx, frames, after = _split(clip28, n_ctx, 12, n_after)
        got = _det_run(eng, gpu_device, frames, mask, areas, context=ctx, lookahead=after)
        want = _det_run(eng, gpu_device, clip28[:n_ctx + 12 + n_after], mask, areas)[n_ctx:n_ctx + 12]
        assert np.array_equal(got, want)
        rows = np.ones(H, dtype=bool)
        for a in areas:
            rows[a[0]:a[1]] = False
        assert rows.any() and np.array_equal(got[:, rows], frames[:, rows]), "rows outside the inpaint areas are untouched"
        assert (got[:, mask > 0] != frames[:, mask > 0]).any()
        assert not np.array_equal(_det_run(eng, gpu_device, frames, mask, areas, context=ctx), got), "the look-ahead changes the fill"
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------
# the sttn-auto plugin, file to file
# ------------------------------------------------------------------------------------------------
def _write_y4m(path, frames):
    w = video_io.Y4mWriter(path, 25.0, (W, H), chroma="444")
    for f in frames:
        w.write(f)
    w.release()


def _read_all(path):
    r = video_io.Y4mVideo(path)
    out = []
    while True:
        ok, fr = r.read()
        if not ok:
            break
        out.append(fr)
    r.release()
    return np.stack(out)


def _records(path):
    """the FRAME records of a *.y4m file, header line dropped"""
    data = open(path, "rb").read()
    return data[data.index(b"\n") + 1:]


def _write_expected(path, expected, monkeypatch):
    monkeypatch.setenv("VSR_IO_COLOR", "host")
    w = video_io.open_writer(path, 25.0, (W, H), frames=len(expected))
    for f in expected:
        w.write(f)
    w.release()
    return _records(path)


@pytest.fixture(scope="module")
def plugin(built_lib, gpu_device, sd):
    from vsr_amd.backend.inpaint.sttn_auto_inpaint import STTNAutoInpaint

    return STTNAutoInpaint("cuda:0", {"netG": sd}, None, clip_gap=12)


def _plugin_run(plugin, monkeypatch, src, out, resident="1", ab=None, context=0, scene_split=False, lookahead=0):
    """one run of the plugin's chunk loop src -> out (lookahead=None: the environment)"""
    from vsr_amd.backend.main import SubtitleRemover

    monkeypatch.setenv("VSR_IO_COLOR", "device")
    monkeypatch.setenv("VSR_IO_RESIDENT", resident)
    monkeypatch.setenv("VSR_IO_PER_RANK", "0")
    plugin.video_path = src
    plugin.context, plugin.scene_split, plugin.lookahead = context, scene_split, lookahead
    sr = SubtitleRemover(src, model_path=None)
    sr.ab_sections = ab
    sr.video_out_path = out
    mask, _, _ = _mask_and_areas()
    plugin(input_mask=mask, input_sub_remover=sr, tbar=None)
    if plugin.last_error is not None:
        raise plugin.last_error
    sr.video_writer.release()
    return sr


def _by_definition(eng, dev, src_frames, pieces, cuts, N, M, ab=None):
    """the definition at the top of this file, through the plain chunk call on whole frames read back from the source file"""
    _, mask01, areas = _mask_and_areas()
    out = src_frames.copy()
    starts, ends = [0] + list(cuts), list(cuts) + [len(src_frames)]
    spans = []
    for a, b in pieces:
        c = max(x for x in starts if x <= a)
        c1 = min(x for x in ends if x >= b)
        lo, _ = context_span(a, c, N)
        _, hi = lookahead_span(b, c1, M)
        spans.append((lo, hi))
        keep = [j for j in range(a, b) if is_frame_number_in_ab_sections(j, ab)]
        if not keep:
            continue
        sel = list(range(a - lo)) + [j - lo for j in keep] + list(range(b - lo, hi - lo))
        res = _run(eng, dev, src_frames[lo:hi], mask01, areas, sel=None if len(sel) == hi - lo else sel)
        out[a:b] = res[a - lo:b - lo]
    return out, spans


@pytest.mark.parametrize("ab", [None, [range(3, 20)]], ids=["all", "ab3-20"])
@pytest.mark.parametrize("N", [5, 0], ids=["N5", "N0"])
def test_plugin_lookahead_equals_the_definition(built_lib, gpu_device, plugin, tmp_path, monkeypatch, N, ab):
    """30 frames, clip_gap 12, look-ahead 5: pieces (0,12) (12,24) (24,30); the first and second look ahead at source frames 12..16 and
    24..28, the last has nothing behind it.  The resident loop and the host-frame loop write the same bytes, and those are the
    definition's."""
    N_FR, M = 30, 5
    src = str(tmp_path / "in.y4m")
    monkeypatch.setenv("VSR_IO_COLOR", "host")
    _write_y4m(src, synth.make_clip(N_FR, H, W, BOX, seed=29))
    frames = _read_all(src)                                # what every loop decodes
    pieces = scene_chunk_ranges(N_FR, 12, [])
    expected, spans = _by_definition(plugin.sttn_inpaint.engine, gpu_device, frames, pieces, [], N, M, ab)
    assert spans == [(0, 17), (12 - N, 29), (24 - N, 30)]
    want = _write_expected(str(tmp_path / "want.y4m"), expected, monkeypatch)
    outs = {}
    for mode, resident in (("resident", "1"), ("host", "0")):
        out = str(tmp_path / f"out_{mode}.y4m")
        _plugin_run(plugin, monkeypatch, src, out, resident=resident, ab=ab, context=N, lookahead=M)
        outs[mode] = _records(out)
    assert outs["resident"] == outs["host"]
    assert outs["resident"] == want
    back = str(tmp_path / "back.y4m")
    _plugin_run(plugin, monkeypatch, src, back, ab=ab, context=N, lookahead=0)
    assert _records(back) != outs["resident"], "the look-ahead changes what is written"
    if N == 0 and ab is None:
        # M = 0 is byte for byte the run without the variable set
        monkeypatch.delenv("VSR_STTN_LOOKAHEAD", raising=False)
        unset = str(tmp_path / "unset.y4m")
        _plugin_run(plugin, monkeypatch, src, unset, context=0, lookahead=None)
        assert _records(unset) == _records(back)
        monkeypatch.setenv("VSR_STTN_LOOKAHEAD", str(M))
        env = str(tmp_path / "env.y4m")
        _plugin_run(plugin, monkeypatch, src, env, context=0, lookahead=None)
        assert _records(env) == outs["resident"], "the environment variable reaches the run"


def test_plugin_lookahead_stops_at_the_cut(built_lib, gpu_device, plugin, tmp_path, monkeypatch):
    """With scene_split the clip A ++ B (17 + 16 frames) is written as run(A) followed by run(B), byte for byte, with N = M = 5: the
    piece (12, 17) has nothing behind it in its scene, the piece (17, 29) nothing in front"""
    from vsr_amd.backend.tools.subtitle_detect import SubtitleDetect

    A, B = synth.make_clip(17, H, W, BOX, seed=1), synth.make_clip(16, H, W, BOX, seed=2)
    paths = {k: str(tmp_path / f"{k}.y4m") for k in ("a", "b", "ab")}
    monkeypatch.setenv("VSR_IO_COLOR", "host")
    _write_y4m(paths["a"], A)
    _write_y4m(paths["b"], B)
    _write_y4m(paths["ab"], np.concatenate([A, B]))
    assert SubtitleDetect.get_scene_div_frame_no(paths["ab"], 0) == [18]
    rec = {}
    for k in ("a", "b"):
        out = str(tmp_path / f"out_{k}.y4m")
        _plugin_run(plugin, monkeypatch, paths[k], out, context=5, lookahead=5)
        rec[k] = _records(out)
    out = str(tmp_path / "out_split.y4m")
    _plugin_run(plugin, monkeypatch, paths["ab"], out, context=5, lookahead=5, scene_split=True)
    assert plugin.scene_cuts == [17]
    assert _records(out) == rec["a"] + rec["b"]
    out2 = str(tmp_path / "out_grid.y4m")
    _plugin_run(plugin, monkeypatch, paths["ab"], out2, context=5, lookahead=5, scene_split=False)
    assert _records(out2) != rec["a"] + rec["b"], "the fixed grid feeds frames of the other scene to the attention"


# ------------------------------------------------------------------------------------------------
# the sttn-det driver: SubtitleRemover.video_inpaint
# ------------------------------------------------------------------------------------------------
QUAD = np.array([[[BOX[2], BOX[0]], [BOX[3], BOX[0]], [BOX[3], BOX[1]], [BOX[2], BOX[1]]]])


class Det:
    """an injected detector that reports the same box on every frame (the reference's host signature)"""
    batch_size = 4

    def predict(self, img):
        return [{"dt_polys": QUAD}]


class config_values:
    """batches of at most 12 frames, stride 2, references every 3, sttn-det; put back afterwards"""

    def __enter__(self):
        from vsr_amd.backend.config import config
        from vsr_amd.backend.tools.constant import InpaintMode

        self.keys = {"sttnMaxLoadNum": 12, "sttnNeighborStride": 2, "sttnReferenceLength": 3}
        self.old = {k: getattr(config, k).value for k in self.keys}
        self.old_mode = config.inpaintMode.value
        for k, v in self.keys.items():
            getattr(config, k).value = v
        config.inpaintMode.value = InpaintMode.STTN_DET
        assert config.getSttnMaxLoadNum() == 12

    def __exit__(self, *exc):
        from vsr_amd.backend.config import config

        for k, v in self.old.items():
            getattr(config, k).value = v
        config.inpaintMode.value = self.old_mode


@pytest.fixture(scope="module")
def det_plugin(built_lib, gpu_device):
    from vsr_amd.backend.inpaint.sttn_det_inpaint import STTNDetInpaint

    with config_values():
        return STTNDetInpaint("cuda:0", {"netG": make_state_dict(1, "det")})


class Recording:
    """the plugin, with the masks the driver hands it written down"""
    accepts_device_frames = True
    accepts_context = True

    def __init__(self, inner):
        self.inner, self.masks = inner, []

    def __call__(self, frames, mask, context=None, lookahead=None):
        self.masks.append(np.array(mask))
        return self.inner(frames, mask, context=context, lookahead=lookahead)


def _driver_run(plugin, monkeypatch, src, out, resident="1", context=0, lookahead=0, lanes=1):
    from vsr_amd.backend.main import SubtitleRemover

    monkeypatch.setenv("VSR_IO_COLOR", "device")
    monkeypatch.setenv("VSR_IO_RESIDENT", resident)
    monkeypatch.setenv("VSR_BATCH_LANES", str(lanes))
    monkeypatch.setenv("VSR_STTN_CONTEXT", str(context))
    monkeypatch.setenv("VSR_STTN_LOOKAHEAD", str(lookahead))
    monkeypatch.setenv("VSR_SCENE_SPLIT", "0")
    with config_values():
        sr = SubtitleRemover(src, device="cuda:0")
        sr.sub_areas = [(0, sr.frame_height, 0, sr.frame_width)]
        sr.video_out_path = out
        sr.update_progress = lambda tbar, increment: None
        sr.video_inpaint(object(), plugin, text_detector=Det())
        sr.video_writer.release()
    return sr


@pytest.mark.parametrize("N", [5, 0], ids=["N5", "N0"])
def test_driver_lookahead_across_batch_seams(built_lib, gpu_device, det_plugin, tmp_path, monkeypatch, N):
    """27 frames in one interval at a batch limit of 12 give batches 10 / 10 / 7; with M = 12 the first batch looks ahead at source
    frames 10..21 -- rows of the second AND of the third batch.  The resident loop (in place: a batch copies its look-ahead aside before
    the batches behind it may run), the host-frame loop and two plugin instances side by side write the same records, and those are the
    definition's: the plain two-argument plugin call on every batch's extended list, read back from the source file."""
    N_FR, M = 27, 12
    src = str(tmp_path / "in.y4m")
    monkeypatch.setenv("VSR_IO_COLOR", "host")
    _write_y4m(src, synth.make_clip(N_FR, H, W, BOX, seed=31))
    frames = _read_all(src)
    jobs = det_jobs({1: N_FR}, N_FR, lambda a, b: None, (), N, 12, M)
    assert [(j[0], j[1], j[4]) for j in jobs] == [(0, 10, 22), (10, 20, 27), (20, 27, 27)]
    outs, rec = {}, Recording(det_plugin)
    for mode, resident, lanes in (("lanes2", "1", 2), ("resident", "1", 1), ("host", "0", 1)):
        out = str(tmp_path / f"out_{mode}.y4m")
        sr = _driver_run(rec if mode == "host" else det_plugin, monkeypatch, src, out, resident=resident, context=N, lookahead=M, lanes=lanes)
        assert ("read + upload + YUV->BGR" in sr.phase_seconds) == (resident == "1"), "the loop the test means to run"
        outs[mode] = _records(out)
    assert len(rec.masks) == 3 and all(np.array_equal(x, rec.masks[0]) for x in rec.masks)
    mask = rec.masks[0]
    expected = frames.copy()
    for lo, hi, ctx_lo, _, ahead_hi in jobs:
        expected[lo:hi] = np.stack(det_plugin(list(frames[ctx_lo:ahead_hi]), mask)[lo - ctx_lo:hi - ctx_lo])
    want = _write_expected(str(tmp_path / "want.y4m"), expected, monkeypatch)
    assert outs["resident"] == want
    assert outs["host"] == outs["resident"]
    assert outs["lanes2"] == outs["resident"]
    back = str(tmp_path / "back.y4m")
    _driver_run(det_plugin, monkeypatch, src, back, context=N, lookahead=0)
    assert _records(back) != outs["resident"], "the look-ahead changes what is written"


def test_windows_are_refused_before_a_frame_is_read(built_lib, gpu_device, det_plugin, tmp_path, monkeypatch):
    """a windowed run with M > 0: the header says the clip is over the budget (3 of its 6 frames fit), the refusal names the option"""
    from vsr_amd.backend import main as m
    from vsr_amd.backend.tools.resident import ResidentClip
    from vsr_amd.backend.tools.subtitle_detect import SubtitleDetect

    src = str(tmp_path / "in.y4m")
    monkeypatch.setenv("VSR_IO_COLOR", "host")
    _write_y4m(src, synth.make_clip(6, H, W, BOX, seed=3))
    monkeypatch.setenv("VSR_IO_COLOR", "device")
    reads = []

    def no_read(*a, **kw):
        reads.append(1)
        raise AssertionError("a frame was read")

    with config_values():
        sr = m.SubtitleRemover(src, device="cuda:0")
        sr.sub_areas = [(0, sr.frame_height, 0, sr.frame_width)]
        sr.video_out_path = str(tmp_path / "out.y4m")
        monkeypatch.setattr(ResidentClip, "load", no_read)
        monkeypatch.setattr(SubtitleDetect, "find_subtitle_frame_no", no_read)
        monkeypatch.setenv("VSR_STTN_CONTEXT", "0")
        monkeypatch.setenv("VSR_SCENE_SPLIT", "0")
        monkeypatch.setenv("VSR_STTN_LOOKAHEAD", "5")
        monkeypatch.setenv("VSR_IO_RESIDENT", "windows")
        monkeypatch.setenv("VSR_RESIDENT_GB", repr(3 * H * W * 3 / 2 ** 30))
        with pytest.raises(RuntimeError, match="resident windows") as e:
            sr.video_inpaint(object(), det_plugin, text_detector=Det())
        assert "--sttn-lookahead" in str(e.value)
    assert not reads
