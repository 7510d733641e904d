"""sttn-auto with look-back context frames and scene-bounded chunks on the GPU: the engine's context entry point against the plain
call on the extended list (bit for bit), one oracle anchor, and the plugin's two loops against the definition:

    pieces    scene_chunk_ranges(total, clip_gap, cuts)        (cuts = p - 1 of SubtitleDetect.get_scene_div_frame_no)
    context   the source frames [max(a - N, c), a) of a piece [a, b) in the scene starting at c
    result    what the plain chunk call gives for the selected frames of [a, b) when run on the list context ++ selected
"""
import numpy as np
import pytest
import torch

from vsr_amd import synth
from vsr_amd.backend.tools import video_io
from vsr_amd.backend.tools.chunk_parallel import context_span, scene_chunk_ranges
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
def clip19():
    return synth.make_clip(19, H, W, BOX, seed=17)


def _run(eng, dev, frames, mask01, areas, sel=None, context=None):
    d = torch.from_numpy(np.ascontiguousarray(frames)).to(dev)
    c = None if context is None else torch.from_numpy(np.ascontiguousarray(context)).to(dev)
    keep = None if c is None else c.clone()
    eng.auto_chunk(d, torch.from_numpy(mask01).to(dev), areas, sel=sel, context=c)
    torch.cuda.synchronize()
    if c is not None:
        assert torch.equal(c, keep), "the context tensor is read-only"
    return d.cpu().numpy()


@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("mode", ["f32", "f16"])
@pytest.mark.parametrize("n_ctx", [3, 5, 7])
def test_context_call_equals_the_extended_list(built_lib, gpu_device, engines, clip19, n_ctx, mode, lanes):
    """L = 12 frames behind n_ctx context frames: the frames written are frames n_ctx: of the plain call on all n_ctx + 12, bit for
    bit (7 is no multiple of the stride: the window grid sits elsewhere on the written frames)."""
    eng = engines(mode)
    eng.set_lanes(lanes)
    _, mask01, areas = _mask_and_areas()
    ctx, frames = clip19[7 - n_ctx:7], clip19[7:19]
    got = _run(eng, gpu_device, frames, mask01, areas, context=ctx)
    want = _run(eng, gpu_device, np.concatenate([ctx, frames]), mask01, areas)[n_ctx:]
    assert np.array_equal(got, want)
    m = mask01.astype(bool)
    assert np.array_equal(got[:, ~m], frames[:, ~m]), "pixels outside the mask are untouched"
    assert (got[:, m] != frames[:, m]).mean() > 0.5
    alone = _run(eng, gpu_device, frames, mask01, areas)
    assert not np.array_equal(alone, got), "the context changes the fill"


def test_context_call_two_areas_and_selection(built_lib, gpu_device, engines, clip19):
    eng = engines("f32")
    eng.set_lanes(2)
    _, mask01, areas = _mask_and_areas((BOX, (20, 60, 200, 600)))
    assert len(areas) >= 2
    n_ctx = 5
    ctx, frames = clip19[2:7], clip19[7:19]
    sel = [0, 1, 3, 4, 5, 8, 9, 11]
    got = _run(eng, gpu_device, frames, mask01, areas, sel=sel, context=ctx)
    ext = _run(eng, gpu_device, np.concatenate([ctx, frames]), mask01, areas, sel=list(range(n_ctx)) + [n_ctx + s for s in sel])
    assert np.array_equal(got, ext[n_ctx:])
    drop = [i for i in range(12) if i not in sel]
    assert np.array_equal(got[drop], frames[drop]), "unselected frames pass through"
    assert (got[sel] != frames[sel]).any()


def test_empty_context_is_the_plain_call(built_lib, gpu_device, engines, clip19):
    eng = engines("f32")
    eng.set_lanes(2)
    _, mask01, areas = _mask_and_areas()
    frames = clip19[:12]
    got = _run(eng, gpu_device, frames, mask01, areas, context=np.zeros((0, H, W, 3), np.uint8))
    assert np.array_equal(got, _run(eng, gpu_device, frames, mask01, areas))


def test_context_call_vs_oracle(built_lib, gpu_device, sd):
    """the one anchor: 3 context + 4 written frames (stride 2, references every 3) against the reference's chunk on the 7-frame list"""
    from vsr_amd.engine import SttnEngine

    eng = SttnEngine(sd, "auto", device=0, neighbor_stride=2, ref_length=3)
    clip = synth.make_clip(7, H, W, BOX, seed=23)
    _, mask01, areas = _mask_and_areas()
    got = _run(eng, gpu_device, clip[3:], mask01, areas, context=clip[:3])
    ref = np.stack(STTNInpaintOracle(sd, "auto", 2, 3).chunk(list(clip), mask01[:, :, None], areas))[3:]
    m = mask01.astype(bool)
    psnr = calculate_psnr(got[:, m], ref[:, m])
    dmax = np.abs(got.astype(int) - ref.astype(int)).max()
    print(f"context 3 + 4 frames vs oracle: PSNR masked pixels {psnr:.2f} dB, max |d| {dmax}")
    assert np.array_equal(got[:, ~m], clip[3:][:, ~m])
    assert psnr >= PSNR_MIN_DB
    assert dmax <= 2
    eng.close()


# ------------------------------------------------------------------------------------------------
# the plugin
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


@pytest.fixture(scope="module")
def plugin(built_lib, gpu_device, sd):
    from vsr_amd.backend.inpaint.sttn_auto_inpaint import STTNAutoInpaint

    return STTNAutoInpaint("cuda:0", {"netG": sd}, None, clip_gap=12)


def _plugin_run(plugin, monkeypatch, src, out, resident="1", ab=None, **opts):
    """one run of the plugin's chunk loop src -> out; returns the remover (phase_seconds)"""
    from vsr_amd.backend.main import SubtitleRemover

    monkeypatch.setenv("VSR_IO_COLOR", "device")
    monkeypatch.setenv("VSR_IO_RESIDENT", resident)
    monkeypatch.setenv("VSR_IO_PER_RANK", "0")
    plugin.video_path = src
    plugin.context, plugin.scene_split = opts.get("context", 0), opts.get("scene_split", False)
    sr = SubtitleRemover(src, model_path=None)
    sr.ab_sections = ab
    sr.video_out_path = out
    mask, _, _ = _mask_and_areas()
    plugin(input_mask=mask, input_sub_remover=sr, tbar=None)
    if plugin.last_error is not None:
        raise plugin.last_error
    sr.video_writer.release()
    return sr


def _by_definition(eng, dev, src_frames, pieces, cuts, N, ab=None):
    """the definition at the top of this file, through the plain chunk call on whole frames read back from the source file"""
    _, mask01, areas = _mask_and_areas()
    out = src_frames.copy()
    starts = [0] + list(cuts)
    for a, b in pieces:
        c = max(x for x in starts if x <= a)
        lo, _ = context_span(a, c, N)
        keep = [j for j in range(a, b) if is_frame_number_in_ab_sections(j, ab)]
        if not keep:
            continue
        sel = list(range(a - lo)) + [j - lo for j in keep]
        res = _run(eng, dev, src_frames[lo:b], mask01, areas, sel=None if len(sel) == b - lo else sel)
        out[a:b] = res[a - lo:]
    return out


@pytest.mark.parametrize("ab", [None, [range(3, 20)]], ids=["all", "ab3-20"])
def test_plugin_context_equals_the_definition(built_lib, gpu_device, plugin, tmp_path, monkeypatch, ab):
    """30 frames, clip_gap 12, context 5: pieces (0,12) (12,24) (24,30); the second and third look back at source frames 7..11 and
    19..23.  The resident loop and the host-frame loop write the same bytes, and those are the definition's."""
    N_FR, N = 30, 5
    src = str(tmp_path / "in.y4m")
    monkeypatch.setenv("VSR_IO_COLOR", "host")
    _write_y4m(src, synth.make_clip(N_FR, H, W, BOX, seed=29))
    frames = _read_all(src)                                # what every loop decodes
    pieces = scene_chunk_ranges(N_FR, 12, [])
    assert pieces == [(0, 12), (12, 24), (24, 30)]
    want = str(tmp_path / "want.y4m")
    expected = _by_definition(plugin.sttn_inpaint.engine, gpu_device, frames, pieces, [], N, ab)
    w = video_io.open_writer(want, 25.0, (W, H), frames=N_FR)
    for f in expected:
        w.write(f)
    w.release()
    outs = {}
    for mode, resident in (("resident", "1"), ("host", "0")):
        out = str(tmp_path / f"out_{mode}.y4m")
        _plugin_run(plugin, monkeypatch, src, out, resident=resident, ab=ab, context=N)
        outs[mode] = _records(out)
    assert outs["resident"] == outs["host"]
    assert outs["resident"] == _records(want)
    plain = str(tmp_path / "plain.y4m")
    _plugin_run(plugin, monkeypatch, src, plain, ab=ab, context=0)
    assert _records(plain) != outs["resident"], "the look-back changes what is written"


@pytest.fixture(scope="module")
def two_scenes():
    """scene A (17 frames) then scene B (16): two seeded textures, each translating slowly"""
    return synth.make_clip(17, H, W, BOX, seed=1), synth.make_clip(16, H, W, BOX, seed=2)


@pytest.mark.parametrize("N", [0, 5], ids=["split", "split+context5"])
def test_plugin_scene_split(built_lib, gpu_device, plugin, two_scenes, tmp_path, monkeypatch, N):
    """With scene_split the clip A ++ B is written as run(A) followed by run(B), byte for byte (with a context too: it stops at the
    cut); without it the chunk (12, 24) straddles the cut at frame 17 and the output differs."""
    from vsr_amd.backend.tools.subtitle_detect import SubtitleDetect

    A, B = two_scenes
    paths = {k: str(tmp_path / f"{k}.y4m") for k in ("a", "b", "ab")}
    monkeypatch.setenv("VSR_IO_COLOR", "host")
    _write_y4m(paths["a"], A)
    _write_y4m(paths["b"], B)
    _write_y4m(paths["ab"], np.concatenate([A, B]))
    assert SubtitleDetect.get_scene_div_frame_no(paths["ab"], 0) == [18]
    rec = {}
    for k in ("a", "b"):
        out = str(tmp_path / f"out_{k}.y4m")
        _plugin_run(plugin, monkeypatch, paths[k], out, context=N)
        rec[k] = _records(out)
    out = str(tmp_path / "out_split.y4m")
    sr = _plugin_run(plugin, monkeypatch, paths["ab"], out, context=N, scene_split=True)
    assert plugin.scene_cuts == [17]
    assert sr.phase_seconds.get("scene cuts", 0.0) > 0.0
    assert _records(out) == rec["a"] + rec["b"]
    out2 = str(tmp_path / "out_grid.y4m")
    _plugin_run(plugin, monkeypatch, paths["ab"], out2, context=N, scene_split=False)
    assert _records(out2) != rec["a"] + rec["b"], "the fixed grid feeds frames of the other scene to the attention"


def test_several_ranks_are_refused_before_a_frame_is_read(built_lib, gpu_device, plugin, monkeypatch):
    class FakeDist:
        @staticmethod
        def get_world_size():
            return 2

        @staticmethod
        def get_rank():
            return 0

    class Source:
        reads = 0

        def info(self):
            Source.reads += 1
            raise AssertionError("the source was opened")

        read = info

    monkeypatch.setattr(plugin, "_distributed", lambda: FakeDist)
    plugin.video_path = Source()
    for opts in ({"context": 5, "scene_split": False}, {"context": 0, "scene_split": True}):
        plugin.context, plugin.scene_split = opts["context"], opts["scene_split"]
        plugin(input_mask=_mask_and_areas()[0])
        assert isinstance(plugin.last_error, RuntimeError) and "one process" in str(plugin.last_error)
    assert Source.reads == 0
    plugin.context, plugin.scene_split = 13, False        # more than clip_gap = 12
    monkeypatch.setattr(plugin, "_distributed", lambda: None)
    plugin(input_mask=_mask_and_areas()[0])
    assert isinstance(plugin.last_error, ValueError) and Source.reads == 0
