"""--seam-feather at plugin and file level (backend/tools/seam_feather.py): for every mode the plugin call's frames equal the statement

    out == composite(fill, src, composite_mask(M), F)             tests/_feather_statement.py

exactly, where fill is the same plugin's output with the option off, in the same process; the device-tensor form and the list form
agree; with the option off nothing changes; the loops of SubtitleRemover write the same bytes; and the defect the option removes
(sttn-det rewriting its whole strip) is shown to be there without it.  Synthetic weights: what is shown is that the output equals the
definition, not what it looks like."""
import numpy as np
import pytest
import torch

from tests import _feather_statement as fs
from vsr_amd import synth
from vsr_amd.backend.tools import video_io
from vsr_amd.backend.tools.inpaint_tools import create_mask, get_inpaint_area_by_mask

pytestmark = pytest.mark.gpu

N_BATCH = 6
N, CUT = 34, 22
ON = [i for i in range(N) if 3 <= i < 15 or i >= 22]              # the frames of the file clip that carry the subtitle
PER_WINDOW = 10


def geometry(mode):
    """(H, W, box): RAFT wants strips of at least 128 rows, so propainter runs on the larger frame of the existing tests"""
    return (480, 852, (400, 450, 100, 760)) if mode == "propainter" else (240, 432, (180, 214, 60, 380))


def mask_of(mode):
    H, W, box = geometry(mode)
    if mode == "propainter":
        # columns 3..: the 4-fold dilation reaches the strip's first column (the strips are cut to a multiple of 8: columns 2 .. 850)
        m = np.zeros((H, W), np.uint8)
        m[box[0]:box[1], 3:box[3]] = 255
        return m
    return create_mask((H, W), [(box[2], box[3], box[0], box[1])])


def make_plugin(mode):
    if mode == "sttn-det":
        from vsr_amd.backend.inpaint.sttn_det_inpaint import STTNDetInpaint
        return STTNDetInpaint("cuda:0", {"netG": synth.make_state_dict(0, "det")})
    if mode == "sttn-auto":
        from vsr_amd.backend.inpaint.sttn_auto_inpaint import STTNInpaint
        return STTNInpaint("cuda:0", {"netG": synth.make_state_dict(0, "auto")})
    if mode == "lama":
        from vsr_amd.backend.inpaint.lama_inpaint import LamaInpaint
        return LamaInpaint("cuda:0", synth.make_lama_state_dict(3, 2))
    if mode == "opencv":
        from vsr_amd.backend.inpaint.opencv_inpaint import OpenCVInpaint
        return OpenCVInpaint("cuda:0")
    from vsr_amd.backend.inpaint.propainter_inpaint import PropainterInpaint
    plugin = PropainterInpaint("cuda:0", {"raft": synth.make_raft_state_dict(0), "rfc": synth.make_rfc_state_dict(0),
                                          "propainter": synth.make_propainter_state_dict(0)})
    plugin.raft_iter = 4
    return plugin


_plugins = {}


@pytest.fixture(scope="module")
def plugins(built_lib, gpu_device):
    """one plugin per mode for the whole module, built on first use"""
    def get(mode):
        if mode not in _plugins:
            _plugins[mode] = make_plugin(mode)
        return _plugins[mode]

    yield get
    for p in _plugins.values():
        if hasattr(p, "close"):
            p.close()
    _plugins.clear()


def call_device(plugin, clip, mask, dev, **kw):
    t = torch.from_numpy(np.ascontiguousarray(clip)).to(dev)
    out = plugin(t, mask, **kw)
    torch.cuda.synchronize()
    assert out.data_ptr() == t.data_ptr(), "the device form works in place"
    return t.cpu().numpy()


def call_list(plugin, clip, mask, **kw):
    frames = [f.copy() for f in clip]
    out = plugin(frames, mask, **kw)
    assert all(np.array_equal(a, b) for a, b in zip(frames, clip)), "the list inputs are unmutated"
    assert all(o is not f for o, f in zip(out, frames))
    return np.stack(out)


@pytest.mark.parametrize("mode", ["sttn-det", "lama", "opencv", "propainter"])
def test_plugin_call_equals_the_statement(built_lib, gpu_device, plugins, monkeypatch, mode):
    H, W, box = geometry(mode)
    clip = synth.make_clip(N_BATCH, H, W, box, seed=5)
    mask = mask_of(mode)
    plugin = plugins(mode)
    captured = []
    if mode == "propainter":
        from vsr_amd.backend.inpaint import propainter_inpaint as pp

        real = pp.read_mask

        def spy(m, *a, **kw):
            out = real(m, *a, **kw)
            captured.append(out[1])
            return out

        monkeypatch.setattr(pp, "read_mask", spy)
    monkeypatch.delenv("VSR_SEAM_FEATHER", raising=False)
    fill = call_device(plugin, clip, mask, gpu_device)
    blended_under = list(captured)
    assert (fill != clip).any(), "the plugin fills something"
    monkeypatch.setenv("VSR_SEAM_FEATHER", "0")
    assert np.array_equal(call_device(plugin, clip, mask, gpu_device), fill), "F = 0 is off"
    assert np.array_equal(call_list(plugin, clip, mask), fill), "the two forms agree with the option off"
    C = plugin.composite_mask(mask)
    assert np.array_equal(C, fs.composite_mask(mode, mask)) and C.any()
    if mode == "propainter":
        # C is the `md` array inpaint() blended under, put back at its strip
        areas = get_inpaint_area_by_mask(W, H, int(W * 3 / 16), mask[:, :, None], multiple=8)
        assert len(areas) == len(blended_under) >= 1
        placed = np.zeros((H, W), np.uint8)
        for (y0, y1, x0, x1), md in zip(areas, blended_under):
            placed[y0:y1, x0:x1] |= md
            assert md[:, 0].any(), "the dilation reaches the strip's first column"
        assert np.array_equal(C, placed)
    for F in (1, 8):
        monkeypatch.setenv("VSR_SEAM_FEATHER", str(F))
        want = fs.composite(fill, clip, C, F)
        got = call_device(plugin, clip, mask, gpu_device)
        assert np.array_equal(got, want), f"{mode} F={F}: {int((got != want).sum())} bytes differ from the statement"
        assert np.array_equal(got[:, C == 0], clip[:, C == 0]), "outside C the frame is the source, bit for bit"
    assert np.array_equal(call_list(plugin, clip, mask), want), "the list form gives the device form's frames"
    assert not np.array_equal(want, fill)


def test_sttn_det_rewrites_its_strip_and_f1_does_not(built_lib, gpu_device, plugins, monkeypatch):
    """The defect being removed: with the option off sttn-det changes pixels outside C (the whole strip goes through 432 x 240 and
    back); with F = 1 every pixel outside C is the source's.  The fixture was chosen with the reference's own arithmetic
    (oracle/sttn_det.py on the CPU, same clip, mask and weights): it changes pixels outside C as well."""
    H, W, box = geometry("sttn-det")
    clip = synth.make_clip(N_BATCH, H, W, box, seed=5)
    mask = mask_of("sttn-det")
    plugin = plugins("sttn-det")
    C = plugin.composite_mask(mask)
    monkeypatch.delenv("VSR_SEAM_FEATHER", raising=False)
    fill = call_device(plugin, clip, mask, gpu_device)
    assert (fill[:, C == 0] != clip[:, C == 0]).any(), "option off: the strip is rewritten outside the mask"
    monkeypatch.setenv("VSR_SEAM_FEATHER", "1")
    got = call_device(plugin, clip, mask, gpu_device)
    assert np.array_equal(got[:, C == 0], clip[:, C == 0])
    assert np.array_equal(got[:, C != 0], fill[:, C != 0])


def test_sttn_det_context_frames_take_no_part(built_lib, gpu_device, plugins, monkeypatch):
    H, W, box = geometry("sttn-det")
    clip = synth.make_clip(N_BATCH + 3, H, W, box, seed=5)
    ctx, batch = clip[:3], clip[3:]
    mask = mask_of("sttn-det")
    plugin = plugins("sttn-det")
    C = plugin.composite_mask(mask)
    monkeypatch.delenv("VSR_SEAM_FEATHER", raising=False)
    ctx_dev = torch.from_numpy(np.ascontiguousarray(ctx)).to(gpu_device)
    fill = call_device(plugin, batch, mask, gpu_device, context=ctx_dev)
    assert not np.array_equal(fill, call_device(plugin, batch, mask, gpu_device)), "the context changes the fill"
    monkeypatch.setenv("VSR_SEAM_FEATHER", "8")
    got = call_device(plugin, batch, mask, gpu_device, context=ctx_dev)
    assert np.array_equal(ctx_dev.cpu().numpy(), ctx), "the context is read-only and is not composited"
    want = fs.composite(fill, batch, C, 8)
    assert np.array_equal(got, want)
    assert np.array_equal(call_list(plugin, batch, mask, context=[f.copy() for f in ctx]), want)


def test_sttn_auto(built_lib, gpu_device, plugins, monkeypatch):
    """STTNInpaint.__call__ (list form) against the statement; F = 1 is byte-identical to off (its blend is mask-exact already); and
    the strip-rows form of the chunk loops: a mask taller than its strip touches the strip's first and last row, d comes from the
    full frame, so the rows handed to the engine come back as the rows of the full-frame result."""
    H, W, box = geometry("sttn-auto")
    plugin = plugins("sttn-auto")
    clip = synth.make_clip(N_BATCH, H, W, box, seed=5)
    tall = np.zeros((H, W), np.uint8)
    tall[100:230, 60:380] = 255                                    # 130 rows, the strip has int(432 * 3 / 16) = 81
    for mask in (mask_of("sttn-auto"), tall):
        monkeypatch.delenv("VSR_SEAM_FEATHER", raising=False)
        fill = call_list(plugin, clip, mask)
        assert (fill != clip).any()
        C = plugin.composite_mask(mask)
        assert np.array_equal(C, fs.composite_mask("sttn-auto", mask)) and C.any()
        monkeypatch.setenv("VSR_SEAM_FEATHER", "1")
        assert np.array_equal(call_list(plugin, clip, mask), fill), "F = 1: byte-identical to off"
        monkeypatch.setenv("VSR_SEAM_FEATHER", "8")
        got = call_list(plugin, clip, mask)
        want = fs.composite(fill, clip, C, 8)
        assert np.array_equal(got, want)
        assert not np.array_equal(got, fill)
    # the rows form, on the tall mask (F = 8 still set)
    from vsr_amd.backend.tools.inpaint_tools import threshold_mask

    m = threshold_mask(tall)
    areas = get_inpaint_area_by_mask(W, H, int(W * 3 / 16), m)
    y_lo, y_hi = min(a[0] for a in areas), max(a[1] for a in areas)
    assert C[y_lo].any() and C[y_hi - 1].any() and 0 < y_lo and y_hi < H, "the mask touches the strip's first and last row"
    rows = torch.from_numpy(np.ascontiguousarray(clip[:, y_lo:y_hi])).to(gpu_device)
    dmask = torch.from_numpy(np.ascontiguousarray(m[y_lo:y_hi, :, 0])).to(gpu_device)
    local = [(a[0] - y_lo, a[1] - y_lo, a[2], a[3]) for a in areas]
    plugin.auto_chunk(rows, dmask, local, cmask=C, rows=(y_lo, y_hi), mask_host=m[y_lo:y_hi, :, 0])
    torch.cuda.synchronize()
    assert np.array_equal(rows.cpu().numpy(), want[:, y_lo:y_hi]), "strip rows: the full-frame definition"


def test_lama_single_frame(built_lib, gpu_device, plugins, monkeypatch):
    """LamaInpaint.inpaint: the single picture and propainter's single-frame fall-back"""
    H, W, box = geometry("lama")
    frame = synth.make_clip(1, H, W, box, seed=9)[0]
    mask = mask_of("lama")
    plugin = plugins("lama")
    monkeypatch.delenv("VSR_SEAM_FEATHER", raising=False)
    keep = frame.copy()
    fill = plugin.inpaint(frame, mask)
    monkeypatch.setenv("VSR_SEAM_FEATHER", "8")
    got = plugin.inpaint(frame, mask)
    assert np.array_equal(frame, keep)
    assert np.array_equal(got, fs.composite(fill[None], frame[None], plugin.composite_mask(mask), 8)[0])


# ---- file to file -------------------------------------------------------------------------------------------------------------------
def make_clip(H, W, box):
    """two subtitle intervals with a gap; from frame CUT on the background is inverted (the glyph blocks stay)"""
    clip = synth.make_clip(N, H, W, box, seed=5)
    plain = synth.make_clip(N, H, W, (0, 1, 0, 1), seed=5)
    for i in range(N):
        if i not in ON:
            clip[i] = plain[i]
    for i in range(CUT, N):
        glyph = (clip[i] != plain[i]).any(axis=-1, keepdims=True)
        clip[i] = np.where(glyph, clip[i], 255 - clip[i])
    return clip


def write_source(path, clip, monkeypatch):
    _, H, W, _ = clip.shape
    monkeypatch.setenv("VSR_IO_COLOR", "host")
    w = video_io.Y4mWriter(path, 25.0, (W, H), chroma="420")
    for f in clip:
        w.write(f)
    w.release()
    monkeypatch.setenv("VSR_IO_COLOR", "device")


def make_detector(box):
    quad = np.array([[[box[2], box[0]], [box[3], box[0]], [box[3], box[1]], [box[2], box[1]]]])

    class Det:                                             # the reference's host signature
        batch_size = 4

        def predict(self, img):
            white = (img[box[0] + 8:box[1] - 8, box[2] + 8:box[3] - 8] > 200).mean()
            return [{"dt_polys": quad if white > 0.05 else np.zeros((0, 4, 2), np.int32)}]

    return Det


class config_values:
    """batches of at most 8 frames (so that windows of ten can hold them), put back afterwards"""

    def __enter__(self):
        from vsr_amd.backend.config import config

        self.keys = {"sttnMaxLoadNum": 8, "sttnNeighborStride": 1, "sttnReferenceLength": 6}
        self.old = {k: getattr(config, k).value for k in self.keys}
        for k, v in self.keys.items():
            getattr(config, k).value = v

    def __exit__(self, *exc):
        from vsr_amd.backend.config import config

        for k, v in self.old.items():
            getattr(config, k).value = v


class Recording:
    """the plugin, keeping the masks it is called with"""
    accepts_device_frames = True

    def __init__(self, plugin):
        self.plugin, self.masks = plugin, []
        self.accepts_context = getattr(plugin, "accepts_context", False)

    def __call__(self, frames, mask, **kw):
        self.masks.append(np.array(mask, copy=True))
        return self.plugin(frames, mask, **kw)


def run(src, out, plugin, det, monkeypatch, resident, gb=None):
    from vsr_amd.backend.main import SubtitleRemover

    monkeypatch.setenv("VSR_IO_COLOR", "device")
    monkeypatch.setenv("VSR_IO_RESIDENT", resident)
    if gb is None:
        monkeypatch.delenv("VSR_RESIDENT_GB", raising=False)
    else:
        monkeypatch.setenv("VSR_RESIDENT_GB", gb)
    sr = SubtitleRemover(src, device="cuda:0")
    sr.sub_areas = [(0, sr.frame_height, 0, sr.frame_width)]
    sr.video_out_path = out
    sr.video_inpaint(None, plugin, text_detector=det)
    sr.video_writer.release()
    return open(out, "rb").read(), sr


@pytest.mark.parametrize("mode", ["sttn-det", "opencv"])
def test_every_loop_writes_the_same_file(built_lib, gpu_device, plugins, tmp_path, monkeypatch, mode):
    """F = 8: the host-frame loop, the HBM-resident loop and resident windows (a budget of 2 x 10 frames) write the same bytes, and
    not the bytes of a run with the option off"""
    H, W, box = geometry(mode)
    src = str(tmp_path / "in.y4m")
    write_source(src, make_clip(H, W, box), monkeypatch)
    Det = make_detector(box)
    plugin = plugins(mode)
    gb = repr((2 * PER_WINDOW * H * W * 3 + 1024) / 2 ** 30)
    with config_values():
        monkeypatch.delenv("VSR_SEAM_FEATHER", raising=False)
        off, _ = run(src, str(tmp_path / "off.y4m"), plugin, Det(), monkeypatch, "1")
        monkeypatch.setenv("VSR_SEAM_FEATHER", "8")
        host, sr_host = run(src, str(tmp_path / "host.y4m"), plugin, Det(), monkeypatch, "0")
        resident, sr_res = run(src, str(tmp_path / "resident.y4m"), plugin, Det(), monkeypatch, "1")
        windows, sr_win = run(src, str(tmp_path / "windows.y4m"), plugin, Det(), monkeypatch, "windows", gb)
    assert "read + inpainting + write (host frames)" in sr_host.phase_seconds
    assert "read + inpainting + write (host frames)" not in sr_res.phase_seconds and sr_res.resident_windows is None
    assert sr_win.resident_windows is not None and len(sr_win.resident_windows["windows"]) >= 3
    assert host == resident == windows
    assert resident != off and len(resident) == len(off)


def luma_records(path, H, W):
    data = open(path, "rb").read()
    pos = data.index(b"\n") + 1
    rec = H * W + 2 * ((H + 1) // 2) * ((W + 1) // 2)
    out = []
    while pos < len(data):
        assert data[pos:pos + 6] == b"FRAME\n"
        pos += 6
        out.append(np.frombuffer(data, np.uint8, H * W, pos).reshape(H, W))
        pos += rec
    return np.stack(out)


def test_source_format_output_keeps_every_luma_sample_outside_the_mask(built_lib, gpu_device, plugins, tmp_path, monkeypatch):
    """VSR_Y4M_OUT=source, a 4:2:0 source, sttn-det: with F = 1 every luma sample outside C is the input file's byte; with the option
    off the same comparison fails (the strip was rewritten, its samples re-encoded)"""
    H, W, box = geometry("sttn-det")
    src = str(tmp_path / "in.y4m")
    write_source(src, make_clip(H, W, box), monkeypatch)
    monkeypatch.setenv("VSR_Y4M_OUT", "source")
    Det = make_detector(box)
    plugin = Recording(plugins("sttn-det"))
    with config_values():
        monkeypatch.delenv("VSR_SEAM_FEATHER", raising=False)
        run(src, str(tmp_path / "off.y4m"), plugin, Det(), monkeypatch, "1")
        monkeypatch.setenv("VSR_SEAM_FEATHER", "1")
        run(src, str(tmp_path / "f1.y4m"), plugin, Det(), monkeypatch, "1")
    assert open(str(tmp_path / "f1.y4m"), "rb").readline() == open(src, "rb").readline(), "the source's format"
    assert plugin.masks
    C = np.zeros((H, W), bool)
    for m in plugin.masks:
        C |= plugin.plugin.composite_mask(m) != 0
    assert C.any() and not C.all()
    source, off, f1 = (luma_records(str(tmp_path / name), H, W) for name in ("in.y4m", "off.y4m", "f1.y4m"))
    assert len(source) == len(off) == len(f1) == N
    assert np.array_equal(f1[:, ~C], source[:, ~C]), "F = 1: every luma sample outside C is the input file's byte"
    assert (f1[:, C] != source[:, C]).any(), "something was inpainted"
    assert (off[:, ~C] != source[:, ~C]).any(), "option off: luma samples outside C were re-encoded"
