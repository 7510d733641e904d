"""--borrow at plugin level (backend/tools/borrow.py inside tools/seam_feather.plugin_call / device_call): the frames equal the statements
in the order of the chain

    out == key(borrow(fill, src, C, rows, T, B), src, C, T)                                             tests/_borrow_statement.py
    out == feather(key(borrow(regrain(deflicker(tone(fill)))))))                                        with the other five around it

exactly, for every mode's plugin call in the tensor and the list form and for sttn-auto's strip form; B = 0 is byte-identical to the
run without the option; the three loops of SubtitleRemover write the same file.  Under the synthetic weights the network fills lie far
from the source and little or nothing passes the threshold there: what those cases show is the wiring of the sets, the sample rows, y0
and the order in each mode.  The case that must borrow runs in opencv mode (Telea's fill of a smooth picture lies close to it) on a
still clip whose caption changes place inside one detected box, at plugin level and file to file through SubtitleRemover with a
stand-in detector; tests/_telea_statement.py says first that borrowed pixels exist."""
import numpy as np
import pytest
import torch

from tests import _borrow_statement as bs
from tests import _deflicker_statement as ds
from tests import _feather_statement as fs
from tests import _key_statement as ks
from tests import _regrain_statement as rs
from tests import _tone_statement as ts
from tests.test_gpu_seam_deflicker import still_file_clip
from tests.test_gpu_seam_feather import (N_BATCH, PER_WINDOW, call_device, call_list, config_values, geometry, make_detector, make_plugin,
                                         mask_of, run, write_source)
from tests.test_gpu_seam_regrain import noisy_clip
from vsr_amd.backend.tools.inpaint_tools import get_inpaint_area_by_mask, threshold_mask

pytestmark = pytest.mark.gpu

T, B = 12, 2
NAMES = ("VSR_SEAM_FEATHER", "VSR_REGRAIN", "VSR_DEFLICKER", "VSR_TONE_MATCH", "VSR_GLYPH_KEY", "VSR_GLYPH_HOLD", "VSR_BORROW")


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


def others_on(monkeypatch):
    monkeypatch.setenv("VSR_TONE_MATCH", "80")
    monkeypatch.setenv("VSR_DEFLICKER", "2")
    monkeypatch.setenv("VSR_REGRAIN", "100")
    monkeypatch.setenv("VSR_SEAM_FEATHER", "4")


def all_off(monkeypatch):
    for name in NAMES:
        monkeypatch.delenv(name, raising=False)


def still_clip(n, H, W, box, seed):
    """a smooth picture with grain of sigma 2 that stands still; a white caption block inside the box, at one place on the first half
    of the frames and at another on the second"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    base = (60 + 0.1 * x + 0.2 * y)[None, :, :, None] + np.zeros((n, 1, 1, 3))
    clip = np.rint(base + rng.normal(0, 2, base.shape))
    r0 = (box[0] + box[1]) // 2 - 3
    clip[:n // 2, r0:r0 + 6, box[2] + 40:box[2] + 70] = 255
    clip[n // 2:, r0:r0 + 6, box[3] - 90:box[3] - 60] = 255
    return np.clip(clip, 0, 255).astype(np.uint8), (slice(r0, r0 + 6), slice(box[2] + 40, box[2] + 70))


def six(fill, clip, C, rows):
    grained = rs.regrain(ds.deflicker(ts.tone(fill, clip, C, rows, 80), clip, C, rows, 2), clip, C, rows, 100)
    return fs.composite(ks.key(bs.borrow(grained, clip, C, rows, T, B), clip, C, T), clip, C, 4)


def test_device_call_with_a_prepared_fill(built_lib, gpu_device, monkeypatch):
    from vsr_amd.backend.tools import borrow, seam_feather

    all_off(monkeypatch)
    H, W, box = geometry("opencv")
    clip, _ = still_clip(6, H, W, box, seed=1)
    C = np.zeros((H, W), np.uint8)
    C[box[0]:box[1], box[2]:box[3]] = 255
    rng = np.random.default_rng(2)
    y, x = np.mgrid[0:H, 0:W]
    plain = np.clip(np.rint((60 + 0.1 * x + 0.2 * y)[None, :, :, None] + rng.normal(0, 2, clip.shape)), 0, 255).astype(np.uint8)
    fill = clip.copy()
    fill[:, C != 0] = plain[:, C != 0]
    fill_dev = torch.from_numpy(fill).to(gpu_device)

    def run(**kw):
        t = torch.from_numpy(clip).to(gpu_device)
        seam_feather.device_call(t, C, lambda d: d.copy_(fill_dev), kw.pop("feather", 0), sample_rows=(0, H), **kw)
        torch.cuda.synchronize()
        return t.cpu().numpy()

    info = {}
    lent = bs.borrow(fill, clip, C, (0, H), T, B, info=info)
    assert (info["lender"] >= 0).sum() > 1000, "the statement borrows"
    calls = borrow.stats["calls"]
    got = run(key=T, borrow=B)
    assert np.array_equal(got, ks.key(lent, clip, C, T)), f"{int((got != ks.key(lent, clip, C, T)).sum())} bytes differ from key(borrow(fill))"
    assert borrow.stats["calls"] == calls + 1
    assert np.array_equal(run(key=T, borrow=0), ks.key(fill, clip, C, T)) and np.array_equal(run(key=T), ks.key(fill, clip, C, T))
    assert np.array_equal(run(key=0, borrow=B), fill), "without a key the pass does not run"
    assert borrow.stats["calls"] == calls + 1
    got = run(feather=4, grain=100, flicker=2, tone=80, key=T, borrow=B)
    want = six(fill, clip, C, (0, H))
    assert np.array_equal(got, want), f"{int((got != want).sum())} bytes differ from feather(key(borrow(regrain(deflicker(tone(fill))))))"


def test_opencv_borrows_the_picture_behind_a_caption_that_changes_place(built_lib, gpu_device, plugins, monkeypatch):
    from vsr_amd.backend.tools import borrow

    all_off(monkeypatch)
    H, W, box = geometry("opencv")
    plugin = plugins("opencv")
    mask = mask_of("opencv")
    clip, first = still_clip(6, H, W, box, seed=3)
    fill = call_device(plugin, clip, mask, gpu_device)
    assert (fill != clip).any()
    C, rows = plugin.composite_mask(mask), plugin.sample_rows(mask)
    info = {}
    lent = bs.borrow(fill, clip, C, rows, T, B, info=info)
    want = ks.key(lent, clip, C, T)
    taken = info["lender"] >= 0
    print("borrowed pixels:", int(taken.sum()), "of", int(info["borrowers"].sum()), "borrowers; weights:", sorted(set(info["b"].values())))
    assert taken[2][first].all() and (info["lender"][2][first] >= 3).all(), "the statement borrows under the first caption's glyphs"
    monkeypatch.setenv("VSR_BORROW", "0")
    monkeypatch.setenv("VSR_GLYPH_KEY", str(T))
    calls = borrow.stats["calls"]
    keyed = call_device(plugin, clip, mask, gpu_device)
    assert np.array_equal(keyed, ks.key(fill, clip, C, T)) and borrow.stats["calls"] == calls, "B = 0: the run without the option"
    monkeypatch.delenv("VSR_BORROW")
    assert np.array_equal(call_device(plugin, clip, mask, gpu_device), keyed)
    monkeypatch.setenv("VSR_BORROW", str(B))
    got = call_device(plugin, clip, mask, gpu_device)
    assert np.array_equal(got, want), f"{int((got != want).sum())} bytes differ from the statement"
    assert np.array_equal(call_list(plugin, clip, mask), want), "the list form (a host body through cv2 or the device body) gives the same frames"
    assert borrow.stats["calls"] == calls + 2
    # under the first caption's glyphs frame 2 shows the source pixels of the frames behind the change
    lender = info["lender"][2][first]
    behind = np.stack([clip[s] for s in range(6)])[lender, np.mgrid[first][0], np.mgrid[first][1]]
    assert np.array_equal(got[2][first], behind) and not np.array_equal(got[2][first], clip[2][first])


@pytest.mark.parametrize("mode", ["sttn-det", "lama", "opencv", "propainter"])
def test_plugin_call_equals_the_statement(built_lib, gpu_device, plugins, monkeypatch, mode):
    """B = 2, T = 12 on the clips of tests/test_gpu_seam_key.py: the tensor and the list form equal key(borrow(fill)), and with the other
    four passes on the whole chain"""
    from vsr_amd.backend.tools import borrow

    H, W, box = geometry(mode)
    clip = noisy_clip(N_BATCH, H, W, box, seed=5, mode=mode)
    mask = mask_of(mode)
    plugin = plugins(mode)
    all_off(monkeypatch)
    fill = call_device(plugin, clip, mask, gpu_device)
    assert (fill != clip).any(), "the plugin fills something"
    C, rows = plugin.composite_mask(mask), plugin.sample_rows(mask)
    assert C.any() and rows == (0, H)
    monkeypatch.setenv("VSR_GLYPH_KEY", str(T))
    monkeypatch.setenv("VSR_BORROW", "0")
    calls = borrow.stats["calls"]
    keyed = call_device(plugin, clip, mask, gpu_device)
    assert np.array_equal(keyed, ks.key(fill, clip, C, T)) and borrow.stats["calls"] == calls, "B = 0 is the run without the option"
    monkeypatch.setenv("VSR_BORROW", str(B))
    info = {}
    want = ks.key(bs.borrow(fill, clip, C, rows, T, B, info=info), clip, C, T)
    print(mode, "borrowers:", int(info["borrowers"].sum()), "taken:", int((info["lender"] >= 0).sum()), "refused by N / threshold / closed:",
          info["refused_near"], info["refused_threshold"], info["refused_closed"], "weights:", sorted(set(info["b"].values())))
    assert info["borrowers"].any(), "the key would show fill somewhere: the pass has pixels to judge"
    got = call_device(plugin, clip, mask, gpu_device)
    assert np.array_equal(got, want), f"{mode}: {int((got != want).sum())} bytes differ from the statement"
    assert np.array_equal(got[:, C == 0], fill[:, C == 0]), "outside C the frame is what the plugin wrote"
    assert np.array_equal(call_list(plugin, clip, mask), want), "the list form gives the device form's frames"
    assert borrow.stats["calls"] == calls + 2
    others_on(monkeypatch)
    all_six = six(fill, clip, C, rows)
    got = call_device(plugin, clip, mask, gpu_device)
    assert np.array_equal(got, all_six), f"{mode}: {int((got != all_six).sum())} bytes differ from the chain of six"
    assert np.array_equal(call_list(plugin, clip, mask), all_six)


def test_sttn_auto(built_lib, gpu_device, plugins, monkeypatch):
    """STTNInpaint.__call__ (list form) and the strip-rows form of the chunk loops: the rows handed to the engine hold the rows of the
    composite mask and of the ring's hull, so they come back as the rows of the full-frame result"""
    from vsr_amd.backend.tools import borrow

    H, W, box = geometry("sttn-auto")
    plugin = plugins("sttn-auto")
    clip = noisy_clip(N_BATCH, H, W, box, seed=5)
    tall = np.zeros((H, W), np.uint8)
    tall[100:230, 60:380] = 255                                    # 130 rows, the strip has int(432 * 3 / 16) = 81
    for mask in (mask_of("sttn-auto"), tall):
        all_off(monkeypatch)
        fill = call_list(plugin, clip, mask)
        assert (fill != clip).any()
        C, rows = plugin.composite_mask(mask), plugin.sample_rows(mask)
        assert 0 < rows[0] < rows[1] <= H and not C[:rows[0]].any() and not C[rows[1]:].any()
        monkeypatch.setenv("VSR_GLYPH_KEY", str(T))
        monkeypatch.setenv("VSR_BORROW", str(B))
        calls = borrow.stats["calls"]
        info = {}
        want = ks.key(bs.borrow(fill, clip, C, rows, T, B, info=info), clip, C, T)
        assert info["borrowers"].any()
        got = call_list(plugin, clip, mask)
        assert np.array_equal(got, want), f"{int((got != want).sum())} bytes differ from the statement"
        assert borrow.stats["calls"] == calls + 1
        others_on(monkeypatch)
        all_six = six(fill, clip, C, rows)
        assert np.array_equal(call_list(plugin, clip, mask), all_six)
    # the rows form, on the tall mask (all six options still set)
    m = threshold_mask(tall)
    areas = get_inpaint_area_by_mask(W, H, int(W * 3 / 16), m)
    y_lo, y_hi = min(a[0] for a in areas), max(a[1] for a in areas)
    assert (y_lo, y_hi) == rows and 0 < y_lo and y_hi < H
    dmask = torch.from_numpy(np.ascontiguousarray(m[y_lo:y_hi, :, 0])).to(gpu_device)
    local = [(a[0] - y_lo, a[1] - y_lo, a[2], a[3]) for a in areas]
    strip = torch.from_numpy(np.ascontiguousarray(clip[:, y_lo:y_hi])).to(gpu_device)
    plugin.auto_chunk(strip, dmask, local, cmask=C, rows=(y_lo, y_hi), mask_host=m[y_lo:y_hi, :, 0])
    torch.cuda.synchronize()
    assert np.array_equal(strip.cpu().numpy(), all_six[:, y_lo:y_hi]), "strip rows: the full-frame definition"
    for name in NAMES[:4]:
        monkeypatch.delenv(name)
    strip = torch.from_numpy(np.ascontiguousarray(clip[:, y_lo:y_hi])).to(gpu_device)
    plugin.auto_chunk(strip, dmask, local, cmask=C, rows=(y_lo, y_hi), mask_host=m[y_lo:y_hi, :, 0])
    torch.cuda.synchronize()
    assert np.array_equal(strip.cpu().numpy(), want[:, y_lo:y_hi])
    own = ks.key(bs.borrow(fill[:, y_lo:y_hi], clip[:, y_lo:y_hi], C, rows, T, B, y0=y_lo), clip[:, y_lo:y_hi], C, T, y0=y_lo)
    assert np.array_equal(strip.cpu().numpy(), own), "and the strip's own statement"


# ---- file to file -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["sttn-det", "opencv"])
def test_every_loop_writes_the_same_file(built_lib, gpu_device, plugins, tmp_path, monkeypatch, mode):
    """T = 12, B = 2: the host-frame loop, the HBM-resident loop and resident windows (a budget of 2 x 10 frames) hand the plugin the same
    batches and write the same bytes.  In opencv mode these are not the bytes of a run with the options off; under the synthetic weights
    sttn-det's fill lies far from the source on every pixel, so that the key shows the fill everywhere, nothing is lent, and the bytes
    are those of the run with the options off: there the three loops must agree with that run too"""
    H, W, box = geometry(mode)
    src = str(tmp_path / "in.y4m")
    write_source(src, still_file_clip(H, W, box), monkeypatch)
    Det = make_detector(box)
    plugin = plugins(mode)
    gb = repr((2 * PER_WINDOW * H * W * 3 + 1024) / 2 ** 30)
    with config_values():
        all_off(monkeypatch)
        off, _ = run(src, str(tmp_path / "off.y4m"), plugin, Det(), monkeypatch, "1")
        monkeypatch.setenv("VSR_GLYPH_KEY", str(T))
        monkeypatch.setenv("VSR_BORROW", str(B))
        host, sr_host = run(src, str(tmp_path / "host.y4m"), plugin, Det(), monkeypatch, "0")
        resident, sr_res = run(src, str(tmp_path / "resident.y4m"), plugin, Det(), monkeypatch, "1")
        windows, sr_win = run(src, str(tmp_path / "windows.y4m"), plugin, Det(), monkeypatch, "windows", gb)
    assert "read + inpainting + write (host frames)" in sr_host.phase_seconds
    assert "read + inpainting + write (host frames)" not in sr_res.phase_seconds and sr_res.resident_windows is None
    assert sr_win.resident_windows is not None and len(sr_win.resident_windows["windows"]) >= 3
    assert host == resident == windows and len(resident) == len(off)
    assert (resident != off) if mode == "opencv" else (resident == off)


N_FILE, CHANGE = 16, 4


def caption_clip(H, W, box):
    """a still picture under grain of sigma 2 with a white caption of 8 x 60 pixels inside the box on every frame: at one place on the
    frames in front of CHANGE, at another from CHANGE on.  -> (clip, the first caption's rows and columns)"""
    rng = np.random.default_rng(31)
    y, x = np.mgrid[0:H, 0:W]
    base = (60 + 0.1 * x + 0.2 * y)[None, :, :, None] + np.zeros((N_FILE, 1, 1, 3))
    clip = np.rint(base + rng.normal(0, 2, base.shape))
    r0 = (box[0] + box[1]) // 2 - 4
    clip[:CHANGE, r0:r0 + 8, box[2] + 40:box[2] + 100] = 255
    clip[CHANGE:, r0:r0 + 8, box[3] - 110:box[3] - 50] = 255
    return np.clip(clip, 0, 255).astype(np.uint8), (slice(r0, r0 + 8), slice(box[2] + 40, box[2] + 100))


class Spy:
    """the plugin, keeping the frames and the mask of every call"""
    accepts_device_frames = True

    def __init__(self, plugin):
        self.plugin, self.calls = plugin, []

    def __call__(self, frames, mask, **kw):
        given = frames.cpu().numpy() if isinstance(frames, torch.Tensor) else np.stack(frames)
        self.calls.append((given.copy(), np.array(mask, copy=True)))
        return self.plugin(frames, mask, **kw)


def run_npy(src, out, plugin, det, monkeypatch, resident):
    """*.npy in and out: the lossless container, so that the written frames are the plugin's bytes"""
    from vsr_amd.backend.main import SubtitleRemover

    monkeypatch.setenv("VSR_IO_RESIDENT", resident)
    monkeypatch.delenv("VSR_RESIDENT_GB", raising=False)
    sr = SubtitleRemover(src, device="cuda:0")
    sr.sub_areas = [(0, sr.frame_height, 0, sr.frame_width)]
    sr.video_out_path = out
    sr.video_inpaint(None, plugin, text_detector=det)
    sr.video_writer.release()
    return np.load(out)


def test_a_run_borrows_across_a_caption_change_inside_one_box(built_lib, gpu_device, plugins, tmp_path, monkeypatch):
    """opencv mode through SubtitleRemover with a stand-in detector that answers with one box for both captions: one plugin call spans
    the change, and the written frames show, under the first caption's glyphs, the source pixels of the frames behind the change"""
    from tests import _telea_statement as tl

    H, W, box = geometry("opencv")
    clip, first = caption_clip(H, W, box)
    src = str(tmp_path / "in.npy")
    np.save(src, clip)
    Det = make_detector(box)
    plugin = plugins("opencv")
    with config_values():
        all_off(monkeypatch)
        spy = Spy(plugin)
        fill = run_npy(src, str(tmp_path / "off.npy"), spy, Det(), monkeypatch, "0")
        monkeypatch.setenv("VSR_GLYPH_KEY", str(T))
        keyed = run_npy(src, str(tmp_path / "key.npy"), Spy(plugin), Det(), monkeypatch, "0")
        monkeypatch.setenv("VSR_BORROW", str(B))
        lent_spy = Spy(plugin)
        got = run_npy(src, str(tmp_path / "borrow.npy"), lent_spy, Det(), monkeypatch, "0")
        resident = run_npy(src, str(tmp_path / "resident.npy"), Spy(plugin), Det(), monkeypatch, "1")
    assert got.shape == clip.shape and np.array_equal(got, resident), "the host-frame and the resident loop write the same frames"
    # one plugin call spans the change: its frames are the source's, CHANGE - 1 and CHANGE among them
    spans = [(given, mask) for given, mask in lent_spy.calls
             if any(np.array_equal(f, clip[CHANGE - 1]) for f in given) and any(np.array_equal(f, clip[CHANGE]) for f in given)]
    assert len(spans) == 1, [len(g) for g, _ in lent_spy.calls]
    given, mask = spans[0]
    lo = next(i for i in range(N_FILE) if np.array_equal(clip[i], given[0]))
    n = len(given)
    assert np.array_equal(given, clip[lo:lo + n]) and lo <= CHANGE - 1 and CHANGE < lo + n
    C, rows = plugin.composite_mask(mask), plugin.sample_rows(mask)
    assert C[first].all(), "the detected box holds both captions"
    # the Telea statement first: its fill of the last frame in front of the change lies within the threshold of the lender's source
    t = CHANGE - 1
    telea, _ = tl.serial(clip[t], C)
    assert np.abs(telea.astype(int) - clip[CHANGE])[first].max() < bs.TH, "borrowed pixels exist"
    info = {}
    want = ks.key(bs.borrow(fill[lo:lo + n], clip[lo:lo + n], C, rows, T, B, info=info), clip[lo:lo + n], C, T)
    lender = info["lender"][t - lo][first]
    print("call of", n, "frames from", lo, "; borrowed in it:", int((info["lender"] >= 0).sum()), "weights:", sorted(set(info["b"].values())))
    assert (lender >= CHANGE - lo).all(), "the statement: every glyph pixel of the first caption is lent by a frame behind the change"
    assert np.array_equal(got[lo:lo + n], want), "the written frames are the statement's"
    yy, xx = np.mgrid[first]
    behind = clip[lo:lo + n][lender, yy, xx]
    assert np.array_equal(got[t][first], behind), "under the first caption's glyphs: the source pixels of the frames behind the change"
    assert not np.array_equal(got[t][first], keyed[t][first]) and not np.array_equal(got[t][first], clip[t][first])
