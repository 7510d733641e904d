"""--borrow-pan at plugin level (backend/tools/borrow.py inside tools/seam_feather.plugin_call / device_call): the frames equal the
statements in the order of the chain, the pass in its unchanged place

    out == key(borrow_pan(fill, src, C, rows, T, B, P), src, C, T)                                  tests/_borrow_pan_statement.py
    out == feather(key(borrow_pan(regrain(deflicker(tone(fill)))))))                                with the other five around it

exactly; P = 0 is byte-identical to the run without the option; one network mode and sttn-auto's strip form show the wiring (under the
synthetic weights their fills lie far from the source and little passes the threshold).  The case that must borrow runs in opencv mode
on a clip that pans by 6 columns per frame over soft vertical stripes -- Telea carries them across the low box, a shift of 6 columns
moves a sample of the ring by about 9 levels, so that every pair of the plain pass is closed -- with a caption that changes place
inside one detected box: at plugin level and file to file through SubtitleRemover with a stand-in detector, after
tests/_telea_statement.py has said that the fill lies within the lender's threshold.  (Stripes say nothing about dy: whichever row the
search settles on shows the same picture, and the statement and the kernels settle on the same one.)"""
import functools

import numpy as np
import pytest
import torch

from tests import _borrow_pan_statement as ps
from tests import _borrow_statement as bs
from tests import _deflicker_statement as ds
from tests import _feather_statement as fs
from tests import _key_statement as ks
from tests import _regrain_statement as rs
from tests import _tone_statement as ts
from tests.test_gpu_seam_borrow import Spy, run_npy
from tests.test_gpu_seam_feather import N_BATCH, call_device, call_list, config_values, geometry, make_detector, make_plugin, mask_of
from vsr_amd.backend.tools.inpaint_tools import get_inpaint_area_by_mask, threshold_mask

pytestmark = pytest.mark.gpu

T, B, PAN, STEP = 12, 2, 8, 6
NAMES = ("VSR_SEAM_FEATHER", "VSR_REGRAIN", "VSR_DEFLICKER", "VSR_TONE_MATCH", "VSR_GLYPH_KEY", "VSR_GLYPH_HOLD", "VSR_BORROW", "VSR_BORROW_PAN")
N_FILE, CHANGE = 16, 4

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


def all_off(monkeypatch):
    for name in NAMES:
        monkeypatch.delenv(name, raising=False)


def others_on(monkeypatch):
    monkeypatch.setenv("VSR_TONE_MATCH", "80")
    monkeypatch.setenv("VSR_DEFLICKER", "2")
    monkeypatch.setenv("VSR_REGRAIN", "100")
    monkeypatch.setenv("VSR_SEAM_FEATHER", "4")


def stripes(n, H, W, seed):
    """soft vertical stripes under grain of sigma 2: what frame t shows at column x, frame t + 1 shows at column x + STEP"""
    rng = np.random.default_rng(seed)
    wave = 90 + 60 * np.sin(2 * np.pi * np.arange(W + STEP * n) / 160.0)
    clean = np.stack([np.broadcast_to(wave[STEP * (n - 1 - t):STEP * (n - 1 - t) + W], (H, W)) for t in range(n)])[..., None]
    return clean + np.zeros((1, 1, 1, 3)), rng


def pan_clip(n, H, W, box, seed, change, cap):
    """a white caption of cap = (rows, columns) inside the box, at one place on the frames in front of `change`, at another from there on
    -> (clip, the first caption's rows and columns)"""
    clean, rng = stripes(n, H, W, seed)
    clip = np.rint(clean + rng.normal(0, 2, clean.shape))
    r0 = (box[0] + box[1]) // 2 - cap[0] // 2
    first = (slice(r0, r0 + cap[0]), slice(box[2] + 40, box[2] + 40 + cap[1]))
    clip[:change, first[0], first[1]] = 255
    clip[change:, first[0], box[3] - 50 - cap[1]:box[3] - 50] = 255
    return np.clip(clip, 0, 255).astype(np.uint8), first


def six(fill, clip, C, rows, p=PAN):
    grained = rs.regrain(ds.deflicker(ts.tone(fill, clip, C, rows, 80), clip, C, rows, 2), clip, C, rows, 100)
    return fs.composite(ks.key(ps.borrow_pan(grained, clip, C, rows, T, B, p), clip, C, T), clip, C, 4)


@functools.lru_cache(maxsize=None)
def file_clip():
    H, W, box = geometry("opencv")
    return pan_clip(N_FILE, H, W, box, 31, CHANGE, (8, 60))


@functools.lru_cache(maxsize=None)
def telea_says_borrowed_pixels_exist():
    """the Telea statement on the last frame in front of the change: under the first caption its fill lies within the threshold of the
    next frame's source STEP columns on"""
    from tests import _telea_statement as tl

    H, W, box = geometry("opencv")
    clip, first = file_clip()
    C = np.zeros((H, W), np.uint8)
    C[box[0]:box[1], box[2]:box[3]] = 255
    telea, _ = tl.serial(clip[CHANGE - 1], C)
    there = (first[0], slice(first[1].start + STEP, first[1].stop + STEP))
    return int(np.abs(telea[first].astype(int) - clip[CHANGE][there]).max())


def test_device_call_with_a_prepared_fill(built_lib, gpu_device, monkeypatch):
    from vsr_amd.backend.tools import borrow, seam_feather

    all_off(monkeypatch)
    H, W, box = geometry("opencv")
    clip, _ = pan_clip(6, H, W, box, 1, 3, (6, 30))
    C = np.zeros((H, W), np.uint8)
    C[box[0]:box[1], box[2]:box[3]] = 255
    clean, rng = stripes(6, H, W, 2)
    plain = np.clip(np.rint(clean + rng.normal(0, 2, clean.shape)), 0, 255).astype(np.uint8)
    fill = clip.copy()
    fill[:, C != 0] = plain[:, C != 0]
    fill_dev = torch.from_numpy(fill).to(gpu_device)

    def run(**kw):
        t = torch.from_numpy(clip).to(gpu_device)
        seam_feather.device_call(t, C, lambda d: d.copy_(fill_dev), kw.pop("feather", 0), sample_rows=(0, H), **kw)
        torch.cuda.synchronize()
        return t.cpu().numpy()

    info, still = {}, {}
    lent = ps.borrow_pan(fill, clip, C, (0, H), T, B, PAN, info=info)
    assert np.array_equal(bs.borrow(fill, clip, C, (0, H), T, B, info=still), fill) and set(still["b"].values()) == {0}, "the plain pass: closed"
    assert (info["lender"] >= 0).sum() > 1000 and all(d[1] == STEP * k for (t, k), d in info["D"].items()), "the statement follows the pan"
    calls = dict(borrow.stats)
    without = run(key=T, borrow=B)
    assert np.array_equal(without, ks.key(fill, clip, C, T)), "no P: the plain pass, which lends nothing here"
    monkeypatch.setenv("VSR_BORROW_PAN", "0")
    assert np.array_equal(run(key=T, borrow=B), without), "P = 0 is the run without the option"
    assert borrow.stats["calls"] == calls["calls"] + 2 and borrow.stats["pan_calls"] == calls["pan_calls"]
    monkeypatch.setenv("VSR_BORROW_PAN", str(PAN))
    got = run(key=T, borrow=B)
    want = ks.key(lent, clip, C, T)
    assert np.array_equal(got, want), f"{int((got != want).sum())} bytes differ from key(borrow_pan(fill))"
    assert borrow.stats["pan_calls"] == calls["pan_calls"] + 1 and not np.array_equal(got, without)
    assert np.array_equal(run(key=T, borrow=0), without) and np.array_equal(run(key=0, borrow=B), fill), "without B or T the pass does not run"
    assert borrow.stats["pan_calls"] == calls["pan_calls"] + 1
    got = run(feather=4, grain=100, flicker=2, tone=80, key=T, borrow=B)
    want = six(fill, clip, C, (0, H))
    assert np.array_equal(got, want), f"{int((got != want).sum())} bytes differ from feather(key(borrow_pan(regrain(deflicker(tone(fill))))))"


def test_opencv_borrows_along_a_pan(built_lib, gpu_device, plugins, monkeypatch):
    from vsr_amd.backend.tools import borrow

    all_off(monkeypatch)
    assert telea_says_borrowed_pixels_exist() < bs.TH, "borrowed pixels exist"
    H, W, box = geometry("opencv")
    plugin = plugins("opencv")
    mask = mask_of("opencv")
    whole, first = file_clip()
    lo = CHANGE - 3
    clip = whole[lo:lo + 6]
    fill = call_device(plugin, clip, mask, gpu_device)
    assert (fill != clip).any()
    C, rows = plugin.composite_mask(mask), plugin.sample_rows(mask)
    info, still = {}, {}
    want = ks.key(ps.borrow_pan(fill, clip, C, rows, T, B, PAN, info=info), clip, C, T)
    plain = ks.key(bs.borrow(fill, clip, C, rows, T, B, info=still), clip, C, T)
    taken = info["lender"] >= 0
    print("borrowed pixels:", int(taken.sum()), "of", int(info["borrowers"].sum()), "borrowers; D:", info["D"], "the plain pass:",
          int((still["lender"] >= 0).sum()), sorted(set(still["b"].values())))
    assert set(still["b"].values()) == {0} and not (still["lender"] >= 0).any(), "the plain pass: every pair is closed"
    assert taken[2][first].all() and (info["lender"][2][first] >= 3).all(), "the statement borrows under the first caption's glyphs"
    monkeypatch.setenv("VSR_GLYPH_KEY", str(T))
    monkeypatch.setenv("VSR_BORROW", str(B))
    calls = borrow.stats["pan_calls"]
    got_plain = call_device(plugin, clip, mask, gpu_device)
    assert np.array_equal(got_plain, plain) and np.array_equal(got_plain, ks.key(fill, clip, C, T)), "plain --borrow shows the fill"
    monkeypatch.setenv("VSR_BORROW_PAN", "0")
    assert np.array_equal(call_device(plugin, clip, mask, gpu_device), got_plain) and borrow.stats["pan_calls"] == calls
    monkeypatch.setenv("VSR_BORROW_PAN", str(PAN))
    got = call_device(plugin, clip, mask, gpu_device)
    assert np.array_equal(got, want), f"{int((got != want).sum())} bytes differ from the statement"
    assert np.array_equal(call_list(plugin, clip, mask), want), "the list form gives the same frames"
    assert borrow.stats["pan_calls"] == calls + 2
    # under the first caption's glyphs frame 2 shows the shifted source pixels of the frames behind the change
    lender, q = info["lender"][2][first], info["q"][2][first]
    behind = clip[lender, q[..., 0], q[..., 1]]
    assert (q[..., 1] == np.mgrid[first][1] + STEP * (lender - 2)).all()
    assert np.array_equal(got[2][first], behind) and not np.array_equal(got[2][first], got_plain[2][first])
    assert not np.array_equal(got[2][first], clip[2][first])


def test_the_wiring_in_a_network_mode_and_in_strip_form(built_lib, gpu_device, plugins, monkeypatch):
    """sttn-det's plugin call in the tensor and the list form, STTNInpaint.__call__ and the strip-rows form of sttn-auto's chunk loops
    (y0 > 0), alone and inside the chain of six"""
    from vsr_amd.backend.tools import borrow

    for mode in ("sttn-det", "sttn-auto"):
        H, W, box = geometry(mode)
        plugin = plugins(mode)
        clip, _ = pan_clip(N_BATCH, H, W, box, 5, N_BATCH // 2, (6, 30))
        mask = np.zeros((H, W), np.uint8)
        if mode == "sttn-auto":
            mask[100:230, 60:380] = 255                            # 130 rows, the strip has int(432 * 3 / 16) = 81
        else:
            mask = mask_of(mode)
        call = (lambda: call_list(plugin, clip, mask)) if mode == "sttn-auto" else (lambda: call_device(plugin, clip, mask, gpu_device))
        all_off(monkeypatch)
        fill = call()
        assert (fill != clip).any()
        C, rows = plugin.composite_mask(mask), plugin.sample_rows(mask)
        monkeypatch.setenv("VSR_GLYPH_KEY", str(T))
        monkeypatch.setenv("VSR_BORROW", str(B))
        monkeypatch.setenv("VSR_BORROW_PAN", str(PAN))
        calls = borrow.stats["pan_calls"]
        info = {}
        want = ks.key(ps.borrow_pan(fill, clip, C, rows, T, B, PAN, info=info), clip, C, T)
        print(mode, "borrowers:", int(info["borrowers"].sum()), "taken:", int((info["lender"] >= 0).sum()), "D:", sorted(set(info["D"].values())))
        assert info["borrowers"].any() and any(d != (0, 0) for d in info["D"].values())
        got = call()
        assert np.array_equal(got, want), f"{mode}: {int((got != want).sum())} bytes differ from the statement"
        assert borrow.stats["pan_calls"] == calls + 1
        if mode == "sttn-det":
            assert np.array_equal(call_list(plugin, clip, mask), want), "the list form gives the device form's frames"
        others_on(monkeypatch)
        all_six = six(fill, clip, C, rows)
        assert np.array_equal(call(), all_six), f"{mode}: the chain of six"
    # the rows form, on sttn-auto's tall mask
    m = threshold_mask(mask)
    areas = get_inpaint_area_by_mask(W, H, int(W * 3 / 16), m)
    y_lo, y_hi = min(a[0] for a in areas), max(a[1] for a in areas)
    assert (y_lo, y_hi) == rows and 0 < y_lo and y_hi < H
    dmask = torch.from_numpy(np.ascontiguousarray(m[y_lo:y_hi, :, 0])).to(gpu_device)
    local = [(a[0] - y_lo, a[1] - y_lo, a[2], a[3]) for a in areas]
    for name in NAMES[:4]:
        monkeypatch.delenv(name)
    strip = torch.from_numpy(np.ascontiguousarray(clip[:, y_lo:y_hi])).to(gpu_device)
    plugin.auto_chunk(strip, dmask, local, cmask=C, rows=(y_lo, y_hi), mask_host=m[y_lo:y_hi, :, 0])
    torch.cuda.synchronize()
    own = ks.key(ps.borrow_pan(fill[:, y_lo:y_hi], clip[:, y_lo:y_hi], C, rows, T, B, PAN, y0=y_lo), clip[:, y_lo:y_hi], C, T, y0=y_lo)
    assert np.array_equal(strip.cpu().numpy(), own), "strip rows: the strip's own statement (V and q end at the rows held)"


def test_a_run_borrows_along_a_pan_across_a_caption_change(built_lib, gpu_device, plugins, tmp_path, monkeypatch):
    """opencv mode through SubtitleRemover, *.npy in and out, with a stand-in detector that answers with one box for both captions: one
    plugin call spans the change, and the written frames show, under the first caption's glyphs, the shifted source pixels of the frames
    behind the change, where plain --borrow writes the fill"""
    assert telea_says_borrowed_pixels_exist() < bs.TH, "borrowed pixels exist"
    H, W, box = geometry("opencv")
    clip, first = file_clip()
    src = str(tmp_path / "in.npy")
    np.save(src, clip)
    Det = make_detector(box)
    plugin = plugins("opencv")
    with config_values():
        all_off(monkeypatch)
        fill = run_npy(src, str(tmp_path / "off.npy"), Spy(plugin), Det(), monkeypatch, "0")
        monkeypatch.setenv("VSR_GLYPH_KEY", str(T))
        monkeypatch.setenv("VSR_BORROW", str(B))
        plain = run_npy(src, str(tmp_path / "plain.npy"), Spy(plugin), Det(), monkeypatch, "0")
        monkeypatch.setenv("VSR_BORROW_PAN", "0")
        assert np.array_equal(run_npy(src, str(tmp_path / "zero.npy"), Spy(plugin), Det(), monkeypatch, "0"), plain), "P = 0"
        monkeypatch.setenv("VSR_BORROW_PAN", str(PAN))
        spy = Spy(plugin)
        got = run_npy(src, str(tmp_path / "pan.npy"), spy, Det(), monkeypatch, "0")
        resident = run_npy(src, str(tmp_path / "resident.npy"), Spy(plugin), Det(), monkeypatch, "1")
    assert got.shape == clip.shape and np.array_equal(got, resident), "the host-frame and the resident loop write the same frames"
    spans = [(given, mask) for given, mask in spy.calls
             if any(np.array_equal(f, clip[CHANGE - 1]) for f in given) and any(np.array_equal(f, clip[CHANGE]) for f in given)]
    assert len(spans) == 1, [len(g) for g, _ in spy.calls]
    given, mask = spans[0]
    lo = next(i for i in range(N_FILE) if np.array_equal(clip[i], given[0]))
    n = len(given)
    assert np.array_equal(given, clip[lo:lo + n]) and lo <= CHANGE - 1 and CHANGE < lo + n
    C, rows = plugin.composite_mask(mask), plugin.sample_rows(mask)
    assert C[first].all(), "the detected box holds both captions"
    t = CHANGE - 1
    info = {}
    want = ks.key(ps.borrow_pan(fill[lo:lo + n], clip[lo:lo + n], C, rows, T, B, PAN, info=info), clip[lo:lo + n], C, T)
    lender, q = info["lender"][t - lo][first], info["q"][t - lo][first]
    print("call of", n, "frames from", lo, "; borrowed in it:", int((info["lender"] >= 0).sum()), "D:", info["D"])
    assert (lender >= CHANGE - lo).all(), "the statement: every glyph pixel of the first caption is lent by a frame behind the change"
    assert np.array_equal(got[lo:lo + n], want), "the written frames are the statement's"
    assert (q[..., 1] == np.mgrid[first][1] + STEP * (lender - (t - lo))).all(), "read STEP columns on per frame"
    behind = clip[lo:lo + n][lender, q[..., 0], q[..., 1]]
    assert np.array_equal(got[t][first], behind), "under the first caption's glyphs: the shifted source pixels of the frames behind the change"
    assert np.array_equal(plain[t][first], ks.key(fill[lo:lo + n], clip[lo:lo + n], C, T)[t - lo][first]), "where plain --borrow shows the fill"
    assert not np.array_equal(got[t][first], plain[t][first]) and not np.array_equal(got[t][first], clip[t][first])
