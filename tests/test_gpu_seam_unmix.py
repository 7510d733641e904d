"""--logo-unblend at plugin level (backend/tools/unblend.py inside tools/seam_feather.plugin_call / device_call) and through a whole run:

    out == unmix(fill, src)                                 tests/_unmix_statement.py, with every other option off
    out == unmix(feather(fill), src)                        behind the composite

exactly, for every mode's plugin call in the tensor and the list form and for sttn-auto's strip form, on planes that hold opaque,
translucent and clear pixels; then opencv mode (no weights) from the command line on the wave clip whose logo is blended at a = 128: the
written frames show the clean wave inside the area, and every byte outside it is the run's with --logo-scan alone."""
import numpy as np
import pytest
import torch

from tests import _feather_statement as fs
from tests import _static_statement as st
from tests import _unmix_statement as us
from tests.test_gpu_logo_scan import NoText, records, write_y4m
from tests.test_gpu_seam_feather import N_BATCH, call_device, call_list, geometry, make_plugin, mask_of
from tests.test_gpu_seam_regrain import noisy_clip
from vsr_amd.backend.tools.inpaint_tools import get_inpaint_area_by_mask, threshold_mask

pytestmark = pytest.mark.gpu

NAMES = ("VSR_SEAM_FEATHER", "VSR_REGRAIN", "VSR_DEFLICKER", "VSR_TONE_MATCH", "VSR_GLYPH_KEY", "VSR_GLYPH_HOLD", "VSR_BORROW", "VSR_BORROW_PAN",
         "VSR_LOGO_SCAN", "VSR_LOGO_UNBLEND")

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


def planes(box, seed):
    """a gain and an offset plane for the box: columns of opaque (g < 64), level, rim and clear pixels"""
    rng = np.random.default_rng(seed)
    bh, bw = box[1] - box[0], box[3] - box[2]
    gt = np.empty((bh, bw), np.int64)
    gt[:, :bw // 4] = 40
    gt[:, bw // 4:bw // 2] = 150
    gt[:, bw // 2:3 * bw // 4] = rng.integers(64, 300, size=(bh, 3 * bw // 4 - bw // 2))
    gt[:, 3 * bw // 4:] = 256
    ot = rng.integers(0, 1600, size=(bh, bw, 3)).astype(np.int64)
    ot[gt == 256] = 0
    return gt, ot


def make_plan(box, H, W, gt, ot, device):
    from vsr_amd.backend.tools import unblend

    return unblend.Plan(box, H, W, torch.from_numpy(gt.astype(np.uint16).view(np.int16)).to(device), torch.from_numpy(ot.astype(np.int16)).to(device), 150)


def unmixed(frames, clip, gt, ot, box, y0=0):
    out = frames.copy()
    for f, s in zip(out, clip):
        us.unmix(f, s, gt, ot, box, y0=y0)
    return out


@pytest.fixture
def registry():
    from vsr_amd.backend.tools import unblend

    yield unblend
    unblend.clear()


@pytest.mark.parametrize("mode", ["sttn-det", "lama", "opencv", "propainter"])
def test_plugin_call_equals_the_statement(built_lib, gpu_device, plugins, monkeypatch, registry, mode):
    H, W, box = geometry(mode)
    clip = noisy_clip(N_BATCH, H, W, box, seed=5, mode=mode)
    mask = mask_of(mode)
    plugin = plugins(mode)
    all_off(monkeypatch)
    fill = call_device(plugin, clip, mask, gpu_device)
    assert (fill != clip).any(), "the plugin fills something"
    C = plugin.composite_mask(mask)
    area = (box[0] + 3, box[1] - 3, box[2] + 40, box[2] + 141)                # inside the pixels the plugin fills
    assert C[area[0]:area[1], area[2]:area[3]].all()
    gt, ot = planes(area, seed=1)
    applies = registry.stats["applies"]
    monkeypatch.setenv("VSR_LOGO_SCAN", "1")
    monkeypatch.setenv("VSR_LOGO_UNBLEND", "1")
    assert np.array_equal(call_device(plugin, clip, mask, gpu_device), fill) and registry.stats["applies"] == applies, "no plans: the run without"
    registry.register([make_plan(area, H, W, gt, ot, gpu_device)])
    want = unmixed(fill, clip, gt, ot, area)
    inside = (slice(None), slice(area[0], area[1]), slice(area[2], area[3]))
    assert not np.array_equal(want[inside], fill[inside]) and not np.array_equal(want[inside], clip[inside])
    got = call_device(plugin, clip, mask, gpu_device)
    assert np.array_equal(got, want), f"{mode}: {int((got != want).sum())} bytes differ from the statement"
    assert np.array_equal(got[inside][:, gt < 64], fill[inside][:, gt < 64]), "the fill stays under the opaque part"
    assert np.array_equal(call_list(plugin, clip, mask), want), "the list form gives the device form's frames"
    assert registry.stats["applies"] == applies + 2
    monkeypatch.setenv("VSR_SEAM_FEATHER", "4")
    behind = unmixed(fs.composite(fill, clip, C, 4), clip, gt, ot, area)
    got = call_device(plugin, clip, mask, gpu_device)
    assert np.array_equal(got, behind), f"{mode}: {int((got != behind).sum())} bytes differ from unmix(feather(fill))"
    assert np.array_equal(call_list(plugin, clip, mask), behind)
    registry.clear()
    assert np.array_equal(call_device(plugin, clip, mask, gpu_device), fs.composite(fill, clip, C, 4)), "plans cleared: the feather alone"


def test_sttn_auto(built_lib, gpu_device, plugins, monkeypatch, registry):
    """STTNInpaint.__call__ (list form) and the strip-rows form of the chunk loops, with a box the strip cuts"""
    H, W, box = geometry("sttn-auto")
    plugin = plugins("sttn-auto")
    clip = noisy_clip(N_BATCH, H, W, box, seed=5)
    tall = np.zeros((H, W), np.uint8)
    tall[100:230, 60:380] = 255                                    # 130 rows, the strip has int(432 * 3 / 16) = 81
    all_off(monkeypatch)
    fill = call_list(plugin, clip, tall)
    C = plugin.composite_mask(tall)
    m = threshold_mask(tall)
    areas = get_inpaint_area_by_mask(W, H, int(W * 3 / 16), m)
    y_lo, y_hi = min(a[0] for a in areas), max(a[1] for a in areas)
    assert 0 < y_lo and y_hi < H
    area = (y_lo - 6, y_lo + 40, 100, 201)                         # six rows above the strip: the strip form sees the rest
    gt, ot = planes(area, seed=2)
    registry.register([make_plan(area, H, W, gt, ot, gpu_device)])
    want = unmixed(fill, clip, gt, ot, area)
    got = call_list(plugin, clip, tall)
    assert np.array_equal(got, want), f"{int((got != want).sum())} bytes differ from the statement"
    dmask = torch.from_numpy(np.ascontiguousarray(m[y_lo:y_hi, :, 0])).to(gpu_device)
    local = [(a[0] - y_lo, a[1] - y_lo, a[2], a[3]) for a in areas]
    strip = torch.from_numpy(np.ascontiguousarray(clip[:, y_lo:y_hi])).to(gpu_device)
    plugin.auto_chunk(strip, dmask, local, cmask=C, rows=(y_lo, y_hi), mask_host=m[y_lo:y_hi, :, 0])
    torch.cuda.synchronize()
    registry.clear()
    bare = torch.from_numpy(np.ascontiguousarray(clip[:, y_lo:y_hi])).to(gpu_device)
    plugin.auto_chunk(bare, dmask, local, cmask=C, rows=(y_lo, y_hi), mask_host=m[y_lo:y_hi, :, 0])
    torch.cuda.synchronize()
    own = unmixed(bare.cpu().numpy(), clip[:, y_lo:y_hi], gt, ot, area, y0=y_lo)
    assert np.array_equal(strip.cpu().numpy(), own), "strip rows: the strip's own statement"
    assert not np.array_equal(own, bare.cpu().numpy())


# ---- a whole run ----------------------------------------------------------------------------------------------------------------------------
def run_cli(monkeypatch, src, out, flags, said=None):
    """backend.main.main() in opencv mode with a text detector that finds nothing"""
    from vsr_amd.backend import main as m
    from vsr_amd.backend.config import config

    for name in NAMES:
        monkeypatch.setenv(name, "0")                              # (main() writes the flags into the environment: put back afterwards)
    monkeypatch.setenv("VSR_Y4M_OUT", "444")                       # (likewise --y4m-out)
    monkeypatch.delenv("VSR_OPENCV_BACKEND", raising=False)
    monkeypatch.setattr(m.SubtitleRemover, "_default_detector", lambda self: NoText())
    if said is not None:
        monkeypatch.setattr(m.SubtitleRemover, "append_output", lambda self, *a: said.append(" ".join(str(x) for x in a)))
    old = config.inpaintMode.value
    try:
        m.main(["-i", src, "-o", out, "--inpaint-mode", "opencv"] + flags)
    finally:
        config.inpaintMode.value = old


def test_a_run_un_mixes_a_translucent_logo(built_lib, gpu_device, tmp_path, monkeypatch, registry):
    """*.npy in and out (the lossless container) from the command line: with both flags the area of every written frame lies within 2
    levels of the clean wave and everything outside it is the --logo-scan run's byte; the opaque logo is refused and written as
    --logo-scan alone writes it"""
    clean = st.wave()
    clip = us.blend(clean, 128)
    src = str(tmp_path / "in.npy")
    np.save(src, clip)
    run_cli(monkeypatch, src, str(tmp_path / "scan.npy"), ["--logo-scan"])
    said = []
    run_cli(monkeypatch, src, str(tmp_path / "both.npy"), ["--logo-scan", "--logo-unblend"], said)
    assert registry.active() == [], "the run cleared its plans"
    scan, both = np.load(str(tmp_path / "scan.npy")), np.load(str(tmp_path / "both.npy"))
    assert scan.shape == both.shape == clip.shape
    assert any("is un-mixed" in s and str(st.LOGO_AREA) in s for s in said), said
    y0, y1, x0, x1 = st.LOGO_AREA
    err = np.abs(both[:, y0:y1, x0:x1].astype(np.int64) - clean[:, y0:y1, x0:x1])
    print("un-mixed: max", err.max(), "mean", err.mean(), "; inpainted: max",
          np.abs(scan[:, y0:y1, x0:x1].astype(np.int64) - clean[:, y0:y1, x0:x1]).max())
    assert err.max() <= 2, "the area of every written frame lies within 2 levels of the clean wave"
    outside = np.ones(clip.shape[1:3], bool)
    outside[y0:y1, x0:x1] = False
    assert np.array_equal(both[:, outside], scan[:, outside]), "outside the area: the --logo-scan run byte for byte"
    assert (scan[:, outside] != clip[:, outside]).any(), "(the mask margin around the area is inpainted in both)"
    # the opaque logo
    src2 = str(tmp_path / "opaque.npy")
    np.save(src2, st.clip_logo())
    run_cli(monkeypatch, src2, str(tmp_path / "scan2.npy"), ["--logo-scan"])
    said = []
    run_cli(monkeypatch, src2, str(tmp_path / "both2.npy"), ["--logo-scan", "--logo-unblend"], said)
    assert any("stays inpainted (shows)" in s for s in said), said
    assert np.array_equal(np.load(str(tmp_path / "both2.npy")), np.load(str(tmp_path / "scan2.npy")))


def test_source_format_output_copies_the_samples_outside_the_area(built_lib, gpu_device, tmp_path, monkeypatch, registry):
    """--y4m-out source: every stored sample outside the pixels the mode masks for the area is the source's, every sample outside the
    area is the --logo-scan run's, and inside the area the luma is no longer the blended one"""
    from vsr_amd.backend.tools.inpaint_tools import create_mask

    clip = us.blend(st.wave(), 128)
    n, H, W = len(clip), st.CLIP_H, st.CLIP_W
    src = write_y4m(tmp_path / "in.y4m", clip)
    run_cli(monkeypatch, src, str(tmp_path / "scan.y4m"), ["--logo-scan", "--y4m-out", "source"])
    run_cli(monkeypatch, src, str(tmp_path / "both.y4m"), ["--logo-scan", "--logo-unblend", "--y4m-out", "source"])
    before, scan, both = (records(str(tmp_path / name), n) for name in ("in.y4m", "scan.y4m", "both.y4m"))
    ymin, ymax, xmin, xmax = st.LOGO_AREA
    masked = create_mask((H, W), [(xmin, xmax, ymin, ymax)]) != 0
    assert np.array_equal(both[:, :, ~masked], before[:, :, ~masked]), "outside the masked pixels: the source's samples"
    outside = np.ones((H, W), bool)
    outside[ymin:ymax, xmin:xmax] = False
    assert np.array_equal(both[:, :, outside], scan[:, :, outside]), "outside the area: the --logo-scan run's samples"
    y0, y1, x0, x1 = st.LOGO
    assert (both[:, 0, y0:y1, x0:x1] != before[:, 0, y0:y1, x0:x1]).mean() > 0.9, "the logo's pixels were un-mixed"
