"""--tone-match at plugin level (backend/tools/tone_match.py inside tools/seam_feather.plugin_call / device_call): for every mode the
plugin call's frames equal the statement

    out == tone(fill, src, composite_mask(M), sample_rows(M), S)                                         tests/_tone_statement.py
    out == composite(regrain(deflicker(tone(fill, ...), ...), ...), src, composite_mask(M), F)           with the other three on top

exactly, where fill is the same plugin's output with the options off, in the same process; the device-tensor form and the list form
agree; with the option off nothing changes.  Plugins, masks, clip sizes and synthetic weights are those of
tests/test_gpu_seam_regrain.py: what is shown is that the output equals the definition, not what it looks like."""
import numpy as np
import pytest
import torch

from tests import _deflicker_statement as ds
from tests import _feather_statement as fs
from tests import _regrain_statement as rs
from tests import _tone_statement as ts
from tests.test_gpu_seam_feather import N_BATCH, call_device, call_list, geometry, make_plugin, mask_of
from tests.test_gpu_seam_regrain import noisy_clip
from vsr_amd.backend.tools.inpaint_tools import get_inpaint_area_by_mask, threshold_mask

pytestmark = pytest.mark.gpu

S = 80
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
    for name in ("VSR_SEAM_FEATHER", "VSR_REGRAIN", "VSR_DEFLICKER", "VSR_TONE_MATCH"):
        monkeypatch.delenv(name, raising=False)


def four(fill, clip, C, rows):
    """the four statements in the order of the chain: tone-match, deflicker, regrain, feather"""
    toned = ts.tone(fill, clip, C, rows, S)
    return fs.composite(rs.regrain(ds.deflicker(toned, clip, C, rows, 2), clip, C, rows, 100), clip, C, 4)


@pytest.mark.parametrize("mode", ["sttn-det", "lama", "opencv", "propainter"])
def test_plugin_call_equals_the_statement(built_lib, gpu_device, plugins, monkeypatch, mode):
    from vsr_amd.backend.tools import tone_match

    H, W, box = geometry(mode)
    clip = noisy_clip(N_BATCH, H, W, box, seed=5, mode=mode)
    mask = mask_of(mode)
    plugin = plugins(mode)
    all_off(monkeypatch)
    before = dict(tone_match.stats)
    fill = call_device(plugin, clip, mask, gpu_device)
    assert (fill != clip).any(), "the plugin fills something"
    monkeypatch.setenv("VSR_TONE_MATCH", "0")
    assert np.array_equal(call_device(plugin, clip, mask, gpu_device), fill), "S = 0 is off"
    assert np.array_equal(call_list(plugin, clip, mask), fill)
    assert tone_match.stats == before, "option off: nothing of tone match runs"
    C, rows = plugin.composite_mask(mask), plugin.sample_rows(mask)
    assert np.array_equal(C, fs.composite_mask(mode, mask)) and C.any() and rows == rs.sample_rows(mode, mask) == (0, H)
    monkeypatch.setenv("VSR_TONE_MATCH", str(S))
    info = []
    want = ts.tone(fill, clip, C, rows, S, info=info)
    print(mode, "(|E|, |M|, changed, touched):", [i[:4] for i in info], "bytes changed:", int((want != fill).sum()))
    got = call_device(plugin, clip, mask, gpu_device)
    assert np.array_equal(got, want), f"{mode}: {int((got != want).sum())} bytes differ from the statement"
    assert np.array_equal(got[:, C == 0], fill[:, C == 0]), "outside C the frame is what the plugin wrote"
    assert np.array_equal(call_list(plugin, clip, mask), want), "the list form gives the device form's frames"
    assert tone_match.stats["calls"] == before["calls"] + 2
    assert any(i[3] for i in info), "a frame was inpainted and has both bands"
    # all four: tone-match first, then deflicker, the grain and the feathered composite
    monkeypatch.setenv("VSR_DEFLICKER", "2")
    monkeypatch.setenv("VSR_REGRAIN", "100")
    monkeypatch.setenv("VSR_SEAM_FEATHER", "4")
    all_four = four(fill, clip, C, rows)
    got = call_device(plugin, clip, mask, gpu_device)
    assert np.array_equal(got, all_four), f"{mode}: {int((got != all_four).sum())} bytes differ from feather(regrain(deflicker(tone(fill))))"
    assert np.array_equal(call_list(plugin, clip, mask), all_four)
    assert np.array_equal(got[:, C == 0], clip[:, C == 0])
    monkeypatch.setenv("VSR_TONE_MATCH", "0")
    three = fs.composite(rs.regrain(ds.deflicker(fill, clip, C, rows, 2), clip, C, rows, 100), clip, C, 4)
    assert np.array_equal(call_device(plugin, clip, mask, gpu_device), three), "the other three alone are as they were"


def test_sttn_auto(built_lib, gpu_device, plugins, monkeypatch):
    """STTNInpaint.__call__ (list form) and the strip-rows form of the chunk loops: the bands lie in the hull of the inpaint areas' rows,
    in picture coordinates, so the rows handed to the engine come back as the rows of the full-frame result"""
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
        assert rows == rs.sample_rows("sttn-auto", mask) and 0 < rows[0] < rows[1] <= H and not C[:rows[0]].any() and not C[rows[1]:].any()
        monkeypatch.setenv("VSR_TONE_MATCH", str(S))
        want = ts.tone(fill, clip, C, rows, S)
        got = call_list(plugin, clip, mask)
        assert np.array_equal(got, want), f"{int((got != want).sum())} bytes differ from the statement"
        assert not np.array_equal(got, fill)
        monkeypatch.setenv("VSR_DEFLICKER", "2")
        monkeypatch.setenv("VSR_REGRAIN", "100")
        monkeypatch.setenv("VSR_SEAM_FEATHER", "4")
        all_four = four(fill, clip, C, rows)
        assert np.array_equal(call_list(plugin, clip, mask), all_four)
    # the rows form, on the tall mask (all four options still set)
    m = threshold_mask(tall)
    areas = get_inpaint_area_by_mask(W, H, int(W * 3 / 16), m)
    y_lo, y_hi = min(a[0] for a in areas), max(a[1] for a in areas)
    assert (y_lo, y_hi) == rows and 0 < y_lo and y_hi < H
    strip = torch.from_numpy(np.ascontiguousarray(clip[:, y_lo:y_hi])).to(gpu_device)
    dmask = torch.from_numpy(np.ascontiguousarray(m[y_lo:y_hi, :, 0])).to(gpu_device)
    local = [(a[0] - y_lo, a[1] - y_lo, a[2], a[3]) for a in areas]
    plugin.auto_chunk(strip, dmask, local, cmask=C, rows=(y_lo, y_hi), mask_host=m[y_lo:y_hi, :, 0])
    torch.cuda.synchronize()
    assert np.array_equal(strip.cpu().numpy(), all_four[:, y_lo:y_hi]), "strip rows: the full-frame definition"
    # the rows form with the tone match alone
    for name in ("VSR_SEAM_FEATHER", "VSR_REGRAIN", "VSR_DEFLICKER"):
        monkeypatch.delenv(name)
    strip = torch.from_numpy(np.ascontiguousarray(clip[:, y_lo:y_hi])).to(gpu_device)
    plugin.auto_chunk(strip, dmask, local, cmask=C, rows=(y_lo, y_hi), mask_host=m[y_lo:y_hi, :, 0])
    torch.cuda.synchronize()
    assert np.array_equal(strip.cpu().numpy(), want[:, y_lo:y_hi])


def test_the_bands_are_cached(built_lib, gpu_device, plugins, monkeypatch):
    from vsr_amd.backend.tools import tone_match

    H, W, box = geometry("opencv")
    clip = noisy_clip(2, H, W, box, seed=3)
    mask = mask_of("opencv")
    plugin = plugins("opencv")
    all_off(monkeypatch)
    monkeypatch.setenv("VSR_TONE_MATCH", "100")
    call_device(plugin, clip, mask, gpu_device)
    builds, hits = tone_match.stats["set_builds"], tone_match.stats["set_hits"]
    call_device(plugin, clip, mask, gpu_device)
    assert tone_match.stats["set_builds"] == builds and tone_match.stats["set_hits"] == hits + 1
    assert len(tone_match._sets) <= tone_match.MAX_SETS
