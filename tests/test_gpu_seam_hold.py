"""--glyph-hold at plugin level (backend/tools/glyph_key.py inside tools/seam_feather.plugin_call / device_call): for every mode the
plugin call's frames equal the statement

    out == hold(fill, src, composite_mask(M), T, K)                                                         tests/_hold_statement.py
    out == composite(hold(regrain(deflicker(tone(fill, ...), ...), ...), src, C, T, K), src, C, F)          with the other four around it

exactly, where fill is the same plugin's output with the options off, in the same process; the device-tensor form and the list form
agree; K = 0 is the run with --glyph-key alone.  Plugins, masks and clips are those of tests/test_gpu_seam_key.py."""
import numpy as np
import pytest
import torch

from tests import _deflicker_statement as ds
from tests import _feather_statement as fs
from tests import _hold_statement as hs
from tests import _key_statement as ks
from tests import _regrain_statement as rs
from tests import _tone_statement as ts
from tests.test_gpu_seam_feather import N_BATCH, call_device, call_list, geometry, make_plugin, mask_of
from tests.test_gpu_seam_regrain import noisy_clip
from vsr_amd.backend.tools.inpaint_tools import get_inpaint_area_by_mask, threshold_mask

pytestmark = pytest.mark.gpu

T, K = 12, 2
NAMES = ("VSR_SEAM_FEATHER", "VSR_REGRAIN", "VSR_DEFLICKER", "VSR_TONE_MATCH", "VSR_GLYPH_KEY", "VSR_GLYPH_HOLD")
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


def five(fill, clip, C, rows, k=K):
    """the five statements in the order of the chain: tone-match, deflicker, regrain, glyph-key with its hold, feather"""
    grained = rs.regrain(ds.deflicker(ts.tone(fill, clip, C, rows, 80), clip, C, rows, 2), clip, C, rows, 100)
    return fs.composite(hs.hold(grained, clip, C, T, k), clip, C, 4)


@pytest.mark.parametrize("mode", ["sttn-det", "lama", "opencv", "propainter"])
def test_plugin_call_equals_the_statement(built_lib, gpu_device, plugins, monkeypatch, mode):
    from vsr_amd.backend.tools import glyph_key

    H, W, box = geometry(mode)
    clip = noisy_clip(N_BATCH, H, W, box, seed=5, mode=mode)
    mask = mask_of(mode)
    plugin = plugins(mode)
    all_off(monkeypatch)
    fill = call_device(plugin, clip, mask, gpu_device)
    assert (fill != clip).any(), "the plugin fills something"
    C = plugin.composite_mask(mask)
    rows = plugin.sample_rows(mask)
    # K = 0: the run with --glyph-key alone, by the plain call
    monkeypatch.setenv("VSR_GLYPH_KEY", str(T))
    plain = call_device(plugin, clip, mask, gpu_device)
    before = dict(glyph_key.stats)
    monkeypatch.setenv("VSR_GLYPH_HOLD", "0")
    assert np.array_equal(call_device(plugin, clip, mask, gpu_device), plain), "K = 0 is --glyph-key alone"
    assert np.array_equal(call_list(plugin, clip, mask), plain) and np.array_equal(plain, ks.key(fill, clip, C, T))
    assert glyph_key.stats["hold_calls"] == before["hold_calls"] and glyph_key.stats["calls"] == before["calls"] + 2
    monkeypatch.setenv("VSR_GLYPH_HOLD", str(K))
    holds = before["hold_calls"]
    for t in (T, 128):
        monkeypatch.setenv("VSR_GLYPH_KEY", str(t))
        info = []
        want = hs.hold(fill, clip, C, t, K, info=info)
        S, Wk, Z, a = info[0]
        print(mode, "T =", t, "strong:", int(S.sum()), "weak:", int(Wk.sum()), "held:", int(Z.sum()), "of", Z.size,
              "bytes the hold changes:", int((want != ks.key(fill, clip, C, t)).sum()))
        got = call_device(plugin, clip, mask, gpu_device)
        assert np.array_equal(got, want), f"{mode}: {int((got != want).sum())} bytes differ from the statement"
        assert np.array_equal(got[:, C == 0], fill[:, C == 0]), "outside C the frame is what the plugin wrote"
        assert np.array_equal(call_list(plugin, clip, mask), want), "the list form gives the device form's frames"
        holds += 2
        assert glyph_key.stats["hold_calls"] == holds
    # all five: tone-match, deflicker, the grain, the held key and the feathered composite
    monkeypatch.setenv("VSR_GLYPH_KEY", str(T))
    others_on(monkeypatch)
    all_five = five(fill, clip, C, rows)
    got = call_device(plugin, clip, mask, gpu_device)
    assert np.array_equal(got, all_five), f"{mode}: {int((got != all_five).sum())} bytes differ from feather(hold(regrain(deflicker(tone(fill)))))"
    assert np.array_equal(call_list(plugin, clip, mask), all_five)
    assert np.array_equal(got[:, C == 0], clip[:, C == 0])
    monkeypatch.setenv("VSR_GLYPH_HOLD", "0")
    assert np.array_equal(call_device(plugin, clip, mask, gpu_device), five(fill, clip, C, rows, k=0)), "K = 0: the five as they were"


def test_sttn_auto(built_lib, gpu_device, plugins, monkeypatch):
    """STTNInpaint.__call__ (list form) and the strip-rows form of the chunk loops: the rows handed to the engine hold the rows of the
    composite mask, so they come back as the rows of the full-frame result"""
    from vsr_amd.backend.tools import glyph_key

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
        monkeypatch.setenv("VSR_GLYPH_KEY", str(T))
        monkeypatch.setenv("VSR_GLYPH_HOLD", str(K))
        holds = glyph_key.stats["hold_calls"]
        want = hs.hold(fill, clip, C, T, K)
        got = call_list(plugin, clip, mask)
        assert np.array_equal(got, want), f"{int((got != want).sum())} bytes differ from the statement"
        assert glyph_key.stats["hold_calls"] == holds + 1
        others_on(monkeypatch)
        all_five = five(fill, clip, C, rows)
        assert np.array_equal(call_list(plugin, clip, mask), all_five)
    # the rows form, on the tall mask (all five options still set)
    m = threshold_mask(tall)
    areas = get_inpaint_area_by_mask(W, H, int(W * 3 / 16), m)
    y_lo, y_hi = min(a[0] for a in areas), max(a[1] for a in areas)
    assert (y_lo, y_hi) == rows and 0 < y_lo and y_hi < H
    strip = torch.from_numpy(np.ascontiguousarray(clip[:, y_lo:y_hi])).to(gpu_device)
    dmask = torch.from_numpy(np.ascontiguousarray(m[y_lo:y_hi, :, 0])).to(gpu_device)
    local = [(a[0] - y_lo, a[1] - y_lo, a[2], a[3]) for a in areas]
    plugin.auto_chunk(strip, dmask, local, cmask=C, rows=(y_lo, y_hi), mask_host=m[y_lo:y_hi, :, 0])
    torch.cuda.synchronize()
    assert np.array_equal(strip.cpu().numpy(), all_five[:, y_lo:y_hi]), "strip rows: the full-frame definition"
    # the rows form with the held key alone
    for name in NAMES[:4]:
        monkeypatch.delenv(name)
    strip = torch.from_numpy(np.ascontiguousarray(clip[:, y_lo:y_hi])).to(gpu_device)
    plugin.auto_chunk(strip, dmask, local, cmask=C, rows=(y_lo, y_hi), mask_host=m[y_lo:y_hi, :, 0])
    torch.cuda.synchronize()
    assert np.array_equal(strip.cpu().numpy(), want[:, y_lo:y_hi])
    assert np.array_equal(strip.cpu().numpy(), hs.hold(fill[:, y_lo:y_hi], clip[:, y_lo:y_hi], C, T, K, y0=y_lo)), "and the strip's own statement"
