"""--deflicker at plugin and file level (backend/tools/deflicker.py inside tools/seam_feather.plugin_call / device_call): for every mode
the plugin call's frames equal the statement

    out == deflicker(fill, src, composite_mask(M), sample_rows(M), R)                              tests/_deflicker_statement.py
    out == composite(regrain(deflicker(fill, ...), ...), src, composite_mask(M), F)      with --regrain P and --seam-feather F on top

exactly, where fill is the same plugin's output with the options off, in the same process; the device-tensor form and the list form
agree; with the option off nothing changes; the loops of SubtitleRemover write the same bytes.  Plugins, masks and synthetic weights are
those of tests/test_gpu_seam_feather.py; the clips stand still under fresh grain per frame, so that the pairs are open and what differs
from frame to frame in the fill is flicker.  What is shown is that the output equals the definition, not what it looks like."""
import numpy as np
import pytest
import torch

from tests import _deflicker_statement as ds
from tests import _feather_statement as fs
from tests import _regrain_statement as rs
from tests.test_gpu_seam_feather import (CUT, N, N_BATCH, ON, PER_WINDOW, call_device, call_list, config_values, geometry, make_detector,
                                         make_plugin, mask_of, run, write_source)
from vsr_amd import synth
from vsr_amd.backend.tools.inpaint_tools import get_inpaint_area_by_mask, threshold_mask

pytestmark = pytest.mark.gpu

R = 2
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


def still_clip(n, H, W, box, seed):
    """one frame of the synthetic clip n times, each under its own sensor noise: the picture around the mask stands still"""
    frame = synth.make_clip(1, H, W, box, seed=seed)[0].astype(np.int64)
    rng = np.random.default_rng(seed)
    return np.clip(frame[None] + np.rint(rng.normal(0, 3, (n,) + frame.shape)).astype(np.int64), 0, 255).astype(np.uint8)


def all_off(monkeypatch):
    for name in ("VSR_SEAM_FEATHER", "VSR_REGRAIN", "VSR_DEFLICKER"):
        monkeypatch.delenv(name, raising=False)


@pytest.mark.parametrize("mode", ["sttn-det", "lama", "opencv", "propainter"])
def test_plugin_call_equals_the_statement(built_lib, gpu_device, plugins, monkeypatch, mode):
    from vsr_amd.backend.tools import deflicker

    H, W, box = geometry(mode)
    clip = still_clip(N_BATCH, H, W, box, seed=5)
    mask = mask_of(mode)
    plugin = plugins(mode)
    all_off(monkeypatch)
    before = dict(deflicker.stats)
    fill = call_device(plugin, clip, mask, gpu_device)
    assert (fill != clip).any(), "the plugin fills something"
    monkeypatch.setenv("VSR_DEFLICKER", "0")
    assert np.array_equal(call_device(plugin, clip, mask, gpu_device), fill), "R = 0 is off"
    assert np.array_equal(call_list(plugin, clip, mask), fill)
    assert deflicker.stats == before, "option off: nothing of deflicker runs"
    C, rows = plugin.composite_mask(mask), plugin.sample_rows(mask)
    assert np.array_equal(C, fs.composite_mask(mode, mask)) and C.any() and rows == rs.sample_rows(mode, mask) == (0, H)
    monkeypatch.setenv("VSR_DEFLICKER", str(R))
    info = {}
    want = ds.deflicker(fill, clip, C, rows, R, info=info)
    print(mode, "pair weights:", info["a"], "bytes changed:", int((want != fill).sum()))
    assert set(info["a"].values()) == {16}, "a still scene under grain: every pair is open"
    got = call_device(plugin, clip, mask, gpu_device)
    assert np.array_equal(got, want), f"{mode}: {int((got != want).sum())} bytes differ from the statement"
    assert np.array_equal(got[:, C == 0], fill[:, C == 0]), "outside C the frame is what the plugin wrote"
    assert np.array_equal(call_list(plugin, clip, mask), want), "the list form gives the device form's frames"
    assert deflicker.stats["calls"] == before["calls"] + 2
    assert not np.array_equal(want, fill), "the fill flickered and was steadied"
    # --regrain and --seam-feather on top: deflicker first, then the grain, then the feathered composite
    monkeypatch.setenv("VSR_REGRAIN", "100")
    monkeypatch.setenv("VSR_SEAM_FEATHER", "4")
    three = fs.composite(rs.regrain(want, clip, C, rows, 100), clip, C, 4)
    got = call_device(plugin, clip, mask, gpu_device)
    assert np.array_equal(got, three), f"{mode}: {int((got != three).sum())} bytes differ from feather(regrain(deflicker(fill)))"
    assert np.array_equal(call_list(plugin, clip, mask), three)
    assert np.array_equal(got[:, C == 0], clip[:, C == 0])
    monkeypatch.setenv("VSR_DEFLICKER", "0")
    two = fs.composite(rs.regrain(fill, clip, C, rows, 100), clip, C, 4)
    assert np.array_equal(call_device(plugin, clip, mask, gpu_device), two), "the other two alone are as they were"


def test_sttn_auto(built_lib, gpu_device, plugins, monkeypatch):
    """STTNInpaint.__call__ (list form) and the strip-rows form of the chunk loops: the ring lies in the hull of the inpaint areas' rows,
    in full-frame coordinates, so the rows handed to the engine come back as the rows of the full-frame result"""
    H, W, box = geometry("sttn-auto")
    plugin = plugins("sttn-auto")
    clip = still_clip(N_BATCH, H, W, box, seed=5)
    tall = np.zeros((H, W), np.uint8)
    tall[100:230, 60:380] = 255                                    # 130 rows, the strip has int(432 * 3 / 16) = 81
    for mask in (mask_of("sttn-auto"), tall):
        all_off(monkeypatch)
        fill = call_list(plugin, clip, mask)
        assert (fill != clip).any()
        C, rows = plugin.composite_mask(mask), plugin.sample_rows(mask)
        assert rows == rs.sample_rows("sttn-auto", mask) and 0 < rows[0] < rows[1] <= H and not C[:rows[0]].any() and not C[rows[1]:].any()
        monkeypatch.setenv("VSR_DEFLICKER", str(R))
        info = {}
        want = ds.deflicker(fill, clip, C, rows, R, info=info)
        assert set(info["a"].values()) == {16}
        got = call_list(plugin, clip, mask)
        assert np.array_equal(got, want) and not np.array_equal(got, fill)
        monkeypatch.setenv("VSR_REGRAIN", "100")
        monkeypatch.setenv("VSR_SEAM_FEATHER", "4")
        three = fs.composite(rs.regrain(want, clip, C, rows, 100), clip, C, 4)
        assert np.array_equal(call_list(plugin, clip, mask), three)
    # the rows form, on the tall mask (all three options still set)
    m = threshold_mask(tall)
    areas = get_inpaint_area_by_mask(W, H, int(W * 3 / 16), m)
    y_lo, y_hi = min(a[0] for a in areas), max(a[1] for a in areas)
    assert (y_lo, y_hi) == rows and 0 < y_lo and y_hi < H
    strip = torch.from_numpy(np.ascontiguousarray(clip[:, y_lo:y_hi])).to(gpu_device)
    dmask = torch.from_numpy(np.ascontiguousarray(m[y_lo:y_hi, :, 0])).to(gpu_device)
    local = [(a[0] - y_lo, a[1] - y_lo, a[2], a[3]) for a in areas]
    plugin.auto_chunk(strip, dmask, local, cmask=C, rows=(y_lo, y_hi), mask_host=m[y_lo:y_hi, :, 0])
    torch.cuda.synchronize()
    assert np.array_equal(strip.cpu().numpy(), three[:, y_lo:y_hi]), "strip rows: the full-frame definition"
    # the rows form with the deflicker alone
    monkeypatch.delenv("VSR_REGRAIN")
    monkeypatch.delenv("VSR_SEAM_FEATHER")
    strip = torch.from_numpy(np.ascontiguousarray(clip[:, y_lo:y_hi])).to(gpu_device)
    plugin.auto_chunk(strip, dmask, local, cmask=C, rows=(y_lo, y_hi), mask_host=m[y_lo:y_hi, :, 0])
    torch.cuda.synchronize()
    assert np.array_equal(strip.cpu().numpy(), want[:, y_lo:y_hi])


def test_lama_single_frame_is_the_identity(built_lib, gpu_device, plugins, monkeypatch):
    """LamaInpaint.inpaint: the single picture and propainter's single-frame fall-back have no neighbour"""
    from vsr_amd.backend.tools import deflicker

    H, W, box = geometry("lama")
    frame = still_clip(1, H, W, box, seed=9)[0]
    mask = mask_of("lama")
    plugin = plugins("lama")
    all_off(monkeypatch)
    fill = plugin.inpaint(frame, mask)
    before = dict(deflicker.stats)
    monkeypatch.setenv("VSR_DEFLICKER", "8")
    assert np.array_equal(plugin.inpaint(frame, mask), fill) and deflicker.stats == before


# ---- file to file -------------------------------------------------------------------------------------------------------------------
def still_file_clip(H, W, box):
    """the file clip of tests/test_gpu_seam_feather.py (two subtitle intervals with a gap, the background inverted from frame CUT on)
    on a background that stands still, fresh grain on every frame"""
    glyphs = synth.make_clip(1, H, W, box, seed=5)[0]
    plain = synth.make_clip(1, H, W, (0, 1, 0, 1), seed=5)[0]
    rng = np.random.default_rng(12)
    clip = np.empty((N, H, W, 3), np.uint8)
    for i in range(N):
        frame = glyphs if i in ON else plain
        if i >= CUT:
            frame = np.where((frame != plain).any(axis=-1, keepdims=True), frame, 255 - frame)
        clip[i] = np.clip(frame.astype(np.int64) + np.rint(rng.normal(0, 3, frame.shape)).astype(np.int64), 0, 255).astype(np.uint8)
    return clip


@pytest.mark.parametrize("mode", ["sttn-det", "opencv"])
def test_every_loop_writes_the_same_file(built_lib, gpu_device, plugins, tmp_path, monkeypatch, mode):
    """R = 2: the host-frame loop, the HBM-resident loop and resident windows (a budget of 2 x 10 frames) hand the plugin the same
    batches and write the same bytes, and not the bytes of a run with the option off"""
    H, W, box = geometry(mode)
    src = str(tmp_path / "in.y4m")
    write_source(src, still_file_clip(H, W, box), monkeypatch)
    Det = make_detector(box)
    plugin = plugins(mode)
    gb = repr((2 * PER_WINDOW * H * W * 3 + 1024) / 2 ** 30)
    with config_values():
        all_off(monkeypatch)
        off, _ = run(src, str(tmp_path / "off.y4m"), plugin, Det(), monkeypatch, "1")
        monkeypatch.setenv("VSR_DEFLICKER", str(R))
        host, sr_host = run(src, str(tmp_path / "host.y4m"), plugin, Det(), monkeypatch, "0")
        resident, sr_res = run(src, str(tmp_path / "resident.y4m"), plugin, Det(), monkeypatch, "1")
        windows, sr_win = run(src, str(tmp_path / "windows.y4m"), plugin, Det(), monkeypatch, "windows", gb)
    assert "read + inpainting + write (host frames)" in sr_host.phase_seconds
    assert "read + inpainting + write (host frames)" not in sr_res.phase_seconds and sr_res.resident_windows is None
    assert sr_win.resident_windows is not None and len(sr_win.resident_windows["windows"]) >= 3
    assert host == resident == windows
    assert resident != off and len(resident) == len(off)
