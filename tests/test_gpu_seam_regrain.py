"""--regrain at plugin and file level (backend/tools/regrain.py inside tools/seam_feather.plugin_call / device_call): for every mode the
plugin call's frames equal the statement

    out == regrain(fill, src, composite_mask(M), sample_rows(M), P)                              tests/_regrain_statement.py
    out == composite(regrain(fill, ...), src, composite_mask(M), F)     with --seam-feather F     tests/_feather_statement.py

exactly, where fill is the same plugin's output with both options off, in the same process; the device-tensor form and the list form
agree; with the option off nothing changes; the loops of SubtitleRemover write the same bytes.  Clip sizes and synthetic weights are
those of tests/test_gpu_seam_feather.py: what is shown is that the output equals the definition, not what it looks like."""
import numpy as np
import pytest
import torch

from tests import _feather_statement as fs
from tests import _regrain_statement as rs
from tests.test_gpu_seam_feather import (N_BATCH, PER_WINDOW, call_device, call_list, config_values, geometry, make_clip, make_detector,
                                         make_plugin, mask_of, run, write_source)
from vsr_amd import synth
from vsr_amd.backend.tools.inpaint_tools import get_inpaint_area_by_mask, threshold_mask

pytestmark = pytest.mark.gpu

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


def noisy_clip(n, H, W, box, seed, mode=None):
    """the synthetic clip with sensor noise on it: a source without grain has no deficit to put back.  The LaMa of the synthetic
    weights answers with a picture close to random bytes (mean L 1138 under the mask, whatever it is shown; Gaussian noise of sigma 6
    gives the ring 92, and no Gaussian noise reaches it before it clips), so its source is the noisiest there is: every sample 0 or 255."""
    clip = synth.make_clip(n, H, W, box, seed=seed)
    rng = np.random.default_rng(seed)
    if mode == "lama":
        return (rng.integers(0, 2, clip.shape) * 255).astype(np.uint8)
    return np.clip(clip.astype(np.int64) + np.rint(rng.normal(0, 6, clip.shape)).astype(np.int64), 0, 255).astype(np.uint8)


def both_off(monkeypatch):
    monkeypatch.delenv("VSR_SEAM_FEATHER", raising=False)
    monkeypatch.delenv("VSR_REGRAIN", raising=False)


@pytest.mark.parametrize("mode", ["sttn-det", "lama", "opencv", "propainter"])
def test_plugin_call_equals_the_statement(built_lib, gpu_device, plugins, monkeypatch, mode):
    H, W, box = geometry(mode)
    clip = noisy_clip(N_BATCH, H, W, box, seed=5, mode=mode)
    mask = mask_of(mode)
    plugin = plugins(mode)
    both_off(monkeypatch)
    fill = call_device(plugin, clip, mask, gpu_device)
    assert (fill != clip).any(), "the plugin fills something"
    monkeypatch.setenv("VSR_REGRAIN", "0")
    assert np.array_equal(call_device(plugin, clip, mask, gpu_device), fill), "P = 0 is off"
    C, R = plugin.composite_mask(mask), plugin.sample_rows(mask)
    assert np.array_equal(C, fs.composite_mask(mode, mask)) and C.any() and R == rs.sample_rows(mode, mask) == (0, H)
    monkeypatch.setenv("VSR_REGRAIN", "100")
    info = []
    want = rs.regrain(fill, clip, C, R, 100, info=info)
    print(mode, "(A_src, A_fill, changed, r, seed, touched):", info)
    got = call_device(plugin, clip, mask, gpu_device)
    assert np.array_equal(got, want), f"{mode}: {int((got != want).sum())} bytes differ from the statement"
    assert np.array_equal(got[:, C == 0], fill[:, C == 0]), "outside C the frame is what the plugin wrote"
    assert np.array_equal(call_list(plugin, clip, mask), want), "the list form gives the device form's frames"
    grained = any(i[5] and i[3] > 0 for i in info)
    assert grained == (not np.array_equal(want, fill))
    # (lama: whether even that source out-noises the synthetic LaMa's fill is the weights' business; if not, r = 0 and out == fill)
    assert grained or mode == "lama", "the fill lacked grain and got some"
    # --seam-feather on top: regrain first, the feathered composite follows unchanged
    monkeypatch.setenv("VSR_SEAM_FEATHER", "4")
    both = fs.composite(want, clip, C, 4)
    got = call_device(plugin, clip, mask, gpu_device)
    assert np.array_equal(got, both), f"{mode}: {int((got != both).sum())} bytes differ from composite(regrain(fill))"
    assert np.array_equal(call_list(plugin, clip, mask), both)
    assert np.array_equal(got[:, C == 0], clip[:, C == 0])
    monkeypatch.setenv("VSR_REGRAIN", "0")
    assert np.array_equal(call_device(plugin, clip, mask, gpu_device), fs.composite(fill, clip, C, 4)), "the feather alone is as it was"


def test_sttn_auto(built_lib, gpu_device, plugins, monkeypatch):
    """STTNInpaint.__call__ (list form) and the strip-rows form of the chunk loops: the samples are taken in the hull of the inpaint
    areas' rows, in full-frame coordinates, so the rows handed to the engine come back as the rows of the full-frame result"""
    H, W, box = geometry("sttn-auto")
    plugin = plugins("sttn-auto")
    clip = noisy_clip(N_BATCH, H, W, box, seed=5)
    tall = np.zeros((H, W), np.uint8)
    tall[100:230, 60:380] = 255                                    # 130 rows, the strip has int(432 * 3 / 16) = 81
    for mask in (mask_of("sttn-auto"), tall):
        both_off(monkeypatch)
        fill = call_list(plugin, clip, mask)
        assert (fill != clip).any()
        C, R = plugin.composite_mask(mask), plugin.sample_rows(mask)
        assert R == rs.sample_rows("sttn-auto", mask) and 0 < R[0] < R[1] <= H and not C[:R[0]].any() and not C[R[1]:].any()
        monkeypatch.setenv("VSR_REGRAIN", "100")
        want = rs.regrain(fill, clip, C, R, 100)
        got = call_list(plugin, clip, mask)
        assert np.array_equal(got, want) and not np.array_equal(got, fill)
        monkeypatch.setenv("VSR_SEAM_FEATHER", "4")
        both = fs.composite(want, clip, C, 4)
        assert np.array_equal(call_list(plugin, clip, mask), both)
    # the rows form, on the tall mask (both options still set)
    m = threshold_mask(tall)
    areas = get_inpaint_area_by_mask(W, H, int(W * 3 / 16), m)
    y_lo, y_hi = min(a[0] for a in areas), max(a[1] for a in areas)
    assert (y_lo, y_hi) == R and 0 < y_lo and y_hi < H
    rows = torch.from_numpy(np.ascontiguousarray(clip[:, y_lo:y_hi])).to(gpu_device)
    dmask = torch.from_numpy(np.ascontiguousarray(m[y_lo:y_hi, :, 0])).to(gpu_device)
    local = [(a[0] - y_lo, a[1] - y_lo, a[2], a[3]) for a in areas]
    plugin.auto_chunk(rows, dmask, local, cmask=C, rows=(y_lo, y_hi), mask_host=m[y_lo:y_hi, :, 0])
    torch.cuda.synchronize()
    assert np.array_equal(rows.cpu().numpy(), both[:, y_lo:y_hi]), "strip rows: the full-frame definition"


def test_lama_single_frame(built_lib, gpu_device, plugins, monkeypatch):
    """LamaInpaint.inpaint: the single picture and propainter's single-frame fall-back"""
    H, W, box = geometry("lama")
    frame = noisy_clip(1, H, W, box, seed=9, mode="lama")[0]
    mask = mask_of("lama")
    plugin = plugins("lama")
    both_off(monkeypatch)
    keep = frame.copy()
    fill = plugin.inpaint(frame, mask)
    monkeypatch.setenv("VSR_REGRAIN", "100")
    got = plugin.inpaint(frame, mask)
    assert np.array_equal(frame, keep)
    info = []
    want = rs.regrain(fill[None], frame[None], plugin.composite_mask(mask), (0, H), 100, info=info)[0]
    print("lama single frame (A_src, A_fill, changed, r, seed, touched):", info)
    assert np.array_equal(got, want) and np.array_equal(got, fill) == (info[0][3] == 0)


def test_the_sample_sets_are_cached(built_lib, gpu_device, plugins, monkeypatch):
    from vsr_amd.backend.tools import regrain

    H, W, box = geometry("opencv")
    clip = noisy_clip(2, H, W, box, seed=3)
    mask = mask_of("opencv")
    plugin = plugins("opencv")
    both_off(monkeypatch)
    before = dict(regrain.stats)
    call_device(plugin, clip, mask, gpu_device)
    assert regrain.stats == before, "option off: nothing of regrain runs"
    monkeypatch.setenv("VSR_REGRAIN", "100")
    call_device(plugin, clip, mask, gpu_device)
    builds = regrain.stats["set_builds"]
    call_device(plugin, clip, mask, gpu_device)
    assert regrain.stats["set_builds"] == builds and regrain.stats["set_hits"] > before["set_hits"]
    assert regrain.stats["calls"] == before["calls"] + 2


# ---- file to file -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["sttn-det", "opencv"])
def test_every_loop_writes_the_same_file(built_lib, gpu_device, plugins, tmp_path, monkeypatch, mode):
    """P = 100: the host-frame loop, the HBM-resident loop and resident windows (a budget of 2 x 10 frames) write the same bytes, and
    not the bytes of a run with the option off"""
    H, W, box = geometry(mode)
    src = str(tmp_path / "in.y4m")
    clip = make_clip(H, W, box)
    rng = np.random.default_rng(12)
    clip = np.clip(clip.astype(np.int64) + np.rint(rng.normal(0, 6, clip.shape)).astype(np.int64), 0, 255).astype(np.uint8)
    write_source(src, clip, monkeypatch)
    Det = make_detector(box)
    plugin = plugins(mode)
    gb = repr((2 * PER_WINDOW * H * W * 3 + 1024) / 2 ** 30)
    with config_values():
        both_off(monkeypatch)
        off, _ = run(src, str(tmp_path / "off.y4m"), plugin, Det(), monkeypatch, "1")
        monkeypatch.setenv("VSR_REGRAIN", "100")
        host, sr_host = run(src, str(tmp_path / "host.y4m"), plugin, Det(), monkeypatch, "0")
        resident, sr_res = run(src, str(tmp_path / "resident.y4m"), plugin, Det(), monkeypatch, "1")
        windows, sr_win = run(src, str(tmp_path / "windows.y4m"), plugin, Det(), monkeypatch, "windows", gb)
    assert "read + inpainting + write (host frames)" in sr_host.phase_seconds
    assert "read + inpainting + write (host frames)" not in sr_res.phase_seconds and sr_res.resident_windows is None
    assert sr_win.resident_windows is not None and len(sr_win.resident_windows["windows"]) >= 3
    assert host == resident == windows
    assert resident != off and len(resident) == len(off)
