"""The kernels of the source-format *.y4m transport (csrc/io_kernels.hip: vsr_io_planes_to_bgr / vsr_io_bgr_to_planes) against the
numpy statements of backend/tools/video_io.py (decode_record / encode_frame / keep_record), bit for bit; and VSR_Y4M_OUT=source
through every loop that writes a *.y4m: the same file from each, the file the keep rule defines, the input itself when nothing
changes."""
import ctypes as C
import filecmp

import numpy as np
import pytest

from tests.test_y4m_formats import KEEP_CASES, fmt_of, keep_inputs, random_record, read_all, records_of, tag_of, write_raw_y4m
from vsr_amd.backend.tools import video_io

pytestmark = pytest.mark.gpu


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def dev_decode(lib, recs, fmt):
    """recs uint8 [n, frame_bytes] -> uint8 [n,H,W,3] through vsr_io_planes_to_bgr"""
    import torch

    d = torch.from_numpy(np.ascontiguousarray(recs)).cuda()
    out = torch.empty((d.shape[0], fmt["H"], fmt["W"], 3), dtype=torch.uint8, device="cuda")
    rc = lib.vsr_io_planes_to_bgr(_ptr(d), d.shape[1], fmt["H"], fmt["W"], fmt["cw"], fmt["ch"], fmt["depth"], int(fmt["full_range"]),
                                  _ptr(out), d.shape[0], None)
    assert rc == 0
    torch.cuda.synchronize()
    return out.cpu().numpy()


def dev_encode(lib, frames, fmt, src=None, in_place=False):
    """frames uint8 [n,H,W,3] (+ source records [n, frame_bytes]) -> records through vsr_io_bgr_to_planes"""
    import torch

    d = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    fb = video_io.record_bytes(fmt)
    s = torch.from_numpy(np.ascontiguousarray(src)).cuda() if src is not None else None
    out = s if in_place else torch.full((d.shape[0], fb), 0xA5, dtype=torch.uint8, device="cuda")
    rc = lib.vsr_io_bgr_to_planes(_ptr(d), fmt["H"], fmt["W"], fmt["cw"], fmt["ch"], fmt["depth"], int(fmt["full_range"]),
                                  _ptr(s) if s is not None else None, fb if s is not None else 0, _ptr(out), fb, d.shape[0], None)
    assert rc == 0
    torch.cuda.synchronize()
    return out.cpu().numpy()


ALL_FORMATS = [(c, d, f) for c in ("420", "422", "444", "mono") for d in (8, 10, 12) for f in (False, True)]


# ---- check 7 --------------------------------------------------------------------------------------------------------------------
def test_kernels_equal_the_statements_every_format(built_lib, gpu_device):
    """both directions, every chroma layout x depth x range, odd sizes (edge replication, unaligned rows, partial tiles)"""
    lib = built_lib.lib
    for H, W in ((37, 53), (2, 2), (1, 1), (5, 16)):
        for chroma, depth, full in ALL_FORMATS:
            fmt = fmt_of(chroma, depth, full, H, W)
            rng = np.random.default_rng(H * W + depth + int(full))
            recs = np.stack([random_record(rng, fmt, hi=(1 << 16) if (depth > 8 and k == 1) else None) for k in range(2)])
            got = dev_decode(lib, recs, fmt)
            for k in range(2):
                assert np.array_equal(got[k], video_io.decode_record(recs[k], fmt)), (H, W, chroma, depth, full, "decode")
            frames = rng.integers(0, 256, size=(2, H, W, 3), dtype=np.uint8)
            got = dev_encode(lib, frames, fmt)
            for k in range(2):
                assert np.array_equal(got[k], video_io.encode_frame(frames[k], fmt)), (H, W, chroma, depth, full, "encode")


def test_kernels_equal_the_statements_1080p(built_lib, gpu_device):
    lib = built_lib.lib
    H, W = 1080, 1920
    fmt = fmt_of("420", 10, False, H, W)
    rng = np.random.default_rng(1080)
    recs = np.stack([random_record(rng, fmt) for _ in range(2)])
    got = dev_decode(lib, recs, fmt)
    want = [video_io.decode_record(r, fmt) for r in recs]
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    frames = np.stack(want)
    frames[0, 900:1000, 300:1500] = rng.integers(0, 256, size=(100, 1200, 3), dtype=np.uint8)
    enc = dev_encode(lib, frames, fmt)
    assert np.array_equal(enc[0], video_io.encode_frame(frames[0], fmt))
    keep = dev_encode(lib, frames, fmt, src=recs)
    assert np.array_equal(keep[0], video_io.keep_record(recs[0], frames[0], fmt))
    assert np.array_equal(keep[1], recs[1])                      # the untouched frame comes back as stored


@pytest.mark.parametrize("full", [False, True])
def test_decode_value_coverage(built_lib, gpu_device, full):
    """depth 10: every (Y, U) pair with V over 8 values and every (Y, V) pair with U over 8 values; depth 12: every value of each
    plane plus 2^24 random triples"""
    lib = built_lib.lib
    H, W = 2048, 4096
    fmt = fmt_of("444", 10, full, H, W)
    idx = np.arange(H * W, dtype=np.int64)
    a, b = idx & 1023, (idx >> 10) & 1023
    third = np.array([0, 64, 300, 511, 512, 700, 960, 1023])[idx >> 20]
    for planes in ((a, b, third), (a, third, b)):
        rec = np.concatenate(planes).astype("<u2").view(np.uint8)
        assert np.array_equal(dev_decode(lib, rec[None], fmt)[0], video_io.decode_record(rec, fmt))
    H = W = 4096
    fmt = fmt_of("444", 12, full, H, W)
    rng = np.random.default_rng(12 + int(full))
    planes = rng.integers(0, 4096, size=(3, H * W))
    for k in range(3):
        planes[k, :4096] = np.arange(4096)
    rec = planes.reshape(-1).astype("<u2").view(np.uint8)
    assert np.array_equal(dev_decode(lib, rec[None], fmt)[0], video_io.decode_record(rec, fmt))


@pytest.mark.parametrize("depth", [8, 10, 12])
def test_encode_all_bgr_triples(built_lib, gpu_device, depth):
    from tests.test_y4m_formats import all_triples

    t = all_triples()
    for full in (False, True):
        fmt = fmt_of("444", depth, full, 4096, 4096)
        got = dev_encode(built_lib.lib, t[None], fmt)[0]
        assert np.array_equal(got, video_io.encode_frame(t, fmt))
        if depth > 8:                                            # lossless carriage, on the device as well
            assert np.array_equal(dev_decode(built_lib.lib, got[None], fmt)[0], t)


def test_depth_8_equals_the_8_bit_entry_points(built_lib, gpu_device):
    """depth 8 without source records: vsr_io_planes_to_bgr / vsr_io_bgr_to_planes == vsr_io_yuv_to_bgr / vsr_io_bgr_to_yuv"""
    import torch

    lib = built_lib.lib
    for H, W in ((37, 53), (270, 480)):
        for chroma in ("420", "422", "444", "mono"):
            for full in (False, True):
                fmt = fmt_of(chroma, 8, full, H, W)
                rng = np.random.default_rng(H + len(chroma))
                recs = np.stack([random_record(rng, fmt) for _ in range(2)])
                d = torch.from_numpy(recs).cuda()
                old = torch.empty((2, H, W, 3), dtype=torch.uint8, device="cuda")
                assert lib.vsr_io_yuv_to_bgr(_ptr(d), d.shape[1], H, W, fmt["cw"], fmt["ch"], int(full), _ptr(old), 2, None) == 0
                torch.cuda.synchronize()
                assert np.array_equal(dev_decode(lib, recs, fmt), old.cpu().numpy())
                if chroma in ("420", "444"):
                    frames = rng.integers(0, 256, size=(2, H, W, 3), dtype=np.uint8)
                    df = torch.from_numpy(frames).cuda()
                    oldp = torch.empty((2, d.shape[1]), dtype=torch.uint8, device="cuda")
                    assert lib.vsr_io_bgr_to_yuv(_ptr(df), H, W, int(chroma == "420"), int(full), _ptr(oldp), d.shape[1], 2, None) == 0
                    torch.cuda.synchronize()
                    assert np.array_equal(dev_encode(lib, frames, fmt), oldp.cpu().numpy())


# ---- check 8 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chroma,depth,full", KEEP_CASES)
def test_keep_kernel_equals_the_keep_statement(built_lib, gpu_device, chroma, depth, full):
    lib = built_lib.lib
    cases = [keep_inputs(chroma, depth, full, seed=s) for s in range(3)]      # a different rectangle per frame
    fmt = cases[0][0]
    src = np.stack([c[1] for c in cases] + [cases[0][1]])
    frames = np.stack([c[3] for c in cases] + [cases[0][2]])                  # (the last frame is the decoded source itself)
    want = np.stack([video_io.keep_record(s, f, fmt) for s, f in zip(src, frames)])
    assert np.array_equal(want[3], src[3]) and not np.array_equal(want[0], src[0])
    got = dev_encode(lib, frames, fmt, src=src)
    assert np.array_equal(got, want)
    assert np.array_equal(dev_encode(lib, frames, fmt, src=src, in_place=True), want)      # include/vsr_hip.h: in place works
    assert np.array_equal(dev_encode(lib, frames[:1], fmt, src=src[:1]), want[:1])


def test_partial_overlap_is_refused(built_lib, gpu_device):
    import torch

    fmt = fmt_of("420", 8, False, 4, 4)
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    bgr = torch.zeros((2, 4, 4, 3), dtype=torch.uint8, device="cuda")
    rc = built_lib.lib.vsr_io_bgr_to_planes(_ptr(bgr), 4, 4, 2, 2, 8, 0, C.c_void_p(buf.data_ptr() + 8), 24, _ptr(buf), 24, 2, None)
    assert rc == built_lib.VSR_ERR_ARG


def test_writer_and_reader_on_the_device_equal_numpy(built_lib, gpu_device, tmp_path, monkeypatch):
    """Y4mVideo.read() of 10 / 12-bit files and Y4mWriter(like=...) with the GPU colour conversion == the host statements: the batches
    of _DeviceColor, a sink longer than its source (plain encoding behind the last source record)"""
    for chroma, depth, full in (("420", 10, False), ("422", 12, True), ("444", 10, True), ("mono", 10, False), ("420", 8, True)):
        fmt, src, D, F, _ = keep_inputs(chroma, depth, full)
        H, W = fmt["H"], fmt["W"]
        rng = np.random.default_rng(depth)
        recs = [src] + [random_record(rng, fmt) for _ in range(10)]
        sp = str(tmp_path / f"src_{chroma}_{depth}.y4m")
        write_raw_y4m(sp, recs, fmt, tag_of(chroma, depth))
        out = {}
        for mode in ("host", "device"):
            monkeypatch.setenv("VSR_IO_COLOR", mode)
            r = video_io.Y4mVideo(sp)
            assert (r._dc is not None) == (mode == "device")
            r.release()
            frames = read_all(sp)
            frames[0] = F
            p = str(tmp_path / f"{mode}_{chroma}_{depth}.y4m")
            w = video_io.Y4mWriter(p, 25.0, (W, H), like=sp)
            assert (w._dc is not None) == (mode == "device")
            for f in list(frames) + [F, D]:                       # two frames more than the source has
                w.write(f)
            w.release()
            out[mode] = (frames, open(p, "rb").read())
        assert np.array_equal(out["host"][0], out["device"][0])
        assert out["host"][1] == out["device"][1]
        got = records_of(str(tmp_path / f"device_{chroma}_{depth}.y4m"), fmt)
        assert len(got) == 13 and np.array_equal(got[0], video_io.keep_record(src, F, fmt))
        assert all(np.array_equal(got[k], recs[k]) for k in range(1, 11))
        assert np.array_equal(got[11], video_io.encode_frame(F, fmt))


# ---- checks 9 - 12: the loops -----------------------------------------------------------------------------------------------------
def _make_source(path, clip, depth, tag):
    """a 4:2:0 studio-range source of the clip at `depth` bits (the plain statement makes the records)"""
    N, H, W, _ = clip.shape
    fmt = fmt_of("420", depth, False, H, W)
    write_raw_y4m(path, [video_io.encode_frame(f, fmt) for f in clip], fmt, tag)
    return fmt


@pytest.mark.parametrize("depth,tag", [(8, "420jpeg"), (10, "420p10")])
def test_source_format_same_file_from_every_sttn_auto_loop(built_lib, gpu_device, tmp_path, monkeypatch, depth, tag):
    """VSR_Y4M_OUT=source, sttn-auto, A/B sections and a ragged last chunk: host / device-frames / resident / by-offset write one file
    (check 9); that file is the keep rule applied to (source records, the frames the lossless *.npy sink received), its first line is
    the source's, outside the mask's rows every sample is the source's (check 10); sections that select no frame and a run without
    an inpaint area give back the input byte for byte (check 11)."""
    from vsr_amd import synth
    from vsr_amd.backend.config import config
    from vsr_amd.backend.main import SubtitleRemover
    from vsr_amd.backend.tools.constant import InpaintMode

    H, W, N, GAP = 480, 852, 20, 6
    box = (400, 450, 100, 760)
    clip = synth.make_clip(N, H, W, box, seed=11)
    src = str(tmp_path / "in.y4m")
    fmt = _make_source(src, clip, depth, tag)
    keys = {"sttnMaxLoadNum": GAP, "sttnNeighborStride": 1, "sttnReferenceLength": 6}
    old = {k: getattr(config, k).value for k in keys}
    old_mode = config.inpaintMode.value
    monkeypatch.setenv("VSR_Y4M_OUT", "source")
    sections = [range(2, 9), range(13, 19)]

    def run(name, color, resident, per_rank, areas, ab, ext=".y4m"):
        monkeypatch.setenv("VSR_IO_COLOR", color)
        monkeypatch.setenv("VSR_IO_RESIDENT", resident)
        monkeypatch.setenv("VSR_IO_PER_RANK", per_rank)
        sr = SubtitleRemover(src, model_path={"netG": synth.make_state_dict(0, "auto")})
        sr.sub_areas = areas
        sr.ab_sections = ab
        sr.video_out_path = str(tmp_path / f"out_{name}{ext}")
        ticks = []
        sr.update_progress = lambda tbar, increment: ticks.append(increment)
        sr.sttn_auto_mode(tbar=object())
        sr.video_writer.release()
        assert sum(ticks) == N
        return sr.video_out_path

    try:
        for k, v in keys.items():
            getattr(config, k).value = v
        config.inpaintMode.value = InpaintMode.STTN_AUTO
        outs = {name: run(name, color, resident, per_rank, [box], sections)
                for name, color, resident, per_rank in (("host", "host", "0", "0"), ("device-frames", "device", "0", "0"),
                                                        ("resident", "device", "1", "0"), ("by-offset", "device", "1", "1"))}
        npy = run("lossless", "device", "1", "0", [box], sections, ext=".npy")
        same = {name: run(name, color, resident, "0", areas, ab)
                for name, color, resident, areas, ab in (("none-selected-resident", "device", "1", [box], [range(0)]),
                                                         ("none-selected-host", "host", "0", [box], [range(0)]),
                                                         ("no-area-resident", "device", "1", [], None),
                                                         ("no-area-host", "host", "0", [], None))}
    finally:
        for k, v in old.items():
            getattr(config, k).value = v
        config.inpaintMode.value = old_mode
    want = open(outs["host"], "rb").read()
    for name, p in outs.items():
        assert open(p, "rb").read() == want, f"{name} wrote another file than the host loop"
    # check 10
    assert open(outs["resident"], "rb").readline() == open(src, "rb").readline()
    frames = np.load(npy)
    srcs, got = records_of(src, fmt), records_of(outs["resident"], fmt)
    assert len(got) == N == len(frames)
    from vsr_amd.backend.tools.inpaint_tools import create_mask

    changed = inside = 0
    my, mx = np.nonzero(create_mask((H, W), [(box[2], box[3], box[0], box[1])]))      # the run's mask (sttn_auto_mode), its bounding box ...
    y0, y1, x0, x1 = my.min() // 2 * 2, (my.max() + 2) // 2 * 2, mx.min() // 2 * 2, (mx.max() + 2) // 2 * 2      # ... grown to chroma blocks
    assert (y0, y1, x0, x1) != (0, H, 0, W)
    for k in range(N):
        assert np.array_equal(got[k], video_io.keep_record(srcs[k], frames[k], fmt)), f"frame {k} is not the keep rule's record"
        (yo, uo, vo), (ys, us, vs) = video_io.split_record(got[k], fmt), video_io.split_record(srcs[k], fmt)
        for o, s, d in ((yo, ys, 1), (uo, us, 2), (vo, vs, 2)):
            out = np.ones(o.shape, bool)
            out[y0 // d: y1 // d, x0 // d: x1 // d] = False
            assert np.array_equal(o[out], s[out]), f"frame {k}: a sample outside the mask's box is not the source's"
        changed += int((yo[box[0]:box[1], box[2]:box[3]] != ys[box[0]:box[1], box[2]:box[3]]).sum())
        inside += (box[1] - box[0]) * (box[3] - box[2])
        if not any(k in r for r in sections):
            assert np.array_equal(got[k], srcs[k])                 # outside the sections: the stored frame
    assert changed / inside > 0.15, "something was inpainted"
    # check 11
    for name, p in same.items():
        assert filecmp.cmp(p, src, shallow=False), f"{name}: a run that changes nothing must write its input back"


@pytest.mark.parametrize("mode", ["sttn-det", "opencv"])
@pytest.mark.parametrize("depth,tag", [(8, "420jpeg"), (10, "420p10")])
def test_source_format_same_file_from_the_detector_loops(built_lib, gpu_device, tmp_path, monkeypatch, depth, tag, mode):
    """VSR_Y4M_OUT=source in a detector-driven mode: the HBM-resident clip (planes kept next to the BGR tensor) writes the host loop's
    file (check 9); a VSR_RESIDENT_GB that holds the BGR tensor but not BGR + planes sends the run to the host-frame loop, same file
    (check 12); frames without a subtitle come back as stored."""
    from vsr_amd import synth
    from vsr_amd.backend.config import config
    from vsr_amd.backend.main import SubtitleRemover
    from vsr_amd.backend.tools.constant import InpaintMode
    from vsr_amd.backend.tools.resident import ResidentClip

    H, W, N = 240, 432, 34
    box = (180, 214, 60, 380)
    clip = synth.make_clip(N, H, W, box, seed=5)
    on = [i for i in range(N) if 3 <= i < 15 or i >= 22]
    plain = synth.make_clip(N, H, W, (0, 1, 0, 1), seed=5)
    for i in range(N):
        if i not in on:
            clip[i] = plain[i]
    src = str(tmp_path / "in.y4m")
    fmt = _make_source(src, clip, depth, tag)
    quad = np.array([[[box[2], box[0]], [box[3], box[0]], [box[3], box[1]], [box[2], box[1]]]])

    class Det:
        batch_size = 4

        def predict(self, img):
            white = (img[box[0] + 8:box[1] - 8, box[2] + 8:box[3] - 8] > 200).mean()
            return [{"dt_polys": quad if white > 0.05 else np.zeros((0, 4, 2), np.int32)}]

    if mode == "sttn-det":
        from vsr_amd.backend.inpaint.sttn_det_inpaint import STTNDetInpaint
        plugin = STTNDetInpaint("cuda:0", {"netG": synth.make_state_dict(0, "det")})
    else:
        from vsr_amd.backend.inpaint.opencv_inpaint import OpenCVInpaint
        plugin = OpenCVInpaint("cuda:0")
    bgr_bytes, rec_bytes = N * H * W * 3, N * video_io.record_bytes(fmt)
    tight = (bgr_bytes + rec_bytes // 2) / 2 ** 30                # room for the BGR tensor, not for BGR + planes
    old_mode, old_load = config.inpaintMode.value, config.sttnMaxLoadNum.value
    monkeypatch.setenv("VSR_Y4M_OUT", "source")
    outs, phases = {}, {}
    try:
        config.inpaintMode.value = InpaintMode.STTN_DET if mode == "sttn-det" else InpaintMode.OPENCV
        config.sttnMaxLoadNum.value = 8
        for how, color, resident, gb in (("host", "host", "0", None), ("resident", "device", "1", None), ("tight", "device", "1", tight)):
            monkeypatch.setenv("VSR_IO_COLOR", color)
            monkeypatch.setenv("VSR_IO_RESIDENT", resident)
            if gb is None:
                monkeypatch.delenv("VSR_RESIDENT_GB", raising=False)
            else:
                monkeypatch.setenv("VSR_RESIDENT_GB", repr(gb))
                assert ResidentClip.fits(N, H, W) and not ResidentClip.fits(N, H, W, video_io.record_bytes(fmt))
            sr = SubtitleRemover(src, device="cuda:0")
            sr.sub_areas = [(0, H, 0, W)]
            sr.video_out_path = str(tmp_path / f"out_{how}.y4m")
            ticks = []
            sr.update_progress = lambda tbar, increment: ticks.append(increment)
            sr.video_inpaint(object(), plugin, text_detector=Det())
            sr.video_writer.release()
            outs[how] = open(sr.video_out_path, "rb").read()
            phases[how] = dict(sr.phase_seconds)
            assert sum(ticks) == N
    finally:
        config.inpaintMode.value, config.sttnMaxLoadNum.value = old_mode, old_load
        if hasattr(plugin, "close"):
            plugin.close()
    assert "read + upload + YUV->BGR" in phases["resident"] and "read + upload + YUV->BGR" not in phases["host"]
    assert "read + upload + YUV->BGR" not in phases["tight"], "BGR + planes do not fit: the host-frame loop runs"
    assert outs["host"] == outs["resident"] == outs["tight"]
    assert outs["host"].split(b"\n", 1)[0] == open(src, "rb").readline().rstrip(b"\n")
    srcs, got = records_of(src, fmt), records_of(str(tmp_path / "out_resident.y4m"), fmt)
    differ = np.array([not np.array_equal(a, b) for a, b in zip(srcs, got)])
    assert differ[on].mean() > 0.7 and len(got) == N
    for k in range(N):
        ys, yo = video_io.split_record(srcs[k], fmt)[0], video_io.split_record(got[k], fmt)[0]
        if mode == "opencv":                                     # Telea changes masked pixels only (the box grown by config's 10 pixels)
            assert np.array_equal(yo[: box[0] - 24], ys[: box[0] - 24]) and np.array_equal(yo[box[1] + 24:], ys[box[1] + 24:])
        else:                                                    # STTN works on strips of W * 3 / 16 rows that hold the mask: nothing above them
            top = box[0] - 10 - W * 3 // 16
            assert top > 64 and np.array_equal(yo[:top], ys[:top])
