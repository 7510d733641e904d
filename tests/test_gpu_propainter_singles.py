"""propainter_mode with an injected single_frame_inpaint on all three drive paths: the host-frame loop, the HBM-resident clip and
resident windows read the one walk of tools/frame_walk.py, so they hand the single-frame plugin the same frames in the same order
and write the same file.

The clip is the one of tests/test_gpu_resident_windows.py with its number stamped into a corner of every frame; the detector and the
single-frame plugin read it there.  The detector is scripted (25 fps: every second frame is sampled, holes of up to four frames are
filled): the box on frames 5..15, on frame 21 alone, and on frames 27..33 (1-based).  Scene starts at 10 and 15 cut the first interval
into 5..9, 10..14 and the single frame 15; 21 is a single frame by detection."""
import numpy as np
import pytest

from tests.test_gpu_resident_windows import N, budget_gb, config_values, make_clip, write_source

pytestmark = pytest.mark.gpu

STEP = 7                                                          # grey levels between two frame numbers: the 4:2:0 round trip moves a level by one or two
BOXED = set(range(5, 16)) | {21} | set(range(27, 34))            # 1-based frame numbers the scripted detector answers with the box
SCENE_STARTS = [10, 15]
SINGLES = [14, 20]                                                # 0-based: frame 15 (cut off by the scene start) and frame 21


def frame_number(frame):
    return int(round(float(frame[:8, :8].mean()) / STEP))


def test_single_frames_on_host_resident_and_windowed_paths(built_lib, gpu_device, tmp_path, monkeypatch):
    from vsr_amd.backend.inpaint.opencv_inpaint import OpenCVInpaint
    from vsr_amd.backend.main import SubtitleRemover

    H, W, box = 240, 432, (180, 214, 60, 380)
    clip = make_clip(H, W, box)
    for i in range(N):
        clip[i, :8, :8] = STEP * i
    src = str(tmp_path / "in.y4m")
    write_source(src, clip, monkeypatch)
    quad = np.array([[[box[2], box[0]], [box[3], box[0]], [box[3], box[1]], [box[2], box[1]]]])

    class Det:                                                    # the reference's host signature
        batch_size = 4

        def predict(self, img):
            return [{"dt_polys": quad if frame_number(img) + 1 in BOXED else np.zeros((0, 4, 2), np.int32)}]

    plugin = OpenCVInpaint("cuda:0")
    gb = budget_gb(H, W)
    runs = {}
    with config_values("propainter"):
        for name, resident, budget in (("host", "0", None), ("resident", "1", None), ("windows", "windows", gb)):
            monkeypatch.setenv("VSR_IO_COLOR", "device")
            monkeypatch.setenv("VSR_IO_RESIDENT", resident)
            if budget is None:
                monkeypatch.delenv("VSR_RESIDENT_GB", raising=False)
            else:
                monkeypatch.setenv("VSR_RESIDENT_GB", budget)
            calls = []

            def single_frame_inpaint(frame, mask, calls=calls):
                assert isinstance(frame, np.ndarray) and frame.shape == (H, W, 3) and mask.shape == (H, W)
                calls.append((frame_number(frame), int(mask.sum())))
                out = frame.copy()
                out[mask > 0] = 255 - out[mask > 0]
                return out

            sr = SubtitleRemover(src, device="cuda:0")
            sr.sub_areas = [(0, H, 0, W)]
            sr.video_out_path = str(tmp_path / f"{name}.y4m")
            ticks = []
            sr.update_progress = lambda tbar, increment, ticks=ticks: ticks.append(increment)
            sr.propainter_mode(object(), propainter_inpaint=plugin, text_detector=Det(), scene_div_points=SCENE_STARTS,
                               single_frame_inpaint=single_frame_inpaint)
            sr.video_writer.release()
            assert sum(ticks) == N
            runs[name] = (open(sr.video_out_path, "rb").read(), calls, sr)
    host, resident, windows = runs["host"], runs["resident"], runs["windows"]
    assert "read + upload + YUV->BGR" in resident[2].phase_seconds and "read + upload + YUV->BGR" not in host[2].phase_seconds
    assert host[2].resident_windows is None and resident[2].resident_windows is None
    assert windows[2].resident_windows is not None and len(windows[2].resident_windows["windows"]) >= 3
    assert [no for no, _ in host[1]] == SINGLES and host[1][0][1] == host[1][1][1] > 0
    assert resident[1] == host[1] and windows[1] == host[1], "the single-frame plugin saw other frames, or in another order"
    assert [r[2].passed_through_single_frames for r in (host, resident, windows)] == [0, 0, 0]
    assert resident[0] == host[0] and windows[0] == host[0], "the three drive paths must write the same file"
    assert host[0] != open(src, "rb").read()
