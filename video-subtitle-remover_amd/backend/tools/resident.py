"""The decoded video resident in HBM for the detector-driven modes (sttn-det, lama, propainter).

The reference walks the file up to three times on the CPU -- the detector pass (tools/subtitle_detect.py:84-132), the scene-cut pass of
the propainter mode (:158-170), the inpainting pass (main.py:159-245, :260-333) -- decoding every frame each time, and every plugin
call copies its batch to the GPU and back.  With 288 GB of HBM a whole clip fits on the device (a 1080p frame is 6.2 MB as BGR:
1200 frames = 7.5 GB): the stored planes go up ONCE (half the bytes of the BGR frames), vsr_io_yuv_to_bgr converts them there, the
detector samples its frames from that tensor, the scene-cut kernels read it, the plugins work in place on slices of it, and
vsr_io_bgr_to_yuv + one download per batch feed the writer.  The host touches no pixel (round 2 had this for
sttn-auto only).

Eligible: a raw planar source and sink whose colour conversion runs on the GPU (*.y4m, tools/video_io.py), one process, and a clip
that fits VSR_RESIDENT_GB (default 64) as BGR.  Anything else keeps the host-frame loop; VSR_IO_RESIDENT=0 forces it.
VSR_IO_RESIDENT=windows: a clip that does not fit runs as a sequence of resident windows instead (tools/resident_windows.py).
"""
import os

import torch

from .video_io import device_planes_to_bgr


class ResidentClip:
    BATCH = 32

    def __init__(self, frames, fmt_in, planes=None):
        self.frames = frames                     # uint8 [N,H,W,3] BGR on the device
        self.fmt_in = fmt_in
        self.planes = planes                     # uint8 [N,frame_bytes]: the stored records, kept for a writer that keeps untouched samples

    @staticmethod
    def formats(reader, writer):
        """(reader planes format, writer planes format) or None"""
        if os.environ.get("VSR_IO_RESIDENT", "1") == "0":
            return None
        rf, wf = getattr(reader, "planes_format", None), getattr(writer, "planes_format", None)
        rf, wf = (rf() if rf is not None else None), (wf() if wf is not None else None)
        return (rf, wf) if rf is not None and wf is not None else None

    @staticmethod
    def fits(n, H, W, keep_bytes=0):
        """keep_bytes: bytes of a stored record when the records stay in HBM next to the BGR frames (a keeping writer), else 0"""
        return n * (H * W * 3 + keep_bytes) <= float(os.environ.get("VSR_RESIDENT_GB", "64")) * 2 ** 30

    @classmethod
    def load(cls, reader, rf, n, H, W, device, keep_planes=False):
        """read the stored planes of the whole clip, BATCH frames at a time through two pinned buffers, convert on the device.
        keep_planes: the records stay in HBM (uploaded straight into one tensor, converted from it) for store()'s keep rule."""
        dev = torch.device(device)
        frames = torch.empty((n, H, W, 3), dtype=torch.uint8, device=dev)
        pins = [torch.empty((cls.BATCH, rf["frame_bytes"]), dtype=torch.uint8).pin_memory() for _ in range(2)]
        planes = torch.empty((n, rf["frame_bytes"]), dtype=torch.uint8, device=dev) if keep_planes else None
        dplanes = [torch.empty((cls.BATCH, rf["frame_bytes"]), dtype=torch.uint8, device=dev) for _ in range(2)] if planes is None else None
        events = [None, None]
        got, b = 0, 0
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev)
            while got < n:
                if events[b] is not None:
                    events[b].synchronize()          # the upload + conversion that last used this pair of buffers is done
                want = min(cls.BATCH, n - got)
                k = reader.read_planes_into(pins[b].numpy()[:want])
                if k:
                    up = dplanes[b] if planes is None else planes[got:]
                    up[:k].copy_(pins[b][:k], non_blocking=True)
                    device_planes_to_bgr(rf, up.data_ptr(), H, W, frames[got:].data_ptr(), k, stream.cuda_stream)
                    events[b] = torch.cuda.Event()
                    events[b].record(stream)
                got += k
                b ^= 1
                if k < want:                         # a short file: the clip ends with the frames read (reference :259-261)
                    frames = frames[:got]
                    break
            torch.cuda.synchronize(dev)
        return cls(frames, rf, planes[:got] if planes is not None else None)

    def __len__(self):
        return int(self.frames.shape[0])


class StreamingStore:
    """Writes the frames of a ResidentClip in order AS THEY BECOME FINAL, on its own thread and stream.

    The batches of a detector-driven run are inpainted in frame order and nothing after batch j touches a frame in front of batch
    j + 1, so the conversion, download and file write of what is finished run under the inpainting of what is not -- the
    reference writes every batch as soon as its plugin call returns (main.py:239-245, :326-332); round 3's resident path wrote the
    whole clip after the last batch (1.0 s of a 12.3 s run at 1080p x 1200, profiles/r03_e2e_configs_3_4.log).

        st = StreamingStore(clip, writer, wf, tick)
        st.ready(hi, event)      frames [.., hi) are final once `event` (a torch.cuda.Event, or None = now) has completed
        st.finish()              everything up to len(clip); joins the thread, re-raises its error"""

    def __init__(self, clip, writer, wf, tick=None):
        from .resident_windows import Window, WindowStore

        # the whole clip as one window of tools/resident_windows.WindowStore: one conversion / download / write loop for both paths
        _, H, W, _ = clip.frames.shape
        self._win = Window(0, clip.frames, clip.planes, clip.fmt_in, None)
        self._store = WindowStore(writer, wf, H, W, clip.frames.device, ResidentClip.BATCH, tick, name="vsr-streaming-store",
                                  path="the resident clip")

    def ready(self, hi, event=None):
        self._store.ready(self._win, hi, event)

    def abort(self):
        """the run failed: stop writing, release the thread"""
        self._store.abort()

    def finish(self):
        self._store.finish(self._win)
