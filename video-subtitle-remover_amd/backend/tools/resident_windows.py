"""Clips that do not fit VSR_RESIDENT_GB on the HBM-resident path of the detector-driven modes: a sequence of resident WINDOWS.

tools/resident.py keeps the whole decoded clip in HBM; a clip over the budget used to fall back to the host-frame loop (two or three
host decodes, BGR frames over PCIe in both directions).  With VSR_IO_RESIDENT=windows (--resident-windows) such a clip runs in two
passes over the file, every pixel on the device in both:

  pass A   the detector's sampled frames (and, for propainter, every frame for the scene-cut kernels) go through HBM a window at a
           time and are dropped again: SubtitleDetect._find_windowed, scene_detect.SceneStream.  Without scene cuts only the sampled
           records are read (Y4mVideo.skip_records passes over the others), whole detector batches per window; with them the
           windows are cut by frame count and a batch that lies in several (across the hole between two A/B sections, say) is
           gathered in a side buffer of one batch.
  pass B   plan_windows() cuts [0, N) into consecutive windows that no batch straddles; window k + 1 is read, uploaded and converted
           on the loader's thread and stream while the plugins inpaint window k in place, and WindowStore writes window k's frames in
           order as they become final.  Two window buffers exist; a buffer is handed back to the loader when its last frame has been
           stored, so the live bytes are those of two windows: one computing, one loading or storing.

The file written is the resident path's, byte for byte: the same records reach the same kernels in the same batches.  The budget
counts what tools/resident.py counts, the BGR frames plus the stored records when the sink keeps untouched samples; the staging
buffers of the transfers (two of at most BATCH records each way) are small and, as there, not part of it.
"""
import os
import queue
import threading

BATCH = 32                  # records per upload / download, as ResidentClip.BATCH
PASS_A_FRAMES = 256         # pass A keeps nothing: its windows need not be larger than what hides the loader behind the detector


class WindowsDoNotFit(Exception):
    """a single unit of work (the frames of one detector batch, an inpainting batch) is larger than half the budget: the host-frame loop runs"""


def enabled():
    return os.environ.get("VSR_IO_RESIDENT", "1") == "windows"


def budget_bytes():
    return int(float(os.environ.get("VSR_RESIDENT_GB", "64")) * 2 ** 30)


def pass_a_reads_all():
    """VSR_WINDOWS_PASS_A=all: pass A reads every record even when no scene cuts are wanted (default: the sampled ones only)"""
    return os.environ.get("VSR_WINDOWS_PASS_A", "sampled") == "all"


def plan_windows(n, jobs, frame_bytes, budget, keep_bytes=0, max_frames=None):
    """Cut [0, n) into consecutive windows [(lo, hi)].

    jobs: [(lo, hi)] frame ranges in increasing order, disjoint -- none may straddle a window boundary.  frame_bytes (+ keep_bytes
    when the stored records stay next to the BGR frames) is what one frame holds in HBM; two windows are alive at once, so a window
    takes at most budget // 2.  Everything within the budget: one window.  A job over half the budget: None ("does not fit").
    max_frames: an upper bound on the window length beyond the budget's (pass A)."""
    n = int(n)
    if n <= 0:
        return []
    per = int(frame_bytes) + int(keep_bytes)
    if n * per <= budget and (max_frames is None or n <= max_frames):
        return [(0, n)]
    cap = int(budget) // (2 * per)
    if max_frames is not None:
        cap = min(cap, int(max_frames))
    jobs = [(max(0, int(lo)), min(n, int(hi))) for lo, hi in jobs]
    jobs = [(lo, hi) for lo, hi in jobs if hi > lo]
    if cap < 1 or any(hi - lo > cap for lo, hi in jobs):
        return None
    windows, lo, j = [], 0, 0
    while lo < n:
        hi = min(n, lo + cap)
        while j < len(jobs) and jobs[j][1] <= lo:
            j += 1
        k = j
        while k < len(jobs) and jobs[k][0] < hi:           # the furthest cut <= lo + cap that lies inside no job
            if jobs[k][1] > hi:
                hi = jobs[k][0]
                break
            k += 1
        windows.append((lo, hi))                           # hi > lo: a job that starts at lo ends within lo + cap
        lo = hi
    return windows


def live_bytes(windows, frame_bytes, keep_bytes=0):
    """the largest number of bytes two neighbouring windows (one alone, if there is only one) hold"""
    per = int(frame_bytes) + int(keep_bytes)
    sizes = [hi - lo for lo, hi in windows]
    if not sizes:
        return 0
    return per * max([sizes[0]] + [a + b for a, b in zip(sizes, sizes[1:])])


def _runs(indices):
    """sorted frame numbers -> [(first, count)] of consecutive ones"""
    runs = []
    for i in indices:
        if runs and runs[-1][0] + runs[-1][1] == i:
            runs[-1][1] += 1
        else:
            runs.append([i, 1])
    return runs


class WindowLoader:
    """Reads the records of one unit after the other (a unit: increasing 0-based frame numbers, the others are skipped) into one
    of the window buffers, on its own thread and stream: records -> pinned memory -> device -> vsr_io_yuv_to_bgr, as ResidentClip.load.

        b, count = loader.get()      the next unit is in buffer b (count < len(unit): the file ended); raises the loader's error
        loader.release(b)            buffer b may be overwritten
        loader.close()               joins the thread"""

    def __init__(self, reader, rf, H, W, device, units, bufs, planes=None):
        import torch

        self.reader, self.rf, self.H, self.W, self.units, self.bufs, self.planes = reader, rf, H, W, units, bufs, planes
        self.dev = torch.device(device)
        self.records_read = 0
        self._free, self._ready = queue.Queue(), queue.Queue()
        for b in range(len(bufs)):
            self._free.put(b)
        self._thread = threading.Thread(target=self._run, name="vsr-window-loader", daemon=True)
        self._thread.start()

    def _run(self):
        import torch

        try:
            rf, fb = self.rf, self.rf["frame_bytes"]
            batch = max(1, min(BATCH, max((len(u) for u in self.units), default=1)))
            pins = [torch.empty((batch, fb), dtype=torch.uint8).pin_memory() for _ in range(2)]
            stage = [torch.empty((batch, fb), dtype=torch.uint8, device=self.dev) for _ in range(2)] if self.planes is None else None
            pos = 0
            with torch.cuda.device(self.dev), torch.cuda.stream(torch.cuda.Stream(self.dev)):
                stream = torch.cuda.current_stream(self.dev)
                for unit in self.units:
                    b = self._free.get()
                    if b is None:
                        return
                    events, got, p, short = [None, None], 0, 0, False
                    for s in range(0, len(unit), batch):
                        want = unit[s:s + batch]
                        if events[p] is not None:
                            events[p].synchronize()          # the upload + conversion that last used this pair of buffers is done
                        k = 0
                        for first, count in _runs(want):
                            if first > pos:
                                self.reader.skip_records(first - pos)
                            r = self.reader.read_planes_into(pins[p].numpy()[k:k + count])
                            pos = first + r
                            k += r
                            if r < count:
                                short = True
                                break
                        if k:
                            up = stage[p] if self.planes is None else self.planes[b][got:]
                            up[:k].copy_(pins[p][:k], non_blocking=True)
                            from .video_io import device_planes_to_bgr

                            device_planes_to_bgr(rf, up.data_ptr(), self.H, self.W, self.bufs[b][got:].data_ptr(), k, stream.cuda_stream)
                            events[p] = torch.cuda.Event()
                            events[p].record(stream)
                        got += k
                        p ^= 1
                        if short:
                            break
                    stream.synchronize()
                    self.records_read += got
                    self._ready.put((b, got))
                    if short:
                        return
        except BaseException as e:                           # noqa: BLE001 -- re-raised by get() in the caller's thread
            self._ready.put(e)

    def fail(self, error):
        """another thread of the run failed: whoever waits in get() must hear of it"""
        self._ready.put(error)

    def get(self):
        item = self._ready.get()
        if isinstance(item, BaseException):
            raise item
        return item

    def release(self, b):
        self._free.put(b)

    def close(self):
        self._free.put(None)
        self._thread.join()


class Window:
    """frames [lo, lo + len) of the file in one of the window buffers; what ResidentClip is to SubtitleRemover._run_resident_jobs"""

    def __init__(self, lo, frames, planes, fmt_in, buf):
        self.lo, self.frames, self.planes, self.fmt_in, self.buf = lo, frames, planes, fmt_in, buf
        self.stored = 0

    def __len__(self):
        return int(self.frames.shape[0])


class WindowStore:
    """tools/resident.StreamingStore over windows: the frames of a window are converted (vsr_io_bgr_to_yuv / vsr_io_bgr_to_planes),
    downloaded and written in order as they become final, on this thread and stream; pass-through frames like any other.

        st.ready(win, hi, event)     frames [.., hi) of `win` are final once `event` has completed; windows in file order
        st.finish()                  joins the thread, re-raises its error
    on_stored(win): the window's last frame went to the writer (its buffer is free); on_error(e): the first failure."""

    def __init__(self, writer, wf, H, W, device, batch, tick=None, on_stored=None, on_error=None, name="vsr-window-store",
                 path="the resident windows"):
        import torch

        self.writer, self.wf, self.H, self.W, self.tick = writer, wf, H, W, tick
        self.dev = torch.device(device)
        self.batch = max(1, min(BATCH, int(batch)))
        self.on_stored, self.on_error, self.path = on_stored, on_error, path
        self._q = queue.Queue()
        self._error = None
        self._thread = threading.Thread(target=self._run, name=name, daemon=True)
        self._thread.start()

    def _store(self, win, lo, hi, pins, dout, stream):
        from .video_io import device_bgr_to_planes

        b = 0
        for s in range(lo, hi, self.batch):
            k = min(self.batch, hi - s)
            device_bgr_to_planes(self.wf, win.frames[s:].data_ptr(), self.H, self.W, dout[b].data_ptr(), k, stream.cuda_stream,
                                 win.planes[s:].data_ptr() if win.planes is not None else None, win.fmt_in, path=self.path)
            pins[b][:k].copy_(dout[b][:k], non_blocking=True)
            stream.synchronize()
            self.writer.write_planes(pins[b].numpy()[:k])        # the writer thread takes its own copy
            if self.tick is not None:
                for _ in range(k):
                    self.tick()
            b ^= 1

    def _run(self):
        import torch

        pins = dout = None
        with torch.cuda.device(self.dev), torch.cuda.stream(torch.cuda.Stream(self.dev)):
            stream = torch.cuda.current_stream(self.dev)
            while True:
                item = self._q.get()
                if item is None:
                    stream.synchronize()
                    return
                if self._error is not None:       # after a failed write: drain the queue until the sentinel, write nothing more
                    continue
                try:
                    win, hi, event = item
                    if pins is None:
                        fb = self.wf["frame_bytes"]
                        pins = [torch.empty((self.batch, fb), dtype=torch.uint8).pin_memory() for _ in range(2)]
                        dout = [torch.empty((self.batch, fb), dtype=torch.uint8, device=self.dev) for _ in range(2)]
                    if event is not None:
                        event.synchronize()
                    hi = min(int(hi), len(win))
                    if hi > win.stored:
                        self._store(win, win.stored, hi, pins, dout, stream)
                        win.stored = hi
                        if hi == len(win) and self.on_stored is not None:
                            self.on_stored(win)
                except BaseException as e:        # noqa: BLE001 -- re-raised by ready() / finish() in the caller's thread
                    self._error = e
                    if self.on_error is not None:
                        self.on_error(e)

    def ready(self, win, hi, event=None):
        if self._error is not None:               # fail fast: do not inpaint the rest of the clip for a file that cannot be written
            raise self._error
        self._q.put((win, hi, event))

    def handle(self, win):
        """the store as SubtitleRemover._run_resident_jobs sees it: ready(hi, event) in frames of this window"""
        return _Handle(self, win)

    def abort(self):
        """the run failed: stop writing, release the thread"""
        self._q.put(None)
        self._thread.join()

    def finish(self, last=None):
        """last: a window whose frames are all final now (the whole clip of tools/resident.StreamingStore)"""
        if last is not None:
            self._q.put((last, len(last), None))
        self._q.put(None)
        self._thread.join()
        if self._error is not None:
            raise self._error


class _Handle:
    def __init__(self, store, win):
        self.store, self.win = store, win

    def ready(self, hi, event=None):
        self.store.ready(self.win, hi, event)


class WindowedClip:
    """A raw planar source over the budget, opened for the two windowed passes (SubtitleRemover._open_windowed)."""

    windowed = True

    def __init__(self, path, rf, wf, n, H, W, device):
        self.path, self.rf, self.wf, self.n, self.H, self.W, self.device = path, rf, wf, int(n), int(H), int(W), device
        self.frame_bytes = self.H * self.W * 3
        self.keep_bytes = rf["frame_bytes"] if wf.get("keep") else 0
        self.budget = budget_bytes()
        self.want_scene_cuts = False
        self.scene_cuts = None                    # 1-based frame numbers, set by pass A when want_scene_cuts
        # what ran, for SubtitleRemover.resident_windows: the windows of pass B, the most bytes the window buffers of a pass held, the
        # records pass A read (and in how many windows), the scene cuts pass A found (when asked)
        self.report = {"windows": [], "bytes_max": 0, "records_read_pass_a": 0, "pass_a_windows": 0, "scene_cuts": None}

    def __len__(self):
        return self.n

    def _buffers(self, count, frames, keep):
        import torch

        dev = torch.device(self.device)
        bufs = [torch.empty((frames, self.H, self.W, 3), dtype=torch.uint8, device=dev) for _ in range(count)]
        planes = [torch.empty((frames, self.rf["frame_bytes"]), dtype=torch.uint8, device=dev) for _ in range(count)] if keep else None
        self.report["bytes_max"] = max(self.report["bytes_max"], count * frames * (self.frame_bytes + (self.keep_bytes if keep else 0)))
        return bufs, planes

    # ---- pass A ------------------------------------------------------------------------------------------------------------------
    def plan_pass_a(self, parts):
        """parts: the detector's batches (1-based frame numbers, increasing) -> the units of pass A, each the 0-based numbers of the
        frames to read.  When the scene kernels want every frame: [0, n) cut by frame count alone -- a part that straddles a boundary
        (or a whole hole between A/B sections) is gathered across the windows in a side buffer of one batch (carry_bytes, taken off
        the budget).  Else only the sampled frames, whole parts per window."""
        sizes = [len(part) for part in parts]
        self.carry_bytes = 0
        if self.want_scene_cuts or pass_a_reads_all():
            self.carry_bytes = max(sizes, default=0) * self.frame_bytes
            windows = plan_windows(self.n, [], self.frame_bytes, self.budget - self.carry_bytes, max_frames=PASS_A_FRAMES)
            if windows is None:
                raise WindowsDoNotFit(f"a detector batch of {max(sizes, default=1)} frames")
            return [list(range(lo, hi)) for lo, hi in windows]
        starts = [0]
        for s in sizes:
            starts.append(starts[-1] + s)
        windows = plan_windows(starts[-1], list(zip(starts, starts[1:])), self.frame_bytes, self.budget, max_frames=PASS_A_FRAMES)
        if windows is None:
            raise WindowsDoNotFit(f"a detector batch of {max(sizes, default=1)} frames")
        flat = [no - 1 for part in parts for no in part]
        return [flat[lo:hi] for lo, hi in windows]

    def stream_pass_a(self, units):
        """yields (unit number, uint8 [count,H,W,3] BGR on the device: the unit's frames in order); the view is valid until the next one"""
        import torch

        from .video_io import open_video

        if not units:
            return
        self.report["pass_a_windows"] = len(units)
        bufs, _ = self._buffers(min(2, len(units)), max(len(u) for u in units), keep=False)
        self.report["bytes_max"] += getattr(self, "carry_bytes", 0)          # (pass A is the first to allocate)
        reader = open_video(self.path)
        loader = WindowLoader(reader, self.rf, self.H, self.W, self.device, units, bufs)
        try:
            for k in range(len(units)):
                b, count = loader.get()
                yield k, bufs[b][:count]
                torch.cuda.current_stream(bufs[b].device).synchronize()
                loader.release(b)
                if count < len(units[k]):
                    break
        finally:
            loader.close()
            reader.release()
            self.report["records_read_pass_a"] = loader.records_read

    # ---- pass B ------------------------------------------------------------------------------------------------------------------
    def plan_pass_b(self, jobs):
        """jobs: [(lo, hi, ...)] in frame order -> the windows, or WindowsDoNotFit"""
        windows = plan_windows(self.n, [(j[0], j[1]) for j in jobs], self.frame_bytes, self.budget, self.keep_bytes)
        if windows is None:
            raise WindowsDoNotFit(f"an inpainting batch of {max((j[1] - j[0] for j in jobs), default=1)} frames")
        return windows

    def run_pass_b(self, windows, writer, tick, work):
        """work(win): inpaint the window in place and hand its frames to store (win.store.ready(hi, event)) -- called window after
        window while the loader reads the next one and the store writes what is final"""
        import torch

        from .video_io import open_video

        self.report["windows"] = list(windows)
        if not windows:
            return
        keep = bool(self.wf.get("keep"))
        longest = max(hi - lo for lo, hi in windows)
        bufs, planes = self._buffers(min(2, len(windows)), longest, keep)
        reader = open_video(self.path)
        loader = WindowLoader(reader, self.rf, self.H, self.W, self.device, [list(range(lo, hi)) for lo, hi in windows], bufs, planes)
        store = WindowStore(writer, self.wf, self.H, self.W, self.device, longest, tick,
                            on_stored=lambda win: loader.release(win.buf), on_error=loader.fail)
        try:
            try:
                for lo, hi in windows:
                    b, count = loader.get()
                    win = Window(lo, bufs[b][:count], planes[b][:count] if planes is not None else None, self.rf, b)
                    win.store = store.handle(win)
                    work(win)
                    ev = torch.cuda.Event()
                    ev.record(torch.cuda.current_stream(bufs[b].device))
                    store.ready(win, len(win), ev)
                    if count < hi - lo:            # a short file: the clip ends with the frames read
                        break
            except BaseException:
                store.abort()
                raise
            store.finish()
        finally:
            loader.close()
            reader.release()
            torch.cuda.synchronize(bufs[0].device)
