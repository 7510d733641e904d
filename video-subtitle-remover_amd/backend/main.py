"""Command-line surface of the reference's backend/main.py for the accelerated path.

    python -m vsr_amd.backend.main -i IN -o OUT [-c YMIN YMAX XMIN XMAX]... [--inpaint-mode sttn-auto]

Same flags, enum names and call order as the reference (backend/main.py:473-488, tools/args_handler.py:6-30):
SubtitleRemover(path).sub_areas / .ab_sections / .video_out_path / .run() with the modes sttn-auto, sttn-det, lama,
propainter and opencv on the MI355X engines.  Frames are read and written through tools/video_io.py (raw containers, an ffmpeg pipe
when a binary exists; `-o OUT` is written or the run fails -- there is no silent in-memory sink for a file input); audio is
muxed with the reference's two ffmpeg commands when ffmpeg exists (main.py:418-460).  GUI transport and temp files stay
with the reference (surface only, not accelerated).
"""
import os
import sys
import time
from pathlib import Path

import numpy as np

from .config import config
from .inpaint.sttn_auto_inpaint import STTNAutoInpaint
from .tools import frame_walk
from .tools.args_handler import parse_args
from .tools.constant import InpaintMode
from .tools.inpaint_tools import create_mask, expand_frame_ranges
from .tools.subtitle_detect import SubtitleDetect
from .tools.video_io import IMAGE_EXTS, ArrayWriter, AsyncWriter, ffmpeg_path, open_video, open_writer, y4m_out_mode


class SubtitleRemover:
    def __init__(self, vd_path, gui_mode=False, device="cuda:0", model_path=None, video_writer=None):
        self.sub_areas = []                      # [(ymin, ymax, xmin, xmax)] (args_handler.py:19 order)
        self.gui_mode = gui_mode
        self.video_path = vd_path
        self.device = device
        self.ab_sections = None
        info = open_video(vd_path).info() if not isinstance(vd_path, (str, os.PathLike)) else None
        if info is None:
            src = open_video(vd_path)
            info = src.info()
            src.release()
        self.frame_count = info["len"]
        self.fps = info["fps"]
        self.frame_height, self.frame_width = info["H_ori"], info["W_ori"]
        self.mask_size = (self.frame_height, self.frame_width)
        self.is_path = isinstance(vd_path, (str, os.PathLike))
        self.is_picture = False
        # in-memory input: in-memory sink.  File input: the sink is opened on first use for `video_out_path` (the caller may
        # still change it, main.py:486) and streams -- the reference writes through FFmpegVideoWriter as it goes (main.py:66-69)
        self._video_writer = video_writer if video_writer is not None else (None if self.is_path else ArrayWriter())
        if self.is_path:
            self.vd_name = Path(vd_path).stem
            ext = os.path.splitext(str(vd_path))[1].lower()
            self.is_picture = ext in IMAGE_EXTS
            out_ext = ext if ext in (".y4m", ".npy") else ".mp4"
            self.video_out_path = os.path.abspath(os.path.join(os.path.dirname(vd_path), f"{self.vd_name}_no_sub{out_ext}"))
            if self.is_picture:                                          # main.py:73-77
                self.video_out_path = os.path.abspath(os.path.join(os.path.dirname(vd_path), "no_sub", f"{self.vd_name}{ext}"))
        else:
            self.vd_name, self.video_out_path = "clip", None
        self.passed_through_single_frames = 0
        self.model_path = model_path or os.environ.get(
            "STTN_AUTO_MODEL_PATH", os.path.join(os.path.dirname(__file__), "models", "sttn-auto", "infer_model.pth"))
        self.progress_total = 0
        self.isFinished = False
        self.phase_seconds = {}
        self.resident_windows = None             # what a windowed run did (tools/resident_windows.WindowedClip.report); None: no such run
        self.static_areas = []                   # [(ymin, ymax, xmin, xmax)] that --logo-scan found (tools/logo_scan.py); run() fills it
        self.unblend_plans = []                  # the areas --logo-unblend un-mixes (tools/unblend.Plan) and [(area, reason)] of those it
        self.unblend_refusals = []               # leaves to inpainting; run() fills both
        self._logo_scan = None                   # the scan with its sampled frames on the device, until the plans are made

    @property
    def video_writer(self):
        if self._video_writer is None:
            sink = open_writer(self.video_out_path, self.fps, (self.frame_width, self.frame_height), frames=self.frame_count,
                               like=self._y4m_like())
            self._video_writer = AsyncWriter(sink)
        return self._video_writer

    def _y4m_like(self):
        """VSR_Y4M_OUT=source (--y4m-out source): a *.y4m sink takes the format of the *.y4m source and keeps the samples the run did not
        change (tools/video_io.py Y4mWriter like=...); the one place that turns the switch into a writer argument.  None: today's sink."""
        out = self.video_out_path
        if y4m_out_mode() != "source" or out is None or os.path.splitext(os.fspath(out))[1].lower() != ".y4m":
            return None
        if not self.is_path or os.path.splitext(os.fspath(self.video_path))[1].lower() != ".y4m":
            raise RuntimeError(f"VSR_Y4M_OUT=source needs a *.y4m input to take the format from; the input is {self.video_path!r}")
        return os.fspath(self.video_path)

    @video_writer.setter
    def video_writer(self, w):
        self._video_writer = w

    # hooks the plugin calls on its host object (main.py:109-151)
    def update_progress(self, tbar, increment):
        if tbar is not None:
            tbar.update(increment)

    def update_preview_with_comp(self, original, frame):
        pass

    def append_output(self, *args):
        print(*args)

    def sttn_auto_mode(self, tbar):
        """backend/main.py:247-258."""
        mask_area_coordinates = []
        for ymin, ymax, xmin, xmax in self.sub_areas:
            mask_area_coordinates.append((xmin, xmax, ymin, ymax))       # tuple order flips here (main.py:253-255)
        mask = create_mask(self.mask_size, mask_area_coordinates)
        sttn_video_inpaint = STTNAutoInpaint(self.device, self.model_path, self.video_path)
        sttn_video_inpaint(input_mask=mask, input_sub_remover=self, tbar=tbar)
        if sttn_video_inpaint.last_error is not None:
            # the plugin prints and returns like the reference's (sttn_auto_inpaint.py:329-331); the run must not report success
            # over a file that was not (completely) written
            raise sttn_video_inpaint.last_error

    is_current_frame_no_start = staticmethod(frame_walk.is_current_frame_no_start)     # main.py:90-97
    find_frame_no_end = staticmethod(frame_walk.find_frame_no_end)                     # main.py:100-107

    def _device_index(self):
        dev = self.device
        return int(dev.split(":")[1]) if isinstance(dev, str) and ":" in dev else 0

    def _distributed_rank(self):
        d = self._distributed()
        return d.get_rank() if d is not None else 0

    @staticmethod
    def _distributed():
        import torch.distributed as dist

        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            return dist
        return None

    def _run_items(self, tbar, items, process):
        """Drive the (pass-through frame | batch + mask) items of one video: on one GPU in order, on several dealt
        round-robin by tools/batch_parallel.py (rank 0 reads, detects and writes; peers only run `process`)."""
        from .tools.batch_parallel import run_batch_parallel

        def write(frame):
            self.video_writer.write(frame)
            self.update_progress(tbar, increment=1)

        run_batch_parallel(items, process, write, dist=self._distributed(), device=self.device if self._distributed() else "cpu")

    def _probe_resident(self, fits, then):
        """what _open_resident and _open_windowed ask first: one process, no GUI, a file with a raw planar source and sink (the sink is
        opened here, by the first self.video_writer access), and whether the clip fits VSR_RESIDENT_GB.  When that answer is `fits`
        -> then(reader, source format, writer format, info), with the reader still open; else None."""
        from .tools.resident import ResidentClip

        if self._distributed() is not None or getattr(self, "gui_mode", False) or not self.is_path:
            return None
        reader = open_video(self.video_path)
        try:
            fmts = ResidentClip.formats(reader, self.video_writer)
            info = reader.info()
            if fmts is None or fits != ResidentClip.fits(info["len"], info["H_ori"], info["W_ori"], fmts[0]["frame_bytes"] if fmts[1].get("keep") else 0):
                return None
            return then(reader, fmts[0], fmts[1], info)
        finally:
            reader.release()

    def _open_resident(self):
        """(ResidentClip, writer planes format) when this run can keep the decoded video in HBM (tools/resident.py: raw planar source
        and sink, one process, the clip fits), else None: the host-frame loop then runs as before."""
        from .tools.resident import ResidentClip

        def load(reader, fmt, wf, info):
            t0 = time.time()
            clip = ResidentClip.load(reader, fmt, info["len"], info["H_ori"], info["W_ori"], self.device, keep_planes=bool(wf.get("keep")))
            self.phase_seconds["read + upload + YUV->BGR"] = time.time() - t0
            return clip, wf

        return self._probe_resident(True, load)

    def _open_windowed(self):
        """tools/resident_windows.WindowedClip when VSR_IO_RESIDENT=windows (--resident-windows) and this run could keep its video in HBM
        but for the size of the clip; None otherwise (and for a clip that fits: _open_resident took it)"""
        from .tools import resident_windows

        def windowed(reader, fmt, wf, info):
            # (the frames a resident clip would hold after loading: a last record cut short is not one of them)
            n = reader.whole_records() if hasattr(reader, "whole_records") else info["len"]
            return resident_windows.WindowedClip(self.video_path, fmt, wf, n, info["H_ori"], info["W_ori"], self.device)

        return self._probe_resident(False, windowed) if resident_windows.enabled() else None

    def _windows_do_not_fit(self, why):
        self.append_output(f"resident windows: {why} does not fit half of VSR_RESIDENT_GB; taking the host-frame loop")

    def _run_windowed(self, wclip, jobs, plugin, tbar, singles=(), single_frame_inpaint=None):
        """pass B of a windowed run (tools/resident_windows.py): jobs [(lo, hi, mask)] and singles [(frame, mask)] index the file; every
        window is inpainted in place like a resident clip and stored as its frames become final.  False: a batch does not fit, nothing
        was written -- the caller takes the host-frame loop."""
        import torch

        from .tools.resident_windows import WindowsDoNotFit

        try:
            windows = wclip.plan_pass_b(jobs)
        except WindowsDoNotFit as e:
            self._windows_do_not_fit(e)
            self.resident_windows = None           # (pass A ran in windows; the run as a whole does not)
            return False

        def work(win):
            lo, hi = win.lo, win.lo + len(win)
            for at, mask in singles:                                                   # main.py:217-224: LamaInpaint.inpaint on the whole frame
                if lo <= at < hi:
                    one = single_frame_inpaint(win.frames[at - lo].cpu().numpy(), mask)
                    win.frames[at - lo].copy_(torch.from_numpy(np.ascontiguousarray(one)))
            mine = [(win.frames[max(a, lo) - lo:min(b, hi) - lo], mask) for a, b, mask in jobs if a < hi and b > lo]
            self._run_resident_jobs(mine, plugin, win, win.store)

        t0 = time.time()
        wclip.run_pass_b(windows, self.video_writer, lambda: self.update_progress(tbar, increment=1), work)
        self.phase_seconds["windows, pass B: read + upload + YUV->BGR, inpainting, BGR->YUV + download + write"] = time.time() - t0
        return True

    def _run_resident_jobs(self, jobs, plugin, clip, store=None, look=None):
        """the independent batches of a resident run: one after the other, or over VSR_BATCH_LANES plugin instances (tools/batch_lanes.py).
        store: a tools/resident.StreamingStore -- with one lane the frames in front of the next batch are handed to it as each batch
        is enqueued (behind an event on the compute stream), so that they are converted, downloaded and written under the batches
        that follow; jobs are slices of clip.frames in frame order.
        look: a tools/det_lookback.ResidentLookback over the same jobs -- batch j then runs as look.call(plugin, j), which copies the
        source rows later batches look back at aside first (the copies are its own: nothing of them reaches the store)."""
        import torch

        from .tools import batch_lanes

        if not hasattr(self, "_lane_cache"):
            self._lane_cache = {}
        plugins = batch_lanes.lane_plugins(plugin, batch_lanes.lanes_from_env(), self._lane_cache)
        if store is None or len(plugins) > 1 or os.environ.get("VSR_STREAM_STORE", "1") == "0":      # (0: everything is written after the last batch)
            if look is not None:
                batch_lanes.run_map(list(range(len(jobs))), plugins, look.call, clip.frames.device)
            else:
                batch_lanes.run_jobs(jobs, plugins, clip.frames.device)
            return
        dev = clip.frames.device
        frame_elems = clip.frames[0].numel()
        first = [(job[0].data_ptr() - clip.frames.data_ptr()) // frame_elems for job in jobs]     # first frame of every batch
        store.ready(first[0] if jobs else len(clip))
        for j, job in enumerate(jobs):
            if look is not None:
                look.call(plugin, j)
            else:
                plugin(*job)
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(dev))
            store.ready(first[j + 1] if j + 1 < len(jobs) else len(clip), ev)

    def _run_resident(self, resident, tbar, plugin, make_jobs, look=None):
        """the tail of a resident run.  resident: what _open_resident gave; make_jobs(n) -> [(lo, hi, mask)] over the clip's n frames
        (run inside the "inpainting" phase: propainter's single frames are inpainted on the way): a batch is a slice of the clip,
        inpainted in place; look(frames): the tools/det_lookback.ResidentLookback of the jobs just made, if any.  The store
        converts, downloads and writes under the batches (_run_resident_jobs) and is aborted when one fails."""
        from .tools.resident import StreamingStore

        clip, wf = resident

        def inpaint_all():
            jobs = [(clip.frames[lo:hi], mask) for lo, hi, mask in make_jobs(len(clip))]
            self._run_resident_jobs(jobs, plugin, clip, store, look(clip.frames) if look is not None else None)

        store = StreamingStore(clip, self.video_writer, wf, lambda: self.update_progress(tbar, increment=1))
        try:
            self._timed("inpainting", inpaint_all)
        except BaseException:
            store.abort()
            raise
        self._timed("BGR->YUV + download + write (what is left after the last batch)", store.finish)

    def _single_passes_through(self):
        """propainter_mode without a single-frame plugin: an isolated subtitle frame is written as it is, counted, and warned of once"""
        self.passed_through_single_frames += 1
        if self.passed_through_single_frames == 1:
            self.append_output("warning: no LaMa weights configured (LAMA_MODEL_PATH): isolated subtitle frames pass through")

    def _find_subtitles(self, detector, clip, wclip):
        """the detector pass -> (sub_list, wclip): over the resident clip, over the file in windows (pass A; a detector batch that does
        not fit sends the run to the host-frame loop: wclip comes back None), or over host frames"""
        if wclip is not None:
            from .tools.resident_windows import WindowsDoNotFit

            name = "windows, pass A: read + upload + YUV->BGR, detector pass" + (", scene cuts" if wclip.want_scene_cuts else "")
            try:
                sub_list = self._timed(name, detector.find_subtitle_frame_no, sub_remover=self, clip=wclip)
                self.resident_windows = wclip.report
                return sub_list, wclip
            except WindowsDoNotFit as e:
                self._windows_do_not_fit(e)
        return self._timed("detector pass", detector.find_subtitle_frame_no, sub_remover=self, **self._clip_kw(clip)), None

    def _with_static_areas(self, sub_list):
        """the detector pass's {frame_no: [boxes]} with every area of --logo-scan (self.static_areas) in every frame's list, as
        (xmin, xmax, ymin, ymax) for the frames 1 .. frame_count; without such areas (the option off) the dictionary as it came"""
        if not self.static_areas:
            return sub_list
        if self._logo_scan is not None:
            # --logo-unblend: the plans, from the areas that meet no box of the text detector in any frame
            self._make_unblend_plans({(ymin, ymax, xmin, xmax) for have in sub_list.values() for xmin, xmax, ymin, ymax in have})
        boxes = [(xmin, xmax, ymin, ymax) for ymin, ymax, xmin, xmax in self.static_areas]
        out = {}
        for no in range(1, self.frame_count + 1):
            have = list(sub_list.get(no, []))
            out[no] = have + [b for b in boxes if b not in have]
        return out

    def _make_unblend_plans(self, text_boxes):
        """--logo-unblend (tools/unblend.py): the plans of the areas the scan found, registered for the plugin calls of this run; an
        area that meets one of `text_boxes` (ymin, ymax, xmin, xmax), or that cannot be un-mixed, is reported and inpainted as without
        the option.  The scan's sampled frames leave the device here."""
        from .tools import unblend

        scan, self._logo_scan = self._logo_scan, None
        self.unblend_plans, self.unblend_refusals = self._timed("logo unblend plans", unblend.make_plans, scan, self.static_areas,
                                                                sorted(text_boxes))
        unblend.register(self.unblend_plans)
        for plan in self.unblend_plans:
            self.append_output(f"logo unblend: area {plan.box} is un-mixed (gain {plan.level}/256)")
        for area, reason in self.unblend_refusals:
            self.append_output(f"logo unblend: area {area} stays inpainted ({reason})")

    @staticmethod
    def _clip_kw(clip):
        """the HBM-resident clip is handed on only when there is one: without it the calls keep the reference's signatures"""
        return {} if clip is None else {"clip": clip}

    def _timed(self, name, fn, *a, **kw):
        """phase timer of run(): detector pass / scene cuts / inpainting / writing, reported by main() and scripts/bench_e2e.py"""
        import torch

        t0 = time.time()
        r = fn(*a, **kw)
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        self.phase_seconds[name] = self.phase_seconds.get(name, 0.0) + time.time() - t0
        return r

    def propainter_mode(self, tbar, propainter_inpaint=None, text_detector=None, scene_div_points=None, single_frame_inpaint=None):
        """backend/main.py:159-245.  Intervals of frames with the same mask, cut at scene changes, are read whole and
        handed to the plugin in batch_generator batches of propainterMaxLoadNum.  The scene-change frame numbers come
        from tools/scene_detect.py (reference: scenedetect's ContentDetector, subtitle_detect.py:158-170) unless given; the
        detector is injected; isolated single frames go to LaMa as in the reference (main.py:217-224,231-237) when its weights
        are configured (`lama_inpaint`), otherwise they pass through and are counted in `passed_through_single_frames`."""
        if propainter_inpaint is None:
            from .inpaint.propainter_inpaint import PropainterInpaint

            model_dir = os.environ.get("PROPAINTER_MODEL_DIR", os.path.join(os.path.dirname(__file__), "models", "propainter"))
            propainter_inpaint = PropainterInpaint(self.device, model_dir, config.propainterMaxLoadNum.value)
        dist = self._distributed()
        from .tools import seam_feather

        seam_feather.refuse_ranks_all(dist)          # --seam-feather, --regrain, --deflicker, --tone-match, --glyph-key: bad values and several ranks, before any frame is read
        if dist is not None and dist.get_rank() != 0:
            return self._run_items(tbar, (), propainter_inpaint)
        if single_frame_inpaint is None:
            lama = self.lama_inpaint
            single_frame_inpaint = lama.inpaint if lama is not None else None
        detector = SubtitleDetect(self.video_path, self.sub_areas, text_detector=text_detector)
        # one detector lane here unless VSR_DET_LANES says otherwise: with two, the detector pass of config 4 gains 0.45 s and the
        # propainter inpainting that follows loses 2-4 s (62.9-63.1 -> 65.0-67.5 s, same box, profiles/r04_pp_e2e_ab.log; the
        # sttn-det inpainting does not care) -- the second instance's streams stay alive beside the plugin's
        detector.det_lanes_default = 1
        # the clip stays in HBM only for a plugin that takes device tensors (an injected callable, or the cv2 plugin, gets host frames)
        on_device = getattr(propainter_inpaint, "accepts_device_frames", False)
        resident = self._open_resident() if on_device else None
        clip = resident[0] if resident is not None else None
        wclip = self._open_windowed() if on_device and resident is None else None
        if wclip is not None:
            wclip.want_scene_cuts = scene_div_points is None       # pass A is the one walk over every frame: the scene kernels ride along
        sub_list, wclip = self._find_subtitles(detector, clip, wclip)
        sub_list = self._with_static_areas(sub_list)     # --logo-scan: a static overlay is in every frame's list
        if len(sub_list) == 0:
            self._run_items(tbar, (), propainter_inpaint)                  # releases the peers before failing
            raise Exception(f"No subtitle detected in {self.video_path}")
        ranges = detector.find_continuous_ranges_with_same_mask(sub_list)
        if scene_div_points is None:                 # main.py:165: self.sub_detector.get_scene_div_frame_no(self.video_path)
            scene_div_points = self._timed("scene cuts", detector.get_scene_div_frame_no, self.video_path, device=self._device_index(),
                                           **self._clip_kw(clip if wclip is None else wclip))
        ranges = detector.split_range_by_scene(ranges, list(scene_div_points))

        def walk(read):
            """the one walk of this mode (tools/frame_walk.py), over the reader's frames or over frame numbers"""
            return frame_walk.propainter_walk(read, sub_list, ranges, lambda start: create_mask(self.mask_size, sub_list[start]),
                                              config.propainterMaxLoadNum.value)

        def clip_jobs(n, single):
            """-> [(lo, hi, mask)], 0-based: the batches of a clip of n frames; single(frame, mask): an interval of one frame that LaMa takes"""
            return frame_walk.clip_jobs(walk(frame_walk.counted(n)), single if single_frame_inpaint is not None else None,
                                        self._single_passes_through)

        if wclip is not None:
            # over the budget: the same batches, on windows of the file that follow each other through HBM (tools/resident_windows.py)
            singles = []
            jobs = clip_jobs(wclip.n, lambda at, mask: singles.append((at, mask)))
            if self._run_windowed(wclip, jobs, propainter_inpaint, tbar, singles, single_frame_inpaint):
                return
            self.passed_through_single_frames = 0                  # (the host-frame loop below counts them again)
        if resident is not None:
            import torch

            def single(at, mask):                  # main.py:217-224: LamaInpaint.inpaint on the whole frame
                one = single_frame_inpaint(clip.frames[at].cpu().numpy(), mask)
                clip.frames[at].copy_(torch.from_numpy(np.ascontiguousarray(one)))

            return self._run_resident(resident, tbar, propainter_inpaint, lambda n: clip_jobs(n, single))
        reader = open_video(self.video_path)
        try:
            self._run_items(tbar, frame_walk.host_items(walk(reader.read), single_frame_inpaint, self._single_passes_through), propainter_inpaint)
        finally:
            reader.release()

    def video_inpaint(self, tbar, model, text_detector=None):
        """backend/main.py:260-333 -- detector pass, interval construction, then `model(batch, mask)` per batch.
        Frame numbers are 1-based here exactly as in the reference.

        Two options that are not the reference's, both off by default (then every job, every plugin call and every byte are what
        they were) and read only for a plugin that takes context frames (sttn-det; lama and opencv ignore them): --scene-split cuts
        every interval at the scene starts, --sttn-context N lets every batch look back at the N source frames in front of it inside
        its piece, --sttn-lookahead M at the M source frames behind it inside its piece (tools/det_lookback.py holds the definition).
        One process, no resident windows."""
        from .tools import det_lookback

        from .tools import seam_feather

        seam_feather.refuse_ranks_all(self._distributed())   # --seam-feather, --regrain, --deflicker, --tone-match, --glyph-key: bad values and several ranks, before any frame is read
        max_load = config.getSttnMaxLoadNum()
        n_context, scene_split, n_ahead = (0, False, 0)
        if getattr(model, "accepts_context", False):
            n_context, scene_split, n_ahead = det_lookback.lookback_options(max_load, lookahead=None)   # bad values: before any frame is read
        lookback = bool(n_context or scene_split or n_ahead)
        dist = self._distributed()
        if lookback and dist is not None:
            raise RuntimeError("sttn-det context frames (--sttn-context, --sttn-lookahead) / scene-bounded intervals run in one process: a batch "
                               "looks back at its predecessor's frames and ahead at its successor's, "
                               f"which another rank holds (world size {dist.get_world_size()}); run without them or on one GPU")
        if dist is not None and dist.get_rank() != 0:
            return self._run_items(tbar, (), model)
        on_device = getattr(model, "accepts_device_frames", False)
        wclip = self._open_windowed() if lookback and on_device else None      # (the header only: no frame is read)
        if wclip is not None:
            raise RuntimeError("sttn-det context frames (--sttn-context, --sttn-lookahead) / scene-bounded intervals do not run in resident windows "
                               "(--resident-windows on a clip over VSR_RESIDENT_GB): a batch looks back and ahead across window boundaries; run without them, without "
                               "--resident-windows, or with a larger VSR_RESIDENT_GB")
        detector = SubtitleDetect(self.video_path, self.sub_areas, text_detector=text_detector)
        resident = self._open_resident() if on_device else None
        if not lookback:                                           # (with an option on, the answer is in: not a windowed run)
            wclip = self._open_windowed() if on_device and resident is None else None
        sub_list, wclip = self._find_subtitles(detector, resident[0] if resident is not None else None, wclip)
        sub_list = self._with_static_areas(sub_list)     # --logo-scan: a static overlay is in every frame's list
        static = [(xmin, xmax, ymin, ymax) for ymin, ymax, xmin, xmax in self.static_areas]
        if len(sub_list) == 0:
            self._run_items(tbar, (), model)
            raise Exception(f"No subtitle detected in {self.video_path}")
        ranges = detector.find_continuous_ranges_with_same_mask(sub_list)
        ranges = expand_frame_ranges(ranges, config.subtitleTimelineBackwardFrameCount.value,
                                     config.subtitleTimelineForwardFrameCount.value)
        ranges = detector.filter_and_merge_intervals(ranges, config.sttnReferenceLength.value)
        start_end = {s: min(e, self.frame_count) for s, e in ranges}
        cuts = []
        if scene_split:
            # one scene pass (the call propainter_mode makes: the cuts pinned to the reference's SceneManager), over the resident clip
            # when there is one; its numbers are 1-based
            points = self._timed("scene cuts", detector.get_scene_div_frame_no, self.video_path, device=self._device_index(),
                                 **self._clip_kw(resident[0] if resident is not None else None))
            cuts = [int(p) - 1 for p in points]
        self.scene_cuts = cuts

        def interval_mask(first, last):
            coords = []
            for no in range(first, last):                          # NB: the reference's range excludes `last` (:310)
                for area in sub_list.get(no, []):
                    xmin, xmax, ymin, ymax = area
                    if (ymax - ymin) - (xmax - xmin) > config.subtitleYXAxisDifferencePixel.value and area not in static:
                        continue                                   # taller than wide: treated as a false detection (of text: a static area stays)
                    if area not in coords:
                        coords.append(area)
            return create_mask(self.mask_size, coords)

        det = []

        def clip_jobs(n):
            """the batches of a clip of n frames -> [(lo, hi, mask)], 0-based: tools/det_lookback.det_jobs, the one walk over frame numbers
            (options off: no cuts, no context -- the batches this mode has always made); `det` keeps its jobs for ResidentLookback"""
            det[:] = det_lookback.det_jobs(start_end, n, interval_mask, cuts, n_context, max_load, n_ahead if n_ahead else None)
            return [(job[0], job[1], job[3]) for job in det]

        if wclip is not None:
            # over the budget: the same batches, on windows of the file that follow each other through HBM (tools/resident_windows.py)
            if self._run_windowed(wclip, clip_jobs(wclip.n), model, tbar):
                return
        if resident is not None:
            # (the source rows a later batch looks back at are copied aside before their batch is inpainted: ResidentLookback)
            # (... and the rows a batch looks ahead at, by that batch, before their owners are)
            return self._run_resident(resident, tbar, model, clip_jobs,
                                      (lambda frames: det_lookback.ResidentLookback(frames, det)) if (n_context or n_ahead) else None)
        reader = open_video(self.video_path)
        process = model
        if n_context or n_ahead:
            # host frames: a batch's context goes along with its work item, in front of the batch's frames and behind them (they are still
            # the source's here: an interval is read whole before its batches are made); how many of an item's leading and trailing frames
            # are context waits in a queue that items() fills and the plugin call empties, both in
            # item order (one process: tools/batch_parallel.py hands the items to `process` one by one, as they come)
            import collections

            n_ctx_of = collections.deque()

            def process(frames, mask):
                k, ka = n_ctx_of.popleft()
                if not ka:
                    return model(frames[k:], mask, context=frames[:k])
                return model(frames[k:len(frames) - ka], mask, context=frames[:k], lookahead=frames[len(frames) - ka:])

        def items():
            idx = 0
            while True:
                ok, frame = reader.read()
                if not ok:
                    break
                idx += 1
                if idx not in start_end:
                    yield ("pass", frame)
                    continue
                first, last = idx, start_end[idx]
                frames = [frame]
                for _ in range(last - first):
                    ok, frame = reader.read()
                    if not ok:
                        break
                    idx += 1
                    frames.append(frame)
                mask = interval_mask(first, last)
                # (options off: no cuts, ctx_lo = lo, ahead_hi = hi -- batch_generator over the interval's frames)
                for lo, hi, ctx_lo, ahead_hi in det_lookback.piece_jobs(first - 1, first - 1 + len(frames), cuts, n_context, max_load, n_ahead):
                    if n_context or n_ahead:
                        n_ctx_of.append((lo - ctx_lo, ahead_hi - hi))
                    yield ("work", frames[ctx_lo - (first - 1):ahead_hi - (first - 1)], mask)

        try:
            self._timed("read + inpainting + write (host frames)", self._run_items, tbar, items(), process)
            if (n_context or n_ahead) and n_ctx_of:
                raise RuntimeError(f"sttn-det look-back: {len(n_ctx_of)} work items were made and never inpainted")
        finally:
            reader.release()

    @property
    def lama_inpaint(self):
        """main.py:462-466 (cached_property): LamaInpaint over $LAMA_MODEL_PATH or backend/models/big-lama/big-lama.pt; an injected
        object (attribute `_lama_inpaint`) wins; None when no weights can be found."""
        if getattr(self, "_lama_inpaint", None) is None:
            path = os.environ.get("LAMA_MODEL_PATH", os.path.join(os.path.dirname(__file__), "models", "big-lama", "big-lama.pt"))
            if not os.path.exists(path) and not os.path.isfile(os.path.join(os.path.dirname(path), "fs_manifest.csv")):
                return None                                  # neither the checkpoint nor its split parts
            from .inpaint.lama_inpaint import LamaInpaint

            self._lama_inpaint = LamaInpaint(self.device, path)
        return self._lama_inpaint

    @lama_inpaint.setter
    def lama_inpaint(self, plugin):
        self._lama_inpaint = plugin

    def picture_mode(self):
        """main.py:353-371: a single image -- detect, mask, LamaInpaint.inpaint on the whole frame, write."""
        src = open_video(self.video_path)
        ok, frame = src.read()
        src.release()
        if not ok:
            raise Exception(f"cannot read {self.video_path}")
        detector = SubtitleDetect(self.video_path, self.sub_areas, text_detector=self._default_detector())
        sub_list = detector.detect_subtitle(frame)
        if len(sub_list):
            lama = self.lama_inpaint
            if lama is None:
                raise Exception("inpaint mode: lama needs its weights (LAMA_MODEL_PATH)")
            frame = lama.inpaint(frame, create_mask(frame.shape[0:2], sub_list))
        self.video_writer.write(frame)

    def merge_audio_to_video(self):
        """main.py:418-460: copy the input's audio track into the written file; needs ffmpeg, skipped (with a note) without."""
        import shutil
        import subprocess
        import tempfile

        ff = ffmpeg_path()
        out = self.video_out_path
        if ff is None or not self.is_path or os.path.splitext(out)[1].lower() in (".y4m", ".npy"):
            return False
        silent = out + ".video_only" + os.path.splitext(out)[1]
        os.replace(out, silent)
        with tempfile.NamedTemporaryFile(suffix=".aac", delete=False) as tmp:
            audio = tmp.name
        try:
            subprocess.check_output([ff, "-y", "-i", str(self.video_path), "-acodec", "copy", "-vn", "-loglevel", "error", audio],
                                    stdin=subprocess.DEVNULL, timeout=600)
            subprocess.check_output([ff, "-y", "-i", silent, "-i", audio, "-vcodec", "copy", "-acodec", "copy", "-loglevel", "error", out],
                                    stdin=subprocess.DEVNULL, timeout=600)
            os.remove(silent)
            return True
        except Exception as e:
            self.append_output(f"audio not merged ({e}); keeping the silent video")
            shutil.move(silent, out)
            return False
        finally:
            if os.path.exists(audio):
                os.remove(audio)

    def _default_detector(self):
        """the injected detector if any, else the MI355X TextDetection configured through the environment (tools/ocr_det.py)"""
        det = getattr(self, "text_detector", None)
        if det is None:
            from .tools import stroke_det

            if stroke_det.detect_option() == "strokes":                  # --text-detect strokes: no weights (tools/stroke_det.py)
                if getattr(self, "_stroke_detector", None) is None:
                    self._stroke_detector = stroke_det.StrokeTextDetection(self._device_index())
                return self._stroke_detector
            from .tools import ocr_det

            det = ocr_det.from_env(self._device_index())
        return det

    def run(self):
        from .tools import seam_feather

        start_time = time.time()
        seam_feather.refuse_ranks_all(self._distributed())   # --seam-feather, --regrain, --deflicker, --tone-match, --glyph-key: a bad value or several ranks fail before any work is done
        from .tools import logo_scan

        scan = logo_scan.refuse_ranks(self._distributed())   # --logo-scan: a bad value or several ranks, likewise
        from .tools import unblend

        unmix = unblend.refuse()                             # --logo-unblend: a bad value, or on without --logo-scan, likewise
        from .tools import stroke_det

        if stroke_det.detect_option() == "strokes":          # --text-detect: a bad value; strokes in a mode without a detector, beside an injected one, or on several ranks, likewise
            stroke_det.refuse(self._distributed(), self.is_picture or config.inpaintMode.value != InpaintMode.STTN_AUTO,
                              getattr(self, "text_detector", None))
        try:
            self._run(scan, unmix, start_time)
        finally:
            if unmix:
                unblend.clear()
                self._logo_scan = None

    def _run(self, scan, unmix, start_time):
        """run() behind its refusals"""
        from .tools import logo_scan

        if self._video_writer is None and self.is_path:
            self._y4m_like()                                             # a sink that cannot be made fails before any work is done
        mode = config.inpaintMode.value
        if scan:
            # one pass over the clip before the sink is made: a scan that must fail (a picture, a clip of fewer than 16 frames) leaves no file
            if unmix:
                # (--logo-unblend: the sampled frames stay on the device until the plans are made)
                self._logo_scan = self._timed("logo scan", logo_scan.run_scan, self.video_path, device=self._device_index(),
                                              report=self.append_output, keep=True)
                self.static_areas = self._logo_scan.found
                if not self.static_areas:
                    self._logo_scan = None                               # nothing to un-mix: the frames leave the device now
            else:
                self.static_areas = self._timed("logo scan", logo_scan.find_areas, self.video_path, device=self._device_index(),
                                                report=self.append_output)
            self.append_output(f"logo scan: {len(self.static_areas)} static area{'s' if len(self.static_areas) != 1 else ''} "
                               f"(ymin, ymax, xmin, xmax): {self.static_areas}")
            if mode == InpaintMode.STTN_AUTO:
                # the areas join the boxes of -c; without -c they are the mask, in place of the whole frame
                if len(self.sub_areas) == 0 and len(self.static_areas) == 0:
                    raise Exception(f"No static overlay found in {self.video_path} and no subtitle area given (-c)")
                boxed = list(self.sub_areas)
                self.sub_areas.extend(a for a in self.static_areas if a not in self.sub_areas)
                if unmix:
                    self._make_unblend_plans(boxed)                      # an area that meets a box of -c stays inpainted
        if len(self.sub_areas) == 0:
            self.sub_areas.append((0, self.frame_height, 0, self.frame_width))
        if self.is_picture:
            self.picture_mode()
        elif mode == InpaintMode.STTN_AUTO:
            self.sttn_auto_mode(None)
        elif mode == InpaintMode.STTN_DET:
            from .inpaint.sttn_det_inpaint import STTNDetInpaint

            det_path = os.environ.get("STTN_DET_MODEL_PATH", os.path.join(os.path.dirname(__file__), "models", "sttn-det", "sttn.pth"))
            self.video_inpaint(None, STTNDetInpaint(self.device, det_path), text_detector=self._default_detector())
        elif mode == InpaintMode.LAMA:
            lama = self.lama_inpaint
            if lama is None:
                raise Exception("inpaint mode: lama needs its weights (LAMA_MODEL_PATH or backend/models/big-lama/big-lama.pt)")
            self.video_inpaint(None, lama, text_detector=self._default_detector())
        elif mode == InpaintMode.PROPAINTER:
            self.propainter_mode(None, propainter_inpaint=getattr(self, "propainter_inpaint", None),
                                 text_detector=self._default_detector(), scene_div_points=getattr(self, "scene_div_points", None))
        elif mode == InpaintMode.OPENCV:
            # main.py:383-384: cv2.inpaint (Telea, radius 3), restated as a level replay on the GPU (inpaint/opencv_inpaint.py)
            from .inpaint.opencv_inpaint import OpenCVInpaint

            plugin = getattr(self, "opencv_inpaint", None) or OpenCVInpaint(self.device)
            self.video_inpaint(None, plugin, text_detector=self._default_detector())
        else:
            raise Exception(f"inpaint mode: {mode} not implemented")     # main.py:386
        if self._video_writer is not None:
            self._video_writer.release()                                 # main.py:389
            if self.is_path and self._distributed_rank() == 0:
                self.merge_audio_to_video()
        self.isFinished = True
        self.progress_total = 100
        self.append_output(f"Finished in {round(time.time() - start_time)} s")


# command-line flags that reach the run through the environment: (attribute of the parsed arguments, variable, value -> string)
FLAG_ENV = (("y4m_out", "VSR_Y4M_OUT", str), ("resident_windows", "VSR_IO_RESIDENT", lambda _: "windows"),
            ("scene_split", "VSR_SCENE_SPLIT", lambda _: "1"), ("sttn_context", "VSR_STTN_CONTEXT", str),
            ("sttn_lookahead", "VSR_STTN_LOOKAHEAD", str), ("seam_feather", "VSR_SEAM_FEATHER", str), ("regrain", "VSR_REGRAIN", str),
            ("deflicker", "VSR_DEFLICKER", str), ("tone_match", "VSR_TONE_MATCH", str),
            ("glyph_key", "VSR_GLYPH_KEY", str), ("glyph_hold", "VSR_GLYPH_HOLD", str), ("borrow", "VSR_BORROW", str),
            ("borrow_pan", "VSR_BORROW_PAN", str), ("opencv_fill", "VSR_OPENCV_FILL", str),
            ("logo_scan", "VSR_LOGO_SCAN", lambda _: "1"), ("logo_unblend", "VSR_LOGO_UNBLEND", lambda _: "1"),
            ("text_detect", "VSR_TEXT_DETECT", str))


def main(argv=None):
    args = parse_args(argv)
    config.inpaintMode.value = args.inpaint_mode
    for attribute, variable, convert in FLAG_ENV:
        value = getattr(args, attribute)
        if value is not None and value is not False:
            os.environ[variable] = convert(value)
    sr = SubtitleRemover(args.input)
    sr.sub_areas = [tuple(c) for c in args.subtitle_area_coords]
    if args.output is not None:
        sr.video_out_path = os.path.abspath(args.output)
    sr.run()
    sr.append_output(f"written: {sr.video_out_path}")


if __name__ == "__main__":
    main(sys.argv[1:])
