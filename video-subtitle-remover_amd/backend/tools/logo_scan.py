"""--logo-scan: find the static overlays of a clip -- a station logo, a channel bug, a burnt-in watermark -- on the GPU, so that every mode
inpaints them on every frame (not in the reference, which removes a watermark only inside a box drawn by hand with -c; opt-in, DESIGN
4.17; the numpy statement is tests/_static_statement.py).

An overlay is an edge pattern that stays put while the picture around it moves.  Of an N-frame clip (N >= 16) M = min(N, 120) frames are
sampled, i_k = (k N) // M.  Per sampled frame Y = (29 B + 150 G + 77 R + 128) >> 8 and the gradient
g = |Y[y, x + 1] - Y[y, x - 1]| + |Y[y + 1, x] - Y[y - 1, x]| (indices clamped to the frame); per pixel over the samples lo = min Y,
hi = max Y and e = the number of samples with g >= GE.  A pixel is a seed when e >= M - M // 8 and moving when hi - lo >= MV.  The seeds
are dilated by D pixels; an 8-connected component of that map is kept when its area is at least MIN_AREA, its box is at most a third of
the frame in either direction and at least half the pixels of its ring (the box grown by RING, less the box) are moving.  The result is
the kept boxes grown by PAD as (ymin, ymax, xmin, xmax), the convention of -c, at most MAX_AREAS of them, the largest first.

What it cannot tell: a static shot (nothing moves around the overlay, so nothing is kept) and an overlay larger than a third of the
frame (a letterbox, the set of a studio: not told apart from the picture).

    1. vsr_static_accum: one launch over the sampled frames where they are (a resident clip), or one per uploaded batch of a reading
       pass of its own (host frames, a windowed clip), continued with first = 0; three state planes, 4 bytes a pixel,
    2. vsr_static_classify: the dilated seed map and the moving plane,
    3. vsr_det_launch_ccl: the components of the seed map (the text detector's labeller), then one read-back of the component list and
       the moving plane; the choice among the components is host arithmetic on a handful of boxes.

Off (the default): nothing here is called but scan_option, no launch, no byte written that was not before.  The option is read here
and nowhere else (scan_option: --logo-scan sets VSR_LOGO_SCAN=1).  Several ranks are refused (refuse_ranks) before any work, as
--regrain refuses them.

--logo-unblend (tools/unblend.py) estimates its planes from the same sampled frames: run_scan(keep=True) returns the Scan with
them still on the device (Scan.pieces), find_areas is run_scan without keeping.
"""
import ctypes as C
import os

import numpy as np

ENV = "VSR_LOGO_SCAN"
GE, MV, D = 24, 48, 6                       # gradient of an edge, luma range of a moving pixel, dilation of the seeds
MAX_SAMPLES, MIN_FRAMES = 120, 16
MIN_AREA, RING, PAD, MAX_AREAS = 400, 24, 4, 8
BATCH_FRAMES = 16                           # sampled frames per upload of the reading pass
COMPONENT_CAP = 4096                        # components read back at first; a map with more is labelled again with room for all

stats = {"scans": 0, "frames": 0, "accum_launches": 0, "components": 0, "areas": 0, "dropped": 0}


def scan_option(value=None, env=None):
    """whether this run scans: `value`, None = the environment (VSR_LOGO_SCAN, unset, empty or 0 = off, 1 = on).  The one reading of
    the option.  ValueError for anything else."""
    env = os.environ if env is None else env
    if value is None:
        value = env.get(ENV, "0") or "0"
    if isinstance(value, bool):
        return value
    if str(value).strip() in ("0", "1"):
        return str(value).strip() == "1"
    raise ValueError(f"logo scan: {value!r} is neither 0 nor 1")


def refuse_ranks(dist, scan=None):
    """-> whether this run scans.  With the scan on, more than one rank raises before any work: the scan and the masks made from it
    live on the rank that reads the clip, and the peers' loops have not been taught the option (the precedent of --regrain)."""
    on = scan_option(scan)
    if on and dist is not None and dist.get_world_size() > 1:
        raise RuntimeError(f"--logo-scan / {ENV} = 1 runs in one process (world size {dist.get_world_size()}): "
                           "run without it or on one GPU")
    return on


def sample_indices(N):
    """the numbers of the M = min(N, 120) sampled frames of an N-frame clip: distinct and increasing"""
    N = int(N)
    if N < MIN_FRAMES:
        raise ValueError(f"logo scan: {N} frame{'s' if N != 1 else ''} in the input, a scan needs at least {MIN_FRAMES} "
                         "(a picture has no overlay that stays while the rest moves)")
    M = min(N, MAX_SAMPLES)
    return [(k * N) // M for k in range(M)]


def select_areas(comps, moving):
    """the choice among the components -> (areas [(ymin, ymax, xmin, xmax)], components dropped over MAX_AREAS).  comps: rows
    (label, area, xmin, xmax, ymin, ymax) of vsr_det_launch_ccl (inclusive boxes); moving: host uint8 [H,W]"""
    H, W = moving.shape
    # the moving pixels of any box in four look-ups
    table = np.zeros((H + 1, W + 1), np.int64)
    table[1:, 1:] = np.cumsum(np.cumsum(moving != 0, axis=0, dtype=np.int64), axis=1)

    def count(y0, y1, x0, x1):
        return int(table[y1, x1] - table[y0, x1] - table[y1, x0] + table[y0, x0])

    kept = []
    for _, area, xmin, xmax, ymin, ymax in np.asarray(comps, dtype=np.int64).reshape(-1, 6).tolist():
        y0, y1, x0, x1 = ymin, ymax + 1, xmin, xmax + 1
        if area < MIN_AREA or x1 - x0 > W // 3 or y1 - y0 > H // 3:
            continue
        ry0, ry1, rx0, rx1 = max(y0 - RING, 0), min(y1 + RING, H), max(x0 - RING, 0), min(x1 + RING, W)
        ring = (ry1 - ry0) * (rx1 - rx0) - (y1 - y0) * (x1 - x0)
        if 2 * (count(ry0, ry1, rx0, rx1) - count(y0, y1, x0, x1)) >= ring:
            kept.append((area, y0, y1, x0, x1))
    kept.sort(key=lambda c: (-c[0], c[1], c[3]))
    areas = [(max(y0 - PAD, 0), min(y1 + PAD, H), max(x0 - PAD, 0), min(x1 + PAD, W)) for _, y0, y1, x0, x1 in kept[:MAX_AREAS]]
    return sorted(areas, key=lambda b: (b[0], b[2])), max(len(kept) - MAX_AREAS, 0)


def _p(t):
    return C.c_void_p(t.data_ptr())


class Scan:
    """the per-pixel state of one scan on one device.  feed() takes sampled frames in any pieces -- the planes are integers, min, max
    and a count, so the pieces give what one call gives -- and areas() ends the scan."""

    def __init__(self, H, W, device=0, keep=False):
        """keep: the frames fed stay referenced in `pieces` [(frames, idx)] until the scan is dropped (--logo-unblend estimates its planes
        from them, tools/unblend.py): a resident clip as it is, an uploaded batch as uploaded"""
        import torch

        if not torch.cuda.is_available():
            raise RuntimeError("the logo scan runs on the MI355X path only: no HIP device available")
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        self.H, self.W, self.fed = int(H), int(W), 0
        self.keep, self.pieces = bool(keep), []
        self.lo = torch.empty((H, W), dtype=torch.uint8, device=self.device)
        self.hi = torch.empty((H, W), dtype=torch.uint8, device=self.device)
        self.edges = torch.empty((H, W), dtype=torch.int16, device=self.device)      # (uint16 to the kernels)

    def feed(self, frames, idx=None):
        """frames: uint8 [k,H,W,3] BGR on the device, every frame contiguous; idx: the numbers (into `frames`) of the frames to take,
        None = all of them.  One launch on the current stream."""
        import torch

        from ..._lib import check, lib

        k = int(frames.shape[0])
        idx = list(range(k)) if idx is None else [int(i) for i in idx]
        if not idx:
            return
        assert frames.dtype == torch.uint8 and frames.device == self.device and tuple(frames.shape[1:]) == (self.H, self.W, 3)
        assert frames.stride(3) == 1 and frames.stride(2) == 3 and frames.stride(1) == 3 * self.W, "every frame must be contiguous [H,W,3]"
        assert min(idx) >= 0 and max(idx) < k, "a sampled frame outside the frames given"
        stride = frames.stride(0) if k > 1 else self.H * self.W * 3
        with torch.cuda.device(self.device):
            idx_dev = torch.tensor(idx, dtype=torch.int32, device=self.device)
            stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            check(lib.vsr_static_accum(_p(frames), stride, _p(idx_dev), len(idx), self.H, self.W, GE, 0 if self.fed else 1,
                                       _p(self.lo), _p(self.hi), _p(self.edges), stream))
        if self.keep:
            self.pieces.append((frames, idx))
        self.fed += len(idx)
        stats["frames"] += len(idx)
        stats["accum_launches"] += 1

    def maps(self, need=None):
        """-> (grown float [H,W], moving uint8 [H,W]) on the device: vsr_static_classify at need = M - M // 8 of the M frames fed"""
        import torch

        from ..._lib import check, lib

        M = self.fed
        need = M - M // 8 if need is None else int(need)
        grown = torch.empty((self.H, self.W), dtype=torch.float32, device=self.device)
        moving = torch.empty((self.H, self.W), dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            check(lib.vsr_static_classify(_p(self.lo), _p(self.hi), _p(self.edges), self.H, self.W, need, MV, D, _p(grown), _p(moving), stream))
        return grown, moving

    def components(self, grown):
        """host int32 [k,6] rows (label, area, xmin, xmax, ymin, ymax): the 8-connected components of grown > 0.5 (vsr_det_launch_ccl)"""
        import torch

        from ..._lib import check, lib

        H, W, i32 = self.H, self.W, torch.int32
        with torch.cuda.device(self.device):
            stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            labels = torch.empty(H * W, dtype=i32, device=self.device)
            work = torch.empty(H * W * 5, dtype=i32, device=self.device)
            count = torch.zeros(4, dtype=i32, device=self.device)
            cap = COMPONENT_CAP
            while True:
                comps = torch.empty(cap * 6, dtype=i32, device=self.device)
                check(lib.vsr_det_launch_ccl(_p(grown), H, W, C.c_float(0.5), _p(labels), _p(work), _p(comps), cap, _p(count), stream))
                found = int(count[0].item())
                if found <= cap:
                    return comps.cpu().numpy().reshape(cap, 6)[:found]
                cap = found

    def areas(self):
        """-> [(ymin, ymax, xmin, xmax)] of the frames fed so far"""
        if self.fed < MIN_FRAMES:
            raise ValueError(f"logo scan: {self.fed} sampled frames, a scan needs at least {MIN_FRAMES}")
        grown, moving = self.maps()
        comps = self.components(grown)
        areas, dropped = select_areas(comps, moving.cpu().numpy())
        stats["scans"] += 1
        stats["components"] += len(comps)
        stats["areas"] += len(areas)
        stats["dropped"] += dropped
        self.dropped = dropped
        return areas


def find_areas(video, device=0, clip=None, report=None):
    """the static overlays of a video -> [(ymin, ymax, xmin, xmax)], sorted by (ymin, xmin): run_scan(...).found"""
    return run_scan(video, device=device, clip=clip, report=report).found


def run_scan(video, device=0, clip=None, report=None, keep=False):
    """-> the Scan of a video, its areas [(ymin, ymax, xmin, xmax)], sorted by (ymin, xmin), in `found`; keep: its sampled frames stay on
    the device with it (Scan.pieces: at most 120 frames).  `video`: a path or frame source accepted
    by video_io.open_video; clip: the same video resident in HBM (tools/resident.ResidentClip) -- the kernel then reads the sampled
    frames where they are, in one launch.  Without one (host frames, or a windowed clip, which holds no frame yet) the video is read
    once more and its sampled frames are uploaded in batches.  report(text), if given, is told of components dropped over MAX_AREAS."""
    import torch

    from .video_io import open_video

    if clip is not None and not getattr(clip, "windowed", False):
        N, H, W, _ = clip.frames.shape
        idx = sample_indices(N)
        scan = Scan(H, W, clip.frames.device, keep=keep)
        scan.feed(clip.frames, idx)
    else:
        reader = open_video(video)
        try:
            info = reader.info()
            wanted = set(sample_indices(info["len"]))
            H, W = info["H_ori"], info["W_ori"]
            scan = Scan(H, W, device, keep=keep)
            batch, no = [], 0

            def flush():
                if batch:
                    with torch.cuda.device(scan.device):
                        scan.feed(torch.from_numpy(np.ascontiguousarray(np.stack(batch))).to(scan.device))
                        torch.cuda.synchronize(scan.device)
                    batch.clear()

            while no <= max(wanted):                      # (nothing behind the last sample is decoded)
                ok, fr = reader.read()
                if not ok:
                    break
                if no in wanted:
                    if fr.shape != (H, W, 3) or fr.dtype != np.uint8:
                        raise ValueError(f"frame of shape {fr.shape} / {fr.dtype}, expected ({H}, {W}, 3) uint8")
                    batch.append(fr if fr.flags.owndata else fr.copy())
                    if len(batch) == BATCH_FRAMES:
                        flush()
                no += 1
            flush()
        finally:
            reader.release()
    areas = scan.areas()
    if scan.dropped and report is not None:
        report(f"logo scan: {scan.dropped} more static component{'s' if scan.dropped != 1 else ''} found than the {MAX_AREAS} kept "
               "(the largest); box the others with -c")
    scan.found = areas
    return scan
