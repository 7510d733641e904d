"""Frame sources / sinks for the plugins (reference backend/tools/video_io.py: FramePrefetcher :12-51, FFmpegVideoWriter :54-103).

Codec work stays out of scope: nothing here decodes or encodes a compressed stream itself.  What is
provided is what the hot path needs to be a drop-in -- `read() -> (ok, frame)` / `write(frame)` objects over containers of RAW
frames, an ffmpeg pipe when a binary exists (the reference's own transport, same command line), threads on both sides so that
reading and writing overlap the GPU work, and a loud failure when nothing can serve a path:

  source                      sink
  ArrayVideo (in memory)      ArrayWriter / CountingWriter
  *.npy   uint8 [N,H,W,3] BGR NpyWriter         (memory-mapped, lossless: the parity container)
  *.y4m   YUV4MPEG2           Y4mWriter         (C444 / C422 / C420 / mono at 8, 10 or 12 bits, BT.601; what `ffmpeg -i x.mp4 x.y4m`
                                                writes; the colour conversion runs on the GPU, csrc/io_kernels.hip; VSR_Y4M_OUT=source:
                                                the sink takes the source's format and keeps the samples nothing changed)
  anything else               FFmpegVideoWriter (needs an `ffmpeg` on PATH or $VSR_FFMPEG; else cv2 if importable; else an error)
"""
import os
import queue
import re
import shutil
import subprocess
import threading

import numpy as np


# ------------------------------------------------------------------------------------------------------------------------
# in-memory
# ------------------------------------------------------------------------------------------------------------------------
class ArrayVideo:
    """In-memory clip: uint8 [N,H,W,3] BGR.  Stands in for a video path."""

    def __init__(self, frames, fps=30.0):
        self.frames = frames
        self.fps = float(fps)
        self._pos = 0

    def info(self):
        n, h, w, _ = self.frames.shape
        return {"W_ori": int(w), "H_ori": int(h), "fps": self.fps, "len": int(n)}

    def read(self):
        if self._pos >= len(self.frames):
            return False, None
        f = self.frames[self._pos]
        self._pos += 1
        return True, f

    def release(self):
        pass


class ArrayWriter:
    """Collects written frames (the reference's writer converts non-uint8 by clip+cast, video_io.py:85-92)."""

    def __init__(self):
        self.frames = []

    def write(self, frame):
        if frame.dtype != np.uint8:
            frame = np.clip(frame, 0, 255).astype(np.uint8)
        self.frames.append(frame.copy())        # the caller may hand out views of a recycled (pinned) buffer

    def release(self):
        pass


class CountingWriter:
    """Sink that only counts (benchmarks: the encoder is out of scope)."""

    def __init__(self):
        self.count = 0
        self.checksum = 0

    def write(self, frame):
        self.count += 1
        self.checksum = (self.checksum + int(frame[::97, ::89].sum())) & 0xFFFFFFFF

    def release(self):
        pass


# ------------------------------------------------------------------------------------------------------------------------
# raw containers
# ------------------------------------------------------------------------------------------------------------------------
class NpyVideo:
    """*.npy holding uint8 [N,H,W,3] BGR frames, memory-mapped."""

    def __init__(self, path, fps=None):
        self.frames = np.load(path, mmap_mode="r")
        if self.frames.ndim != 4 or self.frames.shape[3] != 3 or self.frames.dtype != np.uint8:
            raise RuntimeError(f"{path}: expected a uint8 array [N,H,W,3], found {self.frames.dtype} {self.frames.shape}")
        side = os.path.splitext(path)[0] + ".fps"
        self.fps = float(fps) if fps else (float(open(side).read()) if os.path.exists(side) else 30.0)
        self._pos = 0

    def info(self):
        n, h, w, _ = self.frames.shape
        return {"W_ori": int(w), "H_ori": int(h), "fps": self.fps, "len": int(n)}

    def read(self):
        if self._pos >= self.frames.shape[0]:
            return False, None
        f = np.array(self.frames[self._pos])
        self._pos += 1
        return True, f

    def release(self):
        self.frames = None


class NpyWriter:
    """Appends frames to a memory-mapped *.npy (header rewritten on release with the final count)."""

    def __init__(self, path, fps, size, capacity=None):
        self.path, self.fps = path, float(fps)
        self.w, self.h = int(size[0]), int(size[1])
        self.capacity = int(capacity) if capacity else 0
        self.n = 0
        self._mm = None
        self._done = False
        self._tmp = path + ".part"
        self._raw = open(self._tmp, "wb") if not self.capacity else None
        if self.capacity:
            self._mm = np.lib.format.open_memmap(path, mode="w+", dtype=np.uint8, shape=(self.capacity, self.h, self.w, 3))

    def write(self, frame):
        if frame.dtype != np.uint8:
            frame = np.clip(frame, 0, 255).astype(np.uint8)
        if frame.shape != (self.h, self.w, 3):
            raise ValueError(f"frame {frame.shape} does not match the writer's {(self.h, self.w, 3)}")
        if self._mm is not None and self.n < self.capacity:
            self._mm[self.n] = frame
        else:
            if self._raw is None:
                self._raw = open(self._tmp, "wb")
            self._raw.write(np.ascontiguousarray(frame).tobytes())
        self.n += 1

    def release(self):
        if self._done:
            return
        self._done = True
        if self._mm is not None and self._raw is None and self.n == self.capacity:
            self._mm.flush()
            self._mm = None
        else:                                       # unknown or wrong frame count: assemble the final file
            head = np.array(self._mm[: min(self.n, self.capacity)]) if self._mm is not None else None
            self._mm = None
            if self._raw is not None:
                self._raw.close()
            out = np.lib.format.open_memmap(self.path + ".new", mode="w+", dtype=np.uint8, shape=(self.n, self.h, self.w, 3))
            k = 0
            if head is not None:
                out[: head.shape[0]] = head
                k = head.shape[0]
            if os.path.exists(self._tmp) and self.n > k:
                out[k:] = np.fromfile(self._tmp, dtype=np.uint8).reshape(self.n - k, self.h, self.w, 3)
            out.flush()
            del out
            os.replace(self.path + ".new", self.path)
        if os.path.exists(self._tmp):
            os.remove(self._tmp)
        with open(os.path.splitext(self.path)[0] + ".fps", "w") as f:
            f.write(repr(self.fps))


# BT.601 studio-swing integer matrices (the ones libswscale and OpenCV use for 8-bit YCbCr <-> RGB), 16.16 fixed point
_DEC8 = {False: (76309, 104597, -25675, -53279, 132201), True: (65536, 91881, -22554, -46802, 116130)}        # ky, krv, kgu, kgv, kbu
_ENC8 = {False: (16829, 33039, 6416, -9714, -19070, 28784, 28784, -24103, -4681),                               # rows Y, U, V over (R, G, B)
         True: (19595, 38470, 7471, -11059, -21709, 32768, 32768, -27439, -5329)}
DEPTHS = (8, 10, 12)


def color_constants(depth, full_range):
    """{"dec": 5 ints, "enc": 9 ints, "yoff", "coff", "peak", "s"} of one depth and range.  Studio range keeps the 8-bit constants (the
    shifts grow by s = depth - 8); full range has its peak white at 2^depth - 1 and not at 255 << s, so the 8-bit constants are
    rescaled once, floor(x + 0.5) in double -- the expression the launcher in csrc/io_kernels.hip uses (vsr_io_color_constants)."""
    if depth not in DEPTHS:
        raise ValueError(f"depth {depth} is not supported ({', '.join(map(str, DEPTHS))} are)")
    full_range, s = bool(full_range), depth - 8
    peak = (1 << depth) - 1
    dec, enc = _DEC8[full_range], _ENC8[full_range]
    if full_range:
        dec = tuple(int(np.floor(float(k) * float(255 << s) / float(peak) + 0.5)) for k in dec)
        enc = tuple(int(np.floor(float(k) * float(peak) / float(255 << s) + 0.5)) for k in enc)
    return {"dec": dec, "enc": enc, "yoff": 0 if full_range else 16 << s, "coff": 128 << s, "peak": peak, "s": s}


def _yuv_to_bgr(y, u, v, full_range, depth=8):
    k = color_constants(depth, full_range)
    ky, krv, kgu, kgv, kbu = k["dec"]
    rnd, sh = 1 << (15 + k["s"]), 16 + k["s"]
    y = np.minimum(y.astype(np.int32), k["peak"])         # stored samples above the peak come from outside the program
    u = np.minimum(u.astype(np.int32), k["peak"]) - k["coff"]
    v = np.minimum(v.astype(np.int32), k["peak"]) - k["coff"]
    c = ky * (y - k["yoff"])
    r = (c + krv * v + rnd) >> sh
    g = (c + kgu * u + kgv * v + rnd) >> sh
    b = (c + kbu * u + rnd) >> sh
    return np.clip(np.stack([b, g, r], axis=-1), 0, 255).astype(np.uint8)


def _bgr_to_yuv(frame, full_range, depth=8):
    k = color_constants(depth, full_range)
    e = k["enc"]
    rnd, sh = 1 << (15 - k["s"]), 16 - k["s"]
    b, g, r = (frame[..., i].astype(np.int32) for i in range(3))
    y = ((e[0] * r + e[1] * g + e[2] * b + rnd) >> sh) + k["yoff"]
    u = ((e[3] * r + e[4] * g + e[5] * b + rnd) >> sh) + k["coff"]
    v = ((e[6] * r + e[7] * g + e[8] * b + rnd) >> sh) + k["coff"]
    dt = np.uint8 if depth == 8 else np.dtype("<u2")
    return (np.clip(p, 0, k["peak"]).astype(dt) for p in (y, u, v))


# ---- records of one format: {"W", "H", "cw", "ch", "depth", "full_range"} (cw == 0: mono) --------------------------------------------
def chroma_size(chroma, W, H):
    """(cw, ch) of "444" / "422" / "420" / "mono" """
    return {"444": (W, H), "422": ((W + 1) // 2, H), "420": ((W + 1) // 2, (H + 1) // 2), "mono": (0, 0)}[chroma]


def record_bytes(fmt):
    return (2 if fmt["depth"] > 8 else 1) * (fmt["W"] * fmt["H"] + 2 * fmt["cw"] * fmt["ch"])


def split_record(rec, fmt):
    """(Y [H,W], U [ch,cw] | None, V | None): views of a stored record (uint8 bytes), samples as stored"""
    W, H, cw, ch = fmt["W"], fmt["H"], fmt["cw"], fmt["ch"]
    a = np.frombuffer(rec, dtype=np.uint8, count=record_bytes(fmt)).view(np.uint8 if fmt["depth"] == 8 else np.dtype("<u2"))
    y = a[: W * H].reshape(H, W)
    if cw == 0:
        return y, None, None
    return y, a[W * H: W * H + cw * ch].reshape(ch, cw), a[W * H + cw * ch:].reshape(ch, cw)


def _up(p, fmt):
    """nearest chroma up-sampling to the luma grid"""
    W, H = fmt["W"], fmt["H"]
    if p.shape == (H, W):
        return p
    ry, rx = (1 if fmt["ch"] == H else 2), (1 if fmt["cw"] == W else 2)
    return np.repeat(np.repeat(p, ry, axis=0), rx, axis=1)[:H, :W]


def _blocks(p, fmt, pad_mode="edge"):
    """[ch, cw, ry*rx]: the pixels of every chroma block, edge pixels repeated for odd sizes"""
    W, H, cw, ch = fmt["W"], fmt["H"], fmt["cw"], fmt["ch"]
    ry, rx = (1 if ch == H else 2), (1 if cw == W else 2)
    p = np.pad(p, ((0, ch * ry - H), (0, cw * rx - W)), mode=pad_mode)
    return p.reshape(ch, ry, cw, rx).transpose(0, 2, 1, 3).reshape(ch, cw, ry * rx)


def _block_mean(p, fmt):
    """the writer's sub-sampler: rounded mean of the block ((a + b + 1) >> 1, (a + b + c + d + 2) >> 2)"""
    b = _blocks(p.astype(np.int32), fmt)
    n = b.shape[2]
    return ((b.sum(axis=2) + (n >> 1)) >> (n.bit_length() - 1)).astype(p.dtype)


def decode_record(rec, fmt):
    """the reader's statement: stored record -> uint8 BGR [H,W,3]"""
    y, u, v = split_record(rec, fmt)
    if u is None:
        mid = np.full_like(y, 128 << (fmt["depth"] - 8))
        return np.repeat(_yuv_to_bgr(y, mid, mid, fmt["full_range"], fmt["depth"])[..., :1], 3, axis=2)
    return _yuv_to_bgr(y, _up(u, fmt), _up(v, fmt), fmt["full_range"], fmt["depth"])


def _join(y, u, v):
    parts = [y] if u is None else [y, u, v]
    return np.concatenate([np.ascontiguousarray(p).reshape(-1).view(np.uint8) for p in parts])


def encode_frame(frame, fmt):
    """the writer's plain statement: uint8 BGR [H,W,3] -> stored record (uint8 bytes)"""
    y, u, v = _bgr_to_yuv(frame, fmt["full_range"], fmt["depth"])
    if fmt["cw"] == 0:
        return _join(y, None, None)
    return _join(y, _block_mean(u, fmt), _block_mean(v, fmt))


def keep_record(src, frame, fmt):
    """THE KEEP RULE (the definition; csrc/io_kernels.hip k_io_bgr_to_planes<KEEP> equals it bit for bit): a luma sample whose pixel
    decodes from the source record to exactly the frame's colour is copied from the source; so is a chroma sample when every real pixel
    of its block does; everything else is encoded from the frame.  src: the stored source record, frame: the final uint8 BGR frame."""
    ys, us, vs = split_record(src, fmt)
    same = np.all(decode_record(src, fmt) == frame, axis=-1)
    ye, ue, ve = _bgr_to_yuv(frame, fmt["full_range"], fmt["depth"])
    y = np.where(same, ys, ye)
    if us is None:
        return _join(y, None, None)
    blk = _blocks(same, fmt).all(axis=2)
    return _join(y, np.where(blk, us, _block_mean(ue, fmt)), np.where(blk, vs, _block_mean(ve, fmt)))


# ---- the two device calls every resident loop makes (they differ in buffer names only) ------------------------------------------------
def device_planes_to_bgr(rf, planes_ptr, H, W, bgr_ptr, n, stream_ptr):
    """stored records at planes_ptr (format rf = a reader's planes_format()) -> uint8 BGR [n,H,W,3] at bgr_ptr, on the device"""
    import ctypes as C

    from ..._lib import check, lib

    P = C.c_void_p
    if rf.get("depth", 8) == 8:
        check(lib.vsr_io_yuv_to_bgr(P(planes_ptr), rf["frame_bytes"], H, W, rf["cw"], rf["ch"], int(bool(rf["full_range"])), P(bgr_ptr), n, P(stream_ptr)))
    else:
        check(lib.vsr_io_planes_to_bgr(P(planes_ptr), rf["frame_bytes"], H, W, rf["cw"], rf["ch"], rf["depth"], int(bool(rf["full_range"])),
                                       P(bgr_ptr), n, P(stream_ptr)))


def device_bgr_to_planes(wf, bgr_ptr, H, W, planes_ptr, n, stream_ptr, src_ptr=None, src_fmt=None, path="this loop"):
    """uint8 BGR [n,H,W,3] at bgr_ptr -> records of the writer's format wf (its planes_format()) at planes_ptr.  A writer that keeps
    untouched samples (wf["keep"]) needs the frames' source records on the device as well (src_ptr, their format src_fmt): a loop that
    has none must not write a differently made file in silence."""
    import ctypes as C

    from ..._lib import check, lib

    P = C.c_void_p
    if wf.get("keep"):
        if src_ptr is None or src_fmt is None:
            raise RuntimeError(f"VSR_Y4M_OUT=source: {path} does not carry the source planes to its store")
        if any(src_fmt.get(k, 8 if k == "depth" else None) != wf[k] for k in ("frame_bytes", "cw", "ch", "depth", "full_range")):
            raise RuntimeError(f"VSR_Y4M_OUT=source: {path} reads {src_fmt} but the sink was opened like {wf}")
    elif wf.get("depth", 8) == 8 and wf.get("chroma", "444") in ("444", "420"):      # the default sink: the kernel and the bytes of old
        check(lib.vsr_io_bgr_to_yuv(P(bgr_ptr), H, W, int(bool(wf["subsample_420"])), int(bool(wf["full_range"])), P(planes_ptr),
                                    wf["frame_bytes"], n, P(stream_ptr)))
        return
    check(lib.vsr_io_bgr_to_planes(P(bgr_ptr), H, W, wf["cw"], wf["ch"], wf["depth"], int(bool(wf["full_range"])),
                                   P(src_ptr) if wf.get("keep") else None, wf["frame_bytes"] if wf.get("keep") else 0, P(planes_ptr),
                                   wf["frame_bytes"], n, P(stream_ptr)))


def y4m_out_mode():
    """VSR_Y4M_OUT: "444" (default: the 8-bit 4:4:4 studio-range sink) or "source" (the source's own format, untouched samples kept)"""
    mode = os.environ.get("VSR_Y4M_OUT", "444")
    if mode not in ("444", "source"):
        raise RuntimeError(f"VSR_Y4M_OUT={mode}: expected 444 or source")
    return mode


def _device_color_enabled():
    """the GPU does the colour conversion whenever there is one (VSR_IO_COLOR=host keeps the numpy statement, which is also what a
    machine without a GPU -- where nothing but IO can run anyway -- uses)"""
    if os.environ.get("VSR_IO_COLOR", "device") == "host":
        return False
    try:
        import torch

        return torch.cuda.is_available()
    except ImportError:
        return False


class _DeviceColor:
    """Planar YCbCr <-> packed BGR on the GPU (csrc/io_kernels.hip: vsr_io_yuv_to_bgr / vsr_io_bgr_to_yuv, the integer matrices
    of _yuv_to_bgr / _bgr_to_yuv bit for bit).  numpy needs 47 ms to turn one 1080p 4:2:0 frame into BGR and 26 ms for the way
    back -- the whole 50-frame STTN chunk takes 310 ms on the GPU -- so the raw planes go up as they are on disk (half the bytes
    of the BGR frame), the kernel converts, and the frames come back.  Frames move in batches of up to `batch` (one upload, one
    launch, one download, one synchronisation per batch: beside a busy compute stream every single operation waits for a slot).
    One instance per reader / writer (own stream and pinned staging: the reader works in the caller's or the prefetch thread, the
    writer in AsyncWriter's)."""

    def __init__(self, H, W, frame_bytes, batch=8):
        import ctypes as C

        import torch

        from ..._lib import check, lib

        self.torch, self.C, self.check, self.lib = torch, C, check, lib
        self.dev = torch.device("cuda", torch.cuda.current_device())
        self.H, self.W, self.frame_bytes, self.batch = H, W, frame_bytes, max(1, int(batch))
        self.stream = torch.cuda.Stream(self.dev)
        B, u8 = self.batch, torch.uint8
        with torch.cuda.stream(self.stream):
            self.d_planes = torch.empty((B, frame_bytes), dtype=u8, device=self.dev)
            self.d_bgr = torch.empty((B, H, W, 3), dtype=u8, device=self.dev)
        self.pin_planes = torch.empty((B, frame_bytes), dtype=u8).pin_memory()
        self.pin_bgr = torch.empty((B, H, W, 3), dtype=u8).pin_memory()

    def _p(self, t):
        return self.C.c_void_p(t.data_ptr())

    def planes_buffer(self):
        """pinned host records [batch][frame_bytes]: where the reader puts stored frames / where from_bgr leaves converted ones"""
        return self.pin_planes.numpy()

    def bgr_buffer(self):
        """pinned host frames [batch][H][W][3]: where the writer collects frames / where to_bgr leaves converted ones"""
        return self.pin_bgr.numpy()

    def to_bgr(self, n, cw, ch, full_range, depth=8):
        """the first n records of planes_buffer() -> the first n frames of bgr_buffer()"""
        t = self.torch
        rf = {"frame_bytes": self.frame_bytes, "cw": cw, "ch": ch, "full_range": full_range, "depth": depth}
        with t.cuda.stream(self.stream):
            self.d_planes[:n].copy_(self.pin_planes[:n], non_blocking=True)
            device_planes_to_bgr(rf, self.d_planes.data_ptr(), self.H, self.W, self.d_bgr.data_ptr(), n, self.stream.cuda_stream)
            self.pin_bgr[:n].copy_(self.d_bgr[:n], non_blocking=True)
        self.stream.synchronize()
        return self.pin_bgr.numpy()[:n]

    def source_buffer(self):
        """pinned host records [batch][frame_bytes] of a keeping writer: the source records of the frames in bgr_buffer()"""
        if getattr(self, "pin_src", None) is None:
            self.pin_src = self.torch.empty((self.batch, self.frame_bytes), dtype=self.torch.uint8).pin_memory()
            with self.torch.cuda.stream(self.stream):
                self.d_src = self.torch.empty((self.batch, self.frame_bytes), dtype=self.torch.uint8, device=self.dev)
        return self.pin_src.numpy()

    def from_bgr(self, n, subsample_420, full_range, fmt=None, n_src=0):
        """the first n frames of bgr_buffer() -> the first n records of planes_buffer().  fmt: a writer's planes_format() (else 8-bit
        4:4:4 / 4:2:0); with fmt["keep"] the first n_src frames go with the records of source_buffer() (the rest is plainly encoded)"""
        t = self.torch
        if fmt is None:
            fmt = {"frame_bytes": self.frame_bytes, "subsample_420": subsample_420, "full_range": full_range}
        plain = dict(fmt, keep=False)
        st = self.stream.cuda_stream
        with t.cuda.stream(self.stream):
            self.d_bgr[:n].copy_(self.pin_bgr[:n], non_blocking=True)
            k = min(n, n_src) if fmt.get("keep") else 0
            if k:
                self.d_src[:k].copy_(self.pin_src[:k], non_blocking=True)
                device_bgr_to_planes(fmt, self.d_bgr.data_ptr(), self.H, self.W, self.d_planes.data_ptr(), k, st, self.d_src.data_ptr(),
                                     src_fmt=fmt)
            if n > k:
                device_bgr_to_planes(plain, self.d_bgr[k:].data_ptr(), self.H, self.W, self.d_planes[k:].data_ptr(), n - k, st)
            self.pin_planes[:n].copy_(self.d_planes[:n], non_blocking=True)
        self.stream.synchronize()
        return self.pin_planes.numpy()[:n]


class Y4mVideo:
    """YUV4MPEG2 reader: C420* / C422 / C444 / Cmono at 8 bits, C420p10 / C422p10 / C444p10 / Cmono10 and the same with 12 (16-bit
    little-endian samples), progressive; frames come out as 8-bit BGR (BT.601)."""

    def __init__(self, path):
        self.path = path
        self._f = open(path, "rb")
        head = self._f.readline()
        if not head.startswith(b"YUV4MPEG2"):
            raise RuntimeError(f"{path}: not a YUV4MPEG2 stream")
        self.w = self.h = 0
        self.fps, self.chroma = 30.0, "420jpeg"
        for tok in head.split()[1:]:
            t = tok.decode("ascii", "replace")
            if t[0] == "W":
                self.w = int(t[1:])
            elif t[0] == "H":
                self.h = int(t[1:])
            elif t[0] == "F":
                n, d = t[1:].split(":")
                self.fps = float(n) / float(d or 1)
            elif t[0] == "C":
                self.chroma = t[1:]
            elif t[0] == "I" and t[1:] not in ("p", "?"):
                raise RuntimeError(f"{path}: interlaced y4m ({t}) is not supported (progressive streams are)")
        self.header = head                            # the stream-header line as stored (a writer opened `like` this file repeats it)
        supported = "420* / 422 / 444 / mono at 8 bits, 420 / 422 / 444 p10 and p12, mono10, mono12"
        self.depth, kind = 8, self.chroma
        deep = re.fullmatch(r"(420|422|444)p(\d+)|(mono)(\d+)", self.chroma)
        if deep is not None:
            kind, self.depth = deep.group(1) or deep.group(3), int(deep.group(2) or deep.group(4))
            if self.depth not in (10, 12):
                raise RuntimeError(f"{path}: {self.depth}-bit y4m (C{self.chroma}) is not supported ({supported})")
        if kind.startswith("420"):
            self.cw, self.ch = (self.w + 1) // 2, (self.h + 1) // 2
        elif kind == "422":
            self.cw, self.ch = (self.w + 1) // 2, self.h
        elif kind == "444":
            self.cw, self.ch = self.w, self.h
        elif kind == "mono":
            self.cw = self.ch = 0
        else:
            raise RuntimeError(f"{path}: chroma format C{self.chroma} is not supported ({supported})")
        self.full_range = b"XCOLORRANGE=FULL" in head
        self._data0 = self._f.tell()
        self.fmt = {"W": self.w, "H": self.h, "cw": self.cw, "ch": self.ch, "depth": self.depth, "full_range": self.full_range}
        self._fsize = record_bytes(self.fmt)
        self._count = None
        self._dc_args = (self.h, self.w, self._fsize) if _device_color_enabled() else None     # the converter is built on first use
        self._dc_obj = None
        self._ready = []                              # frames converted ahead (device path): popped from the end

    @property
    def _dc(self):
        if self._dc_obj is None and self._dc_args is not None:
            self._dc_obj = _DeviceColor(*self._dc_args)
        return self._dc_obj

    def info(self):
        if self._count is None:                       # constant-size records: "FRAME\n" + planes (frame parameters are rare; counted exactly)
            total = os.path.getsize(self.path) - self._data0
            rec = 6 + self._fsize
            if total % rec == 0:
                self._count = total // rec
            else:
                pos = self._f.tell()
                self._f.seek(self._data0)
                n = 0
                while True:
                    line = self._f.readline()
                    if not line.startswith(b"FRAME"):
                        break
                    self._f.seek(self._fsize, 1)
                    n += 1
                self._f.seek(pos)
                self._count = n
        return {"W_ori": self.w, "H_ori": self.h, "fps": self.fps, "len": int(self._count)}

    def read(self):
        if self._dc is not None:                      # planes as stored -> pinned memory -> GPU -> BGR frames, a batch at a time
            if not self._ready:
                n = self.read_planes_into(self._dc.planes_buffer())
                if n == 0:
                    return False, None
                bgr = self._dc.to_bgr(n, self.cw, self.ch, self.full_range, self.depth)
                self._ready = [bgr[k].copy() for k in range(n - 1, -1, -1)]       # frames of their own: the plugins patch rows into them
            return True, self._ready.pop()
        line = self._f.readline()
        if not line.startswith(b"FRAME"):
            return False, None
        buf = self._f.read(self._fsize)
        if len(buf) < self._fsize:
            return False, None
        return True, decode_record(buf, self.fmt)     # nearest chroma up-sampling

    # raw access for the device-resident chunk loop (STTNAutoInpaint._run): the planes travel as stored, the GPU converts
    def planes_format(self):
        """None without a GPU; else the layout of one stored frame: [Y: H*W][U: ch*cw][V: ch*cw], `frame_bytes` in all"""
        if self._dc_args is None:
            return None
        if self._ready:
            raise RuntimeError("read() and read_planes_into() cannot be mixed on one reader")
        return {"frame_bytes": self._fsize, "cw": self.cw, "ch": self.ch, "full_range": self.full_range, "depth": self.depth}

    def record_layout(self):
        """{path, data_offset, prefix, frame_bytes, count} when every frame of the file is one fixed-size record (no per-frame parameters):
        what tools/rank_io.py needs to read a chunk by offset; None otherwise"""
        total = os.path.getsize(self.path) - self._data0
        rec = 6 + self._fsize
        if total % rec != 0:
            return None
        return {"path": os.path.abspath(self.path), "data_offset": self._data0, "prefix": b"FRAME\n", "frame_bytes": self._fsize, "count": total // rec}

    def whole_records(self):
        """how many frames read_planes_into will deliver: info()["len"] counts the FRAME lines, a last record cut short has one"""
        layout = self.record_layout()
        if layout is not None:
            return int(layout["count"])
        size, n = os.path.getsize(self.path), 0
        with open(self.path, "rb") as f:
            f.seek(self._data0)
            while f.readline().startswith(b"FRAME") and f.tell() + self._fsize <= size:
                f.seek(self._fsize, 1)
                n += 1
        return n

    def read_planes_into(self, out):
        """fill out[k] (uint8 [n][frame_bytes], e.g. pinned memory) with the next frames as stored; returns how many were read"""
        k = 0
        while k < out.shape[0]:
            line = self._f.readline()
            if not line.startswith(b"FRAME") or self._f.readinto(out[k]) < self._fsize:
                break
            k += 1
        return k

    def skip_records(self, n):
        """pass over the next n stored frames"""
        for _ in range(n):
            if not self._f.readline().startswith(b"FRAME"):
                break
            self._f.seek(self._fsize, 1)

    def release(self):
        self._f.close()


class Y4mWriter:
    """YUV4MPEG2 writer, BT.601.  By default 8-bit studio range, chroma "444" (no sub-sampling loss) or "420"; also "422" / "mono",
    depth 10 / 12 (16-bit little-endian samples) and full range.

    like=<path of a *.y4m source>: the SOURCE'S OWN FORMAT.  Its stream-header line is written verbatim, frame k written through
    write() is paired with record k of the source (read through a handle of this writer's own, in order), and the output record is
    made by the keep rule (keep_record): samples whose decoded colour did not change are copied, not re-encoded.  A run that changes
    nothing writes its input back byte for byte.  A source record that is missing falls back to plain encoding."""

    def __init__(self, path, fps, size, chroma="444", depth=8, full_range=False, like=None):
        self.w, self.h = int(size[0]), int(size[1])
        self._src = None
        if like is not None:
            self._src = Y4mVideo(os.fspath(like))
            if (self._src.w, self._src.h) != (self.w, self.h):
                self._src.release()
                raise RuntimeError(f"{path}: a sink of {self.w}x{self.h} cannot be written like {like} ({self._src.w}x{self._src.h})")
            self.fmt = dict(self._src.fmt)
            chroma = {(self.w, self.h): "444", ((self.w + 1) // 2, self.h): "422", (0, 0): "mono"}.get((self.fmt["cw"], self.fmt["ch"]), "420")
            header = self._src.header
        else:
            if chroma not in ("444", "422", "420", "mono") or depth not in DEPTHS:
                raise ValueError(f"Y4mWriter: chroma {chroma!r} / depth {depth!r}: expected 444 / 422 / 420 / mono and {DEPTHS}")
            cw, ch = chroma_size(chroma, self.w, self.h)
            self.fmt = {"W": self.w, "H": self.h, "cw": cw, "ch": ch, "depth": int(depth), "full_range": bool(full_range)}
            num, den = (int(round(fps * 1001)), 1001) if abs(fps - round(fps)) > 1e-3 else (int(round(fps)), 1)
            tag = {"444": "444", "420": "420mpeg2", "422": "422", "mono": "mono"}[chroma]
            if depth > 8:
                tag = f"mono{depth}" if chroma == "mono" else f"{chroma}p{depth}"
            header = f"YUV4MPEG2 W{self.w} H{self.h} F{num}:{den} Ip A1:1 C{tag} XCOLORRANGE={'FULL' if full_range else 'LIMITED'}\n".encode()
        self.chroma = chroma
        self._plain = like is None and self.fmt["depth"] == 8 and not self.fmt["full_range"] and chroma in ("444", "420")
        self._f = open(path, "wb", buffering=1 << 22)
        self._f.write(header)
        self._header_bytes = self._f.tell()
        self._dc_args = (self.h, self.w, record_bytes(self.fmt)) if _device_color_enabled() else None
        self._dc_obj = None
        self._pending = 0

    @property
    def _dc(self):
        if self._dc_obj is None and self._dc_args is not None:
            self._dc_obj = _DeviceColor(*self._dc_args)
        return self._dc_obj

    def _format(self):
        return {"frame_bytes": record_bytes(self.fmt), "subsample_420": self.chroma == "420", "full_range": self.fmt["full_range"],
                "cw": self.fmt["cw"], "ch": self.fmt["ch"], "depth": self.fmt["depth"], "chroma": self.chroma, "keep": self._src is not None}

    def _flush(self):
        if self._pending:
            n, self._pending = self._pending, 0
            if self._plain:
                recs = self._dc.from_bgr(n, self.chroma != "444", False)
            else:
                k = self._src.read_planes_into(self._dc.source_buffer()[:n]) if self._src is not None else 0
                recs = self._dc.from_bgr(n, False, False, fmt=self._format(), n_src=k)
            self._write_records(recs)

    def write(self, frame):
        if frame.dtype != np.uint8:
            frame = np.clip(frame, 0, 255).astype(np.uint8)
        if self._dc is not None:                      # collected in pinned memory, converted a batch at a time
            self._dc.bgr_buffer()[self._pending] = frame
            self._pending += 1
            if self._pending == self._dc.batch:
                self._flush()
            return
        self._f.write(b"FRAME\n")
        if self._src is not None:
            rec = np.empty((1, record_bytes(self.fmt)), np.uint8)
            if self._src.read_planes_into(rec) == 1:
                self._f.write(keep_record(rec[0], frame, self.fmt).tobytes())
                return
        self._f.write(encode_frame(frame, self.fmt).tobytes())

    def planes_format(self):
        """None without a GPU; else what write_planes expects per frame.  "keep": this writer pairs frames with the records of a
        source (like=...): whoever converts on the device applies the keep rule with those records (device_bgr_to_planes)."""
        if self._dc_args is None:
            return None
        return self._format()

    def _write_records(self, recs):
        for rec in recs:
            self._f.write(b"FRAME\n")
            self._f.write(rec)

    def write_planes(self, recs):
        """frames already converted on the device: uint8 [n][frame_bytes] (by the keep rule, when this writer keeps)"""
        if self._pending:
            self._flush()
        if self._src is not None:
            self._src.skip_records(len(recs))         # the pairing of write() goes on behind them
        self._write_records(recs)

    def record_layout(self, count):
        """For tools/rank_io.py: the header goes to disk, the file is grown to its final size of `count` frames, and the layout of its
        records comes back ({path, data_offset, prefix, frame_bytes}); the ranks then write their records by offset and this object
        writes nothing more.  None when frames were already written through it, or without the device colour conversion."""
        if self._dc_args is None or self._pending or self._f.tell() != self._header_bytes:
            return None
        self._f.flush()
        os.truncate(self._f.name, self._header_bytes + (6 + self._dc_args[2]) * int(count))
        return {"path": os.path.abspath(self._f.name), "data_offset": self._header_bytes, "prefix": b"FRAME\n", "frame_bytes": self._dc_args[2]}

    def release(self):
        if self._dc_obj is not None:
            self._flush()
        if self._src is not None:
            self._src.release()
        self._f.close()


IMAGE_EXTS = (".png", ".jpg", ".jpeg", ".bmp", ".webp", ".tif", ".tiff")      # tools/common_tools.py:8-9


class ImageVideo:
    """A still image as a one-frame source (main.py:353-356 read_image); PIL decodes, frames are BGR like cv2's."""

    def __init__(self, path):
        from PIL import Image

        self.frame = np.ascontiguousarray(np.array(Image.open(path).convert("RGB"))[:, :, ::-1])
        self._done = False

    def info(self):
        return {"W_ori": int(self.frame.shape[1]), "H_ori": int(self.frame.shape[0]), "fps": 1.0, "len": 1}

    def read(self):
        if self._done:
            return False, None
        self._done = True
        return True, self.frame.copy()

    def release(self):
        pass


class ImageWriter:
    def __init__(self, path):
        self.path = path

    def write(self, frame):
        from PIL import Image

        Image.fromarray(np.ascontiguousarray(frame[:, :, ::-1])).save(self.path)

    def release(self):
        pass


# ------------------------------------------------------------------------------------------------------------------------
# ffmpeg pipe / cv2 (only when the tool exists)
# ------------------------------------------------------------------------------------------------------------------------
def ffmpeg_path():
    """$VSR_FFMPEG, else an `ffmpeg` on PATH (the reference ships its own binary, tools/ffmpeg_cli.py:24-35: a missing blob)."""
    p = os.environ.get("VSR_FFMPEG") or shutil.which("ffmpeg")
    return p if p and os.path.exists(p) else None


def probe_stream(probe, path):
    """(width, height, fps, frames) of the first video stream AS DECODED FRAMES ARRIVE: `ffmpeg -i` applies the display-matrix
    rotation (phone portrait clips) by default -- and so does cv2.VideoCapture, the reference's reader, which reports the rotated
    size -- so a quarter-turn rotation swaps width and height here (round 2 took the stored size: every frame of such a clip was
    reshaped with the sides exchanged, silently).  The frame count falls back from the packet count to nb_frames to duration x rate
    when the container does not know it (`N/A`)."""
    import json

    out = subprocess.check_output([probe, "-v", "error", "-select_streams", "v:0", "-count_packets", "-show_entries",
                                   "stream=width,height,r_frame_rate,avg_frame_rate,nb_read_packets,nb_frames,duration:stream_tags=rotate:"
                                   "stream_side_data=rotation:format=duration", "-of", "json", path], text=True)
    doc = json.loads(out)
    st = doc["streams"][0]
    w, h = int(st["width"]), int(st["height"])
    num, den = (st.get("r_frame_rate") or st.get("avg_frame_rate") or "0/1").split("/")
    fps = float(num) / float(den or 1) if float(den or 1) else 0.0
    rot = 0.0
    for sd in st.get("side_data_list", []) or []:
        if "rotation" in sd:
            rot = float(sd["rotation"])
    if not rot and (st.get("tags") or {}).get("rotate") not in (None, ""):
        rot = float(st["tags"]["rotate"])
    if int(round(abs(rot))) % 180 == 90:
        w, h = h, w

    def as_int(v):
        try:
            return int(v)
        except (TypeError, ValueError):
            return None

    n = as_int(st.get("nb_read_packets"))
    if n is None:
        n = as_int(st.get("nb_frames"))
    if n is None:
        dur = st.get("duration") or (doc.get("format") or {}).get("duration")
        try:
            n = int(round(float(dur) * fps))
        except (TypeError, ValueError):
            raise RuntimeError(f"{path}: ffprobe reports neither a packet count, nor nb_frames, nor a duration") from None
    return w, h, fps, n


class FFmpegVideo:
    """`ffmpeg -i path -f rawvideo -pix_fmt bgr24 -` as a frame source; stream facts from `ffprobe` next to the binary."""

    def __init__(self, path):
        ff = ffmpeg_path()
        if ff is None:
            raise RuntimeError("no ffmpeg binary")
        probe = os.path.join(os.path.dirname(ff), "ffprobe")
        probe = probe if os.path.exists(probe) else (shutil.which("ffprobe") or "ffprobe")
        self.w, self.h, self.fps, self.n = probe_stream(probe, path)
        self._p = subprocess.Popen([ff, "-loglevel", "error", "-i", path, "-f", "rawvideo", "-pix_fmt", "bgr24", "-"],
                                   stdout=subprocess.PIPE, stdin=subprocess.DEVNULL, bufsize=1 << 24)

    def info(self):
        return {"W_ori": self.w, "H_ori": self.h, "fps": self.fps, "len": self.n}

    def read(self):
        need = self.w * self.h * 3
        buf = self._p.stdout.read(need)
        if len(buf) < need:
            return False, None
        return True, np.frombuffer(buf, dtype=np.uint8).reshape(self.h, self.w, 3).copy()

    def release(self):
        try:
            self._p.stdout.close()
            self._p.terminate()
            self._p.wait(timeout=5)
        except Exception:
            pass


class FFmpegVideoWriter:
    """Raw bgr24 frames into `ffmpeg ... -c:v libx264 -crf 18 -preset fast` -- the reference's writer (video_io.py:54-103).
    Unlike the reference's, it does not lose errors: a broken pipe (the encoder died) is remembered and raised by the next write /
    by release(), and release() raises when ffmpeg exits non-zero, with what it wrote to stderr (a run must not print
    'written' over a truncated file)."""

    def __init__(self, output_path, fps, size):
        import tempfile

        ff = ffmpeg_path()
        if ff is None:
            raise RuntimeError("no ffmpeg binary")
        w, h = size
        self.output_path = output_path
        cmd = [ff, "-y", "-f", "rawvideo", "-vcodec", "rawvideo", "-s", f"{w}x{h}", "-pix_fmt", "bgr24", "-r", str(fps), "-i", "-",
               "-c:v", "libx264", "-pix_fmt", "yuv420p", "-crf", "18", "-preset", "fast", "-loglevel", "error", output_path]
        self._log = tempfile.TemporaryFile()
        self._process = subprocess.Popen(cmd, stdin=subprocess.PIPE, stdout=subprocess.DEVNULL, stderr=self._log)
        self._broken = None

    def _fail(self, why):
        self._log.seek(0)
        tail = self._log.read()[-2000:].decode("utf-8", "replace").strip()
        return RuntimeError(f"ffmpeg writing {self.output_path}: {why}" + (f"\n{tail}" if tail else ""))

    def write(self, frame):
        if self._broken is not None:
            raise self._fail(f"the encoder is gone ({self._broken})")
        if frame.dtype != np.uint8:
            frame = np.clip(frame, 0, 255).astype(np.uint8)
        try:
            self._process.stdin.write(frame.tobytes())
        except (BrokenPipeError, OSError) as e:
            self._broken = e
            raise self._fail(f"the encoder closed its input ({e})") from e

    def release(self):
        try:
            self._process.stdin.close()
        except (BrokenPipeError, OSError) as e:
            self._broken = self._broken or e
        try:
            self._process.wait(timeout=600)
        except subprocess.TimeoutExpired:
            self._process.terminate()
            self._process.wait(timeout=5)
            raise self._fail("no exit within 600 s after the last frame") from None
        if self._process.returncode != 0:
            raise self._fail(f"exit code {self._process.returncode}")
        if self._broken is not None:
            raise self._fail(f"the encoder closed its input early ({self._broken})")


class Cv2Video:
    """cv2.VideoCapture-backed source (sttn_auto_inpaint.py:168-180); needs opencv-python."""

    def __init__(self, path):
        import cv2

        self._cv2 = cv2
        self.cap = cv2.VideoCapture(path)

    def info(self):
        cv2 = self._cv2
        return {"W_ori": int(self.cap.get(cv2.CAP_PROP_FRAME_WIDTH) + 0.5),
                "H_ori": int(self.cap.get(cv2.CAP_PROP_FRAME_HEIGHT) + 0.5),
                "fps": self.cap.get(cv2.CAP_PROP_FPS),
                "len": int(self.cap.get(cv2.CAP_PROP_FRAME_COUNT) + 0.5)}

    def read(self):
        return self.cap.read()

    def release(self):
        self.cap.release()


# ------------------------------------------------------------------------------------------------------------------------
# threads: reading and writing overlap the GPU work
# ------------------------------------------------------------------------------------------------------------------------
class FramePrefetcher:
    """Background thread that keeps up to `buffer_size` decoded frames ready; same contract as the reference's
    FramePrefetcher (video_io.py:12-51: read / get-like info / stop / release)."""

    def __init__(self, video_cap, buffer_size=10):
        self.cap = video_cap
        self._buffer = queue.Queue(maxsize=buffer_size)
        self._stopped = False
        self._thread = threading.Thread(target=self._read_loop, daemon=True)
        self._thread.start()

    def _read_loop(self):
        while not self._stopped:
            try:
                ret, frame = self.cap.read()
            except Exception:
                ret, frame = False, None
            while not self._stopped:
                try:
                    self._buffer.put((ret, frame), timeout=0.2)
                    break
                except queue.Full:
                    continue
            if not ret:
                break

    def read(self):
        return self._buffer.get()

    def info(self):
        return self.cap.info()

    def stop(self):
        self._stopped = True
        try:
            while not self._buffer.empty():
                self._buffer.get_nowait()
        except queue.Empty:
            pass
        self._thread.join(timeout=5)

    def release(self):
        self.stop()
        self.cap.release()


class AsyncWriter:
    """Writer thread in front of a sink: `write` returns at once (a copy is queued, at most `buffer_size` frames deep), so colour
    conversion / pipe writes / disk IO run beside the GPU; `release` drains, closes the sink and re-raises a sink error."""

    def __init__(self, sink, buffer_size=32):
        self.sink = sink
        self._q = queue.Queue(maxsize=buffer_size)
        self._err = None
        self._t = threading.Thread(target=self._run, daemon=True)
        self._t.start()

    def _run(self):
        while True:
            f = self._q.get()
            if f is None:
                return
            if self._err is None:
                try:
                    if isinstance(f, tuple):
                        self.sink.write_planes(f[1])
                    else:
                        self.sink.write(f)
                except Exception as e:      # keep draining so the producer never blocks on a dead sink
                    self._err = e

    def write(self, frame):
        if self._err is not None:
            raise self._err
        self._q.put(np.array(frame, copy=True))

    def planes_format(self):
        fmt = getattr(self.sink, "planes_format", None)
        return fmt() if fmt is not None else None

    def record_layout(self, count):
        """see Y4mWriter.record_layout (None for sinks without offsets: pipes, image files)"""
        fn = getattr(self.sink, "record_layout", None)
        if fn is None or self._err is not None or not self._q.empty():
            return None
        return fn(count)

    def write_planes(self, recs):
        """a batch of frames converted on the device (see Y4mWriter.write_planes); keeps its place in the frame order"""
        if self._err is not None:
            raise self._err
        self._q.put(("planes", np.array(recs, copy=True)))

    def release(self):
        if self._t is None:                 # already released (the plugin and run() both release, as in the reference)
            return
        self._q.put(None)
        self._t.join()
        self._t = None
        self.sink.release()
        if self._err is not None:
            raise self._err


# ------------------------------------------------------------------------------------------------------------------------
def open_video(video):
    """A fresh reader positioned at frame 0 (the reference re-opens the file for every pass over the video)."""
    if isinstance(video, ArrayVideo):
        return ArrayVideo(video.frames, video.fps)
    if hasattr(video, "read") and hasattr(video, "info"):
        return video
    path = os.fspath(video)
    ext = os.path.splitext(path)[1].lower()
    if ext == ".npy":
        return NpyVideo(path)
    if ext == ".y4m":
        return Y4mVideo(path)
    if ext in IMAGE_EXTS:
        return ImageVideo(path)
    if ffmpeg_path() is not None:
        return FFmpegVideo(path)
    try:
        return Cv2Video(path)
    except ImportError as e:
        raise RuntimeError(f"cannot read {path}: no ffmpeg binary (PATH / $VSR_FFMPEG) and no opencv-python; raw containers (*.y4m, "
                           f"*.npy) and in-memory ArrayVideo clips need neither") from e


def open_writer(path, fps, size, frames=None, like=None):
    """Sink for `path` (size = (W, H)); raises when nothing on this machine can write that container -- never a silent
    in-memory fallback for a file the caller asked for.  like: a *.y4m source whose format a *.y4m sink takes (Y4mWriter)."""
    path = os.fspath(path)
    ext = os.path.splitext(path)[1].lower()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    if ext == ".npy":
        return NpyWriter(path, fps, size, capacity=frames)
    if ext == ".y4m":
        return Y4mWriter(path, fps, size, like=like)
    if ext in IMAGE_EXTS:
        return ImageWriter(path)
    if ffmpeg_path() is not None:
        return FFmpegVideoWriter(path, fps, size)
    try:
        import cv2

        return cv2.VideoWriter(path, cv2.VideoWriter_fourcc(*"mp4v"), fps, size)
    except ImportError as e:
        raise RuntimeError(f"cannot write {path}: no ffmpeg binary (PATH / $VSR_FFMPEG) and no opencv-python on this machine; "
                           f"choose a raw container (-o out.y4m or -o out.npy)") from e
