"""10- and 12-bit *.y4m, and the sink that takes the source's own format and keeps the samples nothing changed
(backend/tools/video_io.py: color_constants, decode_record / encode_frame / keep_record, Y4mVideo, Y4mWriter like=...).  No GPU: the
numpy statements checked here are what tests/test_gpu_y4m_formats.py holds the kernels of csrc/io_kernels.hip to."""
import os

import numpy as np
import pytest

from vsr_amd.backend.tools import video_io

TAGS = {("420", 8): "420jpeg", ("422", 8): "422", ("444", 8): "444", ("mono", 8): "mono"}


def tag_of(chroma, depth):
    if depth == 8:
        return TAGS[(chroma, 8)]
    return f"mono{depth}" if chroma == "mono" else f"{chroma}p{depth}"


def fmt_of(chroma, depth, full, H, W):
    cw, ch = video_io.chroma_size(chroma, W, H)
    return {"W": W, "H": H, "cw": cw, "ch": ch, "depth": depth, "full_range": full}


def random_record(rng, fmt, hi=None):
    """a stored record of random samples over the whole code range (out-of-gamut triples that clip on decode included)"""
    n = fmt["W"] * fmt["H"] + 2 * fmt["cw"] * fmt["ch"]
    a = rng.integers(0, hi or (1 << fmt["depth"]), size=n)
    return a.astype(np.uint8 if fmt["depth"] == 8 else np.dtype("<u2")).view(np.uint8)


def write_raw_y4m(path, recs, fmt, tag, extra=""):
    with open(path, "wb") as f:
        f.write(f"YUV4MPEG2 W{fmt['W']} H{fmt['H']} F25:1 Ip A1:1 C{tag}{' XCOLORRANGE=FULL' if fmt['full_range'] else ''}{extra}\n".encode())
        for rec in recs:
            f.write(b"FRAME\n")
            f.write(rec.tobytes())


def read_all(path):
    r = video_io.Y4mVideo(path)
    out = []
    while True:
        ok, fr = r.read()
        if not ok:
            break
        out.append(fr)
    r.release()
    return np.stack(out)


def records_of(path, fmt):
    raw = open(path, "rb").read()
    body = raw[raw.index(b"\n") + 1:]
    rb = video_io.record_bytes(fmt)
    assert len(body) % (6 + rb) == 0
    recs = []
    for k in range(len(body) // (6 + rb)):
        assert body[k * (6 + rb): k * (6 + rb) + 6] == b"FRAME\n"
        recs.append(np.frombuffer(body[k * (6 + rb) + 6: (k + 1) * (6 + rb)], np.uint8))
    return recs


# the arithmetic of the 8-bit functions as it stood before they took a depth: frozen here, the extended ones must not move it
def _old_yuv_to_bgr(y, u, v, full_range):
    y = y.astype(np.int32)
    u = u.astype(np.int32) - 128
    v = v.astype(np.int32) - 128
    if full_range:
        c = y << 16
        r = (c + 91881 * v + 32768) >> 16
        g = (c - 22554 * u - 46802 * v + 32768) >> 16
        b = (c + 116130 * u + 32768) >> 16
    else:
        c = 76309 * (y - 16)
        r = (c + 104597 * v + 32768) >> 16
        g = (c - 25675 * u - 53279 * v + 32768) >> 16
        b = (c + 132201 * u + 32768) >> 16
    return np.clip(np.stack([b, g, r], axis=-1), 0, 255).astype(np.uint8)


def _old_bgr_to_yuv(frame, full_range):
    b, g, r = (frame[..., k].astype(np.int32) for k in range(3))
    if full_range:
        y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
        u = ((-11059 * r - 21709 * g + 32768 * b + 32768) >> 16) + 128
        v = ((32768 * r - 27439 * g - 5329 * b + 32768) >> 16) + 128
    else:
        y = ((16829 * r + 33039 * g + 6416 * b + 32768) >> 16) + 16
        u = ((-9714 * r - 19070 * g + 28784 * b + 32768) >> 16) + 128
        v = ((28784 * r - 24103 * g - 4681 * b + 32768) >> 16) + 128
    return [np.clip(p, 0, 255).astype(np.uint8) for p in (y, u, v)]


def all_triples():
    """all 2^24 byte triples as a [4096, 4096, 3] array"""
    g = np.arange(256, dtype=np.uint8)
    a, b, c = np.meshgrid(g, g, g, indexing="ij")
    return np.stack([a.reshape(4096, 4096), b.reshape(4096, 4096), c.reshape(4096, 4096)], axis=-1)


# ---- check 1: the reader --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("chroma,depth", [("420", 10), ("422", 10), ("444", 10), ("mono", 10), ("420", 12), ("444", 12)])
def test_reader_high_depth_equals_the_statement(tmp_path, monkeypatch, chroma, depth, full):
    monkeypatch.setenv("VSR_IO_COLOR", "host")
    H, W = 37, 53
    fmt = fmt_of(chroma, depth, full, H, W)
    rng = np.random.default_rng(depth * 100 + H + len(chroma) + int(full))
    recs = [random_record(rng, fmt) for _ in range(3)]
    recs[2] = random_record(rng, fmt, hi=1 << 16)               # samples above the peak: clipped before decoding
    p = str(tmp_path / "v.y4m")
    write_raw_y4m(p, recs, fmt, tag_of(chroma, depth))
    r = video_io.Y4mVideo(p)
    assert r.info() == {"W_ori": W, "H_ori": H, "fps": 25.0, "len": 3}
    lay = r.record_layout()
    assert lay["frame_bytes"] == 2 * (W * H + 2 * fmt["cw"] * fmt["ch"]) == video_io.record_bytes(fmt) and lay["count"] == 3
    assert lay["prefix"] == b"FRAME\n" and lay["data_offset"] == open(p, "rb").read().index(b"\n") + 1
    buf = np.zeros((2, lay["frame_bytes"]), np.uint8)
    assert r.read_planes_into(buf) == 2 and np.array_equal(buf[1], recs[1])
    r.release()
    got = read_all(p)
    assert got.shape == (3, H, W, 3) and got.dtype == np.uint8
    peak = (1 << depth) - 1
    for k, rec in enumerate(recs):
        a = np.minimum(rec.view("<u2").astype(np.int64), peak)
        y = a[: H * W].reshape(H, W)
        if chroma == "mono":
            u = v = np.full((H, W), 128 << (depth - 8))
        else:
            n = fmt["cw"] * fmt["ch"]
            u, v = a[H * W: H * W + n].reshape(fmt["ch"], fmt["cw"]), a[H * W + n:].reshape(fmt["ch"], fmt["cw"])
            ry, rx = (1 if fmt["ch"] == H else 2), (1 if fmt["cw"] == W else 2)
            u = np.repeat(np.repeat(u, ry, axis=0), rx, axis=1)[:H, :W]
            v = np.repeat(np.repeat(v, ry, axis=0), rx, axis=1)[:H, :W]
        want = video_io._yuv_to_bgr(y, u, v, full, depth)
        if chroma == "mono":
            assert np.array_equal(want[..., 0], want[..., 1]) and np.array_equal(want[..., 0], want[..., 2])
        assert np.array_equal(got[k], want)


def test_reader_decodes_known_high_depth_values(tmp_path, monkeypatch):
    """known answers, not the statement against itself: black / white / mid grey at 10 bits in both ranges"""
    monkeypatch.setenv("VSR_IO_COLOR", "host")
    for full, codes in ((False, [(64, 0), (940, 255), (504, 128)]), (True, [(0, 0), (1023, 255), (514, 128)])):
        fmt = fmt_of("444", 10, full, 1, 3)
        rec = np.array([c for c, _ in codes] + [512] * 6, dtype="<u2").view(np.uint8)
        p = str(tmp_path / f"k{int(full)}.y4m")
        write_raw_y4m(p, [rec], fmt, "444p10")
        got = read_all(p)[0, 0]
        assert [tuple(px) for px in got] == [(v, v, v) for _, v in codes]


@pytest.mark.parametrize("tag", ["420p9", "422p14", "444p16", "mono16", "mono9"])
def test_reader_refuses_other_depths(tmp_path, tag):
    p = str(tmp_path / "v.y4m")
    open(p, "wb").write(f"YUV4MPEG2 W4 H4 F25:1 Ip A1:1 C{tag}\nFRAME\n".encode() + bytes(96))
    with pytest.raises(RuntimeError, match="p10 and p12"):
        video_io.Y4mVideo(p)


@pytest.mark.parametrize("field", ["Ii", "It", "Ib", "Im"])
def test_reader_refuses_interlaced(tmp_path, field):
    p = str(tmp_path / "v.y4m")
    open(p, "wb").write(f"YUV4MPEG2 W4 H4 F25:1 {field} A1:1 C420p10\nFRAME\n".encode() + bytes(48))
    with pytest.raises(RuntimeError, match="interlaced"):
        video_io.Y4mVideo(p)


# ---- check 2: depth 8 did not move ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("full", [False, True])
def test_depth_8_is_the_arithmetic_of_old(full):
    t = all_triples()
    assert np.array_equal(video_io._yuv_to_bgr(t[..., 0], t[..., 1], t[..., 2], full, 8), _old_yuv_to_bgr(t[..., 0], t[..., 1], t[..., 2], full))
    assert np.array_equal(video_io._yuv_to_bgr(t[..., 0], t[..., 1], t[..., 2], full), _old_yuv_to_bgr(t[..., 0], t[..., 1], t[..., 2], full))
    for got, want in zip(video_io._bgr_to_yuv(t, full, 8), _old_bgr_to_yuv(t, full)):
        assert got.dtype == np.uint8 and np.array_equal(got, want)
    for got, want in zip(video_io._bgr_to_yuv(t, full), _old_bgr_to_yuv(t, full)):
        assert np.array_equal(got, want)
    rng = np.random.default_rng(int(full))
    y, u, v = (rng.integers(0, 256, size=(61, 67), dtype=np.uint8) for _ in range(3))
    assert np.array_equal(video_io._yuv_to_bgr(y, u, v, full, 8), _old_yuv_to_bgr(y, u, v, full))


# ---- check 3: a 10- or 12-bit 4:4:4 sink carries the models' 8-bit output without loss ----------------------------------------------
@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("depth", [10, 12])
def test_all_bgr_triples_survive_high_depth_444(depth, full):
    t = all_triples()
    y, u, v = video_io._bgr_to_yuv(t, full, depth)
    assert y.dtype == np.dtype("<u2") and int(max(y.max(), u.max(), v.max())) <= (1 << depth) - 1
    assert np.array_equal(video_io._yuv_to_bgr(y, u, v, full, depth), t)


def test_constants_of_depth_10_and_12(built_lib):
    """the full-range constants, rescaled once per depth: the values of the issue, out of the numpy statement AND out of the launcher's
    host code (one expression, floor(x + 0.5) in double, on both sides)"""
    import ctypes as C

    want = {10: ((65344, 91612, -22488, -46665, 115789), (19653, 38583, 7493, -11092, -21773, 32864, 32864, -27520, -5345)),
            12: ((65296, 91544, -22471, -46631, 115705), (19667, 38611, 7498, -11100, -21789, 32888, 32888, -27540, -5349))}
    for depth, (dec, enc) in want.items():
        k = video_io.color_constants(depth, True)
        assert k["dec"] == dec and k["enc"] == enc
        assert (k["yoff"], k["coff"], k["peak"], k["s"]) == (0, 128 << (depth - 8), (1 << depth) - 1, depth - 8)
    for depth in (8, 10, 12):
        for full in (False, True):
            k = video_io.color_constants(depth, full)
            out = (C.c_int32 * 18)()
            assert built_lib.lib.vsr_io_color_constants(depth, int(full), out) == 0
            assert tuple(out) == k["dec"] + k["enc"] + (k["yoff"], k["coff"], k["peak"], k["s"])
        assert video_io.color_constants(depth, False)["dec"] == (76309, 104597, -25675, -53279, 132201)        # studio range: as at 8 bits
    assert video_io.color_constants(8, True)["dec"] == (65536, 91881, -22554, -46802, 116130)
    assert built_lib.lib.vsr_io_color_constants(9, 0, (C.c_int32 * 18)()) == built_lib.VSR_ERR_ARG
    with pytest.raises(ValueError):
        video_io.color_constants(14, False)


def test_bad_arguments_are_refused_without_a_launch(built_lib):
    """no GPU here: a call that got past the argument checks would fail differently (no device), VSR_ERR_ARG comes first"""
    import ctypes as C

    lib, P = built_lib.lib, C.c_void_p
    a = P(4096)                                                   # never dereferenced by the checks
    b = P(1 << 20)
    E = built_lib.VSR_ERR_ARG
    assert lib.vsr_io_planes_to_bgr(a, 48, 4, 4, 2, 2, 9, 0, b, 1, None) == E                      # depth
    assert lib.vsr_io_planes_to_bgr(a, 47, 4, 4, 2, 2, 10, 0, b, 1, None) == E                     # record too small / odd stride
    assert lib.vsr_io_planes_to_bgr(a, 48, 4, 4, 3, 2, 10, 0, b, 1, None) == E                     # chroma geometry
    assert lib.vsr_io_planes_to_bgr(None, 48, 4, 4, 2, 2, 10, 0, b, 1, None) == E
    assert lib.vsr_io_planes_to_bgr(P(4097), 48, 4, 4, 2, 2, 10, 0, b, 1, None) == E               # 16-bit samples at an odd address
    assert lib.vsr_io_bgr_to_planes(a, 4, 4, 2, 2, 14, 0, None, 0, b, 48, 1, None) == E
    assert lib.vsr_io_bgr_to_planes(a, 4, 4, 2, 2, 10, 0, None, 0, b, 46, 1, None) == E
    assert lib.vsr_io_bgr_to_planes(a, 4, 4, 2, 2, 10, 0, b, 40, P(1 << 21), 48, 1, None) == E      # source records too small
    assert lib.vsr_io_bgr_to_planes(a, 4, 4, 2, 2, 8, 0, P((1 << 20) + 8), 24, b, 24, 2, None) == E  # overlapping, not in place
    assert lib.vsr_io_bgr_to_planes(a, 4, 4, 5, 2, 8, 0, None, 0, b, 24, 1, None) == E
    assert lib.vsr_io_bgr_to_planes(a, 0, 4, 2, 2, 8, 0, None, 0, b, 24, 1, None) == E


# ---- check 4: the keep rule -----------------------------------------------------------------------------------------------------
KEEP_CASES = [(c, d, f) for c in ("420", "422", "444", "mono") for d in (8, 10, 12) for f in (False, True)]


def keep_inputs(chroma, depth, full, H=37, W=53, seed=0):
    """(fmt, source record, decoded source, frame that differs from it inside a rectangle with odd corners only, the rectangle)"""
    fmt = fmt_of(chroma, depth, full, H, W)
    rng = np.random.default_rng(1000 * depth + 10 * len(chroma) + int(full) + seed)
    src = random_record(rng, fmt)
    D = video_io.decode_record(src, fmt)
    y0, y1, x0, x1 = 5 + 2 * (seed % 3), 24 + 2 * (seed % 4) + 1, 7 + 2 * (seed % 5), 41 + 2 * (seed % 2)      # odd corners
    F = D.copy()
    F[y0:y1, x0:x1] = rng.integers(0, 256, size=(y1 - y0, x1 - x0, 3), dtype=np.uint8)
    back = rng.random((y1 - y0, x1 - x0)) < 0.2                  # pixels inside that happen to keep their decoded colour
    F[y0:y1, x0:x1][back] = D[y0:y1, x0:x1][back]
    return fmt, src, D, F, (y0, y1, x0, x1)


def write_like(path, like, frames, W, H):
    w = video_io.Y4mWriter(path, 25.0, (W, H), like=like)
    for f in frames:
        w.write(f)
    w.release()


def check_keep_output(out, src, D, F, fmt, plain):
    """the assertions of check 4b on one output record; plain: the plain encoder's record of F in the same format"""
    H, W, cw, ch = fmt["H"], fmt["W"], fmt["cw"], fmt["ch"]
    yo, uo, vo = video_io.split_record(out, fmt)
    ys, us, vs = video_io.split_record(src, fmt)
    yp, up, vp = video_io.split_record(plain, fmt)
    same = np.all(D == F, axis=-1)
    assert 0.05 < (~same).mean() < 0.6
    assert np.array_equal(yo[same], ys[same])                     # outside the rectangle, and inside where the colour stayed
    assert np.array_equal(yo[~same], yp[~same])
    if cw:
        ry, rx = (1 if ch == H else 2), (1 if cw == W else 2)
        blk = np.ones((ch, cw), bool)
        for dy in range(ry):
            for dx in range(rx):
                part = same[dy::ry, dx::rx]
                blk[: part.shape[0], : part.shape[1]] &= part
        assert blk.any() and (~blk).any()
        for o, s, p in ((uo, us, up), (vo, vs, vp)):
            assert np.array_equal(o[blk], s[blk]) and np.array_equal(o[~blk], p[~blk])


@pytest.mark.parametrize("chroma,depth,full", KEEP_CASES)
def test_keep_rule(tmp_path, monkeypatch, chroma, depth, full):
    monkeypatch.setenv("VSR_IO_COLOR", "host")
    fmt, src, D, F, _ = keep_inputs(chroma, depth, full)
    H, W = fmt["H"], fmt["W"]
    sp = str(tmp_path / "src.y4m")
    write_raw_y4m(sp, [src, src], fmt, tag_of(chroma, depth))
    # a. nothing changed: the source comes back byte for byte
    assert np.array_equal(video_io.keep_record(src, D, fmt), src)
    write_like(str(tmp_path / "same.y4m"), sp, [D, D], W, H)
    assert open(str(tmp_path / "same.y4m"), "rb").read() == open(sp, "rb").read()
    # b. changed inside a rectangle
    pw = video_io.Y4mWriter(str(tmp_path / "plain.y4m"), 25.0, (W, H), chroma=chroma, depth=depth, full_range=full)
    pw.write(F)
    pw.release()
    plain = records_of(str(tmp_path / "plain.y4m"), fmt)[0]
    assert np.array_equal(plain, video_io.encode_frame(F, fmt))
    write_like(str(tmp_path / "out.y4m"), sp, [F, D, F], W, H)    # (the third frame has no source record: plain encoding)
    outs = records_of(str(tmp_path / "out.y4m"), fmt)
    assert len(outs) == 3 and np.array_equal(outs[1], src) and np.array_equal(outs[2], plain)
    assert np.array_equal(outs[0], video_io.keep_record(src, F, fmt))
    check_keep_output(outs[0], src, D, F, fmt, plain)
    # what was kept decodes to the frame where the frame was not changed
    back = video_io.decode_record(outs[0], fmt)
    same = np.all(D == F, axis=-1)
    if chroma in ("444", "mono"):
        assert np.array_equal(back[same], F[same])


def test_plain_writer_formats(tmp_path, monkeypatch):
    """4:2:2 is the rounded mean of the horizontal pair with edge replication; the header names the format; what was written reads back"""
    monkeypatch.setenv("VSR_IO_COLOR", "host")
    H, W = 3, 5
    rng = np.random.default_rng(4)
    F = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    for chroma, depth, full, tag in (("422", 8, False, "C422 "), ("422", 10, True, "C422p10 "), ("mono", 12, False, "Cmono12 "), ("420", 12, True, "C420p12 ")):
        p = str(tmp_path / f"{chroma}_{depth}.y4m")
        w = video_io.Y4mWriter(p, 25.0, (W, H), chroma=chroma, depth=depth, full_range=full)
        w.write(F)
        w.release()
        head = open(p, "rb").readline()
        assert tag.encode() in head and (b"XCOLORRANGE=FULL" in head) == full
        fmt = fmt_of(chroma, depth, full, H, W)
        y, u, v = video_io.split_record(records_of(p, fmt)[0], fmt)
        ye, ue, ve = video_io._bgr_to_yuv(F, full, depth)
        assert np.array_equal(y, ye)
        if chroma == "422":
            a = np.pad(ue.astype(np.int64), ((0, 0), (0, 1)), mode="edge")
            assert np.array_equal(u, (a[:, 0::2] + a[:, 1::2] + 1) >> 1)
        r = video_io.Y4mVideo(p)
        assert (r.depth, r.full_range, r.cw, r.ch) == (depth, full, fmt["cw"], fmt["ch"])
        r.release()
    with pytest.raises(ValueError):
        video_io.Y4mWriter(str(tmp_path / "x.y4m"), 25.0, (W, H), depth=9)


# ---- check 5: the header, the switch --------------------------------------------------------------------------------------------
def test_like_writes_the_header_verbatim(tmp_path, monkeypatch):
    monkeypatch.setenv("VSR_IO_COLOR", "host")
    H, W = 6, 8
    fmt = fmt_of("420", 8, True, H, W)
    rec = random_record(np.random.default_rng(0), fmt)
    sp = str(tmp_path / "src.y4m")
    head = b"YUV4MPEG2 W8 H6 F30000:1001 Ip A4:3 C420mpeg2 XCOLORRANGE=FULL XFOO=bar\n"
    open(sp, "wb").write(head + b"FRAME\n" + rec.tobytes())
    op = str(tmp_path / "out.y4m")
    w = video_io.open_writer(op, 29.97, (W, H), like=sp)
    assert w.planes_format() is None                             # no GPU colour conversion here; the format is w.fmt
    assert w.fmt == fmt
    w.write(video_io.decode_record(rec, fmt))
    w.release()
    assert open(op, "rb").readline() == head
    assert open(op, "rb").read() == open(sp, "rb").read()
    with pytest.raises(RuntimeError, match="8x6"):
        video_io.Y4mWriter(op, 25.0, (W + 2, H), like=sp)


def test_source_switch_needs_a_y4m_input(tmp_path, monkeypatch, built_lib):
    from vsr_amd.backend.main import SubtitleRemover
    from vsr_amd.backend.tools.args_handler import parse_args

    np.save(str(tmp_path / "in.npy"), np.zeros((2, 8, 8, 3), np.uint8))
    monkeypatch.setenv("VSR_Y4M_OUT", "source")
    sr = SubtitleRemover(str(tmp_path / "in.npy"))
    sr.video_out_path = str(tmp_path / "out.y4m")
    with pytest.raises(RuntimeError, match="VSR_Y4M_OUT=source"):
        sr.video_writer
    with pytest.raises(RuntimeError, match="VSR_Y4M_OUT=source"):
        sr.run()                                                  # before any work is done
    assert not os.path.exists(sr.video_out_path)
    sr.video_out_path = str(tmp_path / "out.npy")                 # a sink that is no *.y4m is not concerned
    assert sr._y4m_like() is None
    monkeypatch.setenv("VSR_Y4M_OUT", "422")
    with pytest.raises(RuntimeError, match="444 or source"):
        video_io.y4m_out_mode()
    monkeypatch.delenv("VSR_Y4M_OUT")
    sr.video_out_path = str(tmp_path / "out.y4m")
    assert sr._y4m_like() is None                                 # default: today's sink
    assert parse_args(["-i", "x"]).y4m_out is None
    assert parse_args(["-i", "x", "--y4m-out", "source"]).y4m_out == "source"
    with pytest.raises(SystemExit):
        parse_args(["-i", "x", "--y4m-out", "420"])


def test_switch_opens_the_sink_like_the_source(tmp_path, monkeypatch, built_lib):
    from vsr_amd.backend.main import SubtitleRemover

    monkeypatch.setenv("VSR_IO_COLOR", "host")
    H, W = 6, 10
    fmt = fmt_of("420", 10, False, H, W)
    recs = [random_record(np.random.default_rng(k), fmt) for k in range(3)]
    sp = str(tmp_path / "in.y4m")
    write_raw_y4m(sp, recs, fmt, "420p10", extra=" XFOO=bar")
    for mode, first in (("source", open(sp, "rb").readline()), ("444", None)):
        monkeypatch.setenv("VSR_Y4M_OUT", mode)
        sr = SubtitleRemover(sp)
        sr.video_out_path = str(tmp_path / f"out_{mode}.y4m")
        for f in read_all(sp):
            sr.video_writer.write(f)
        sr.video_writer.release()
        if first is not None:
            assert open(sr.video_out_path, "rb").read() == open(sp, "rb").read()
        else:
            assert b"C444 " in open(sr.video_out_path, "rb").readline()


def test_resident_clip_counts_the_kept_planes(built_lib, monkeypatch):
    from vsr_amd.backend.tools.resident import ResidentClip

    monkeypatch.setenv("VSR_RESIDENT_GB", str(100 * 64 * 64 * 3.5 / 2 ** 30))
    assert ResidentClip.fits(100, 64, 64)
    assert ResidentClip.fits(100, 64, 64, 64 * 64 // 2)
    assert not ResidentClip.fits(100, 64, 64, 64 * 64 * 3 // 2)


def test_device_helper_refuses_a_keeping_sink_without_source_planes(built_lib):
    wf = {"frame_bytes": 24, "subsample_420": True, "full_range": False, "cw": 2, "ch": 2, "depth": 8, "chroma": "420", "keep": True}
    with pytest.raises(RuntimeError, match="some loop does not carry the source planes"):
        video_io.device_bgr_to_planes(wf, 0, 4, 4, 0, 1, 0, path="some loop")
    rf = {"frame_bytes": 48, "cw": 2, "ch": 2, "depth": 10, "full_range": False}
    with pytest.raises(RuntimeError, match="opened like"):
        video_io.device_bgr_to_planes(wf, 0, 4, 4, 0, 1, 0, src_ptr=64, src_fmt=rf, path="some loop")
