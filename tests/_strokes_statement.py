"""The definition of --text-detect strokes in plain numpy: the boxes of a frame that hold stroke-like text -- bright or
dark thin strokes with strong contrast against their surroundings, in both orientations, packed densely along a line.  The kernels of
csrc/stroke_kernels.hip are held to `cells` and `text_cells` bit for bit, backend/tools/stroke_det.StrokeTextDetection to `boxes` and
`detect`.  All arithmetic is in integers.

Per frame (uint8 [H,W,3], BGR), at the analysis scale F (the host derives F = clamp(ceil(min(H, W) / 720), 1, 8): `scale`):
    Y = (29 B + 150 G + 77 R + 128) >> 8                                       the luma of --logo-scan
    y[i][j] = (the sum of the F x F lumas + F F // 2) // (F F)                 h = H // F rows, w = W // F columns; the rest is not read
With indices clamped to the analysis frame, along the horizontal direction
    loL = min_{k = 1..S} y[i][j - k], loR = min_{k = 1..S} y[i][j + k], hiL, hiR the maxima over the same pixels;
    (i, j) is a V-stroke pixel (thin horizontally) when y - max(loL, loR) >= C (a bright ridge) or min(hiL, hiR) - y >= C (a dark one),
and the same test along the vertical direction gives the H-stroke pixels.  A step edge is no ridge; a bar wider than S loses its rim, one of 2 S or more is none at all.
    cv[a][b], ch[a][b] = the V- and H-stroke pixels of the CELL x CELL cell, hc = ceil(h / CELL), wc = ceil(w / CELL); outside the frame: 0
    sv, sh = the sums of cv, ch over the (2 WX + 1) x (2 WY + 1) cells centred on the cell (outside the frame: 0)
    text = (sv >= NV) & (sh >= NH)                                             text has strokes both ways, a fence has them one way
The 8-connected components of text, as rows (label, area, xmin, xmax, ymin, ymax) in cells (the rows of vsr_det_launch_ccl), give the
boxes: per component the tight box is the bounding box of the cells with cv + ch >= MINC inside the component's box (none: dropped), hh
and ww its size in analysis pixels, inked the number of such cells in it; it is kept when hh >= MIN_H, ww >= 2 hh and 4 inked >= its
cells.  The result, in source pixels, is (y0 CELL F, min(y1 CELL F, H), x0 CELL F, min(x1 CELL F, W)) with the score inked / cells as
float32, sorted by (ymin, xmin)."""
import numpy as np

from tests import _static_statement as ss

S, C, CELL, WX, WY, NV, NH, MINC, MIN_H = 6, 48, 4, 5, 3, 64, 40, 2, 8


def scale(H, W):
    return min(max(-(-min(H, W) // 720), 1), 8)


def luma(frame):
    return ss.luma(frame)


def analysis(frame, F):
    """int64 [H // F, W // F]: the rounded mean of the F x F lumas"""
    Y = luma(frame)
    h, w = Y.shape[0] // F, Y.shape[1] // F
    return (Y[:h * F, :w * F].reshape(h, F, w, F).sum(axis=(1, 3)) + F * F // 2) // (F * F)


def ridges(y, s=S, c=C):
    """(V-stroke pixels, H-stroke pixels): bool [h,w] each"""
    h, w = y.shape
    out = []
    for axis in (1, 0):
        pad = [(0, 0), (0, 0)]
        pad[axis] = (s, s)
        p = np.pad(y, pad, mode="edge")
        n = y.shape[axis]

        def shifted(d):
            return p[:, s + d:s + d + n] if axis == 1 else p[s + d:s + d + n, :]

        before, after = [shifted(-k) for k in range(1, s + 1)], [shifted(k) for k in range(1, s + 1)]
        lo_b, lo_a, hi_b, hi_a = np.min(before, axis=0), np.min(after, axis=0), np.max(before, axis=0), np.max(after, axis=0)
        out.append((y - np.maximum(lo_b, lo_a) >= c) | (np.minimum(hi_b, hi_a) - y >= c))
    return out[0], out[1]


def cell_counts(flag):
    h, w = flag.shape
    hc, wc = -(-h // CELL), -(-w // CELL)
    p = np.zeros((hc * CELL, wc * CELL), np.int64)
    p[:h, :w] = flag
    return p.reshape(hc, CELL, wc, CELL).sum(axis=(1, 3))


def cells(frame, F, s=S, c=C):
    """(cv, ch): int64 [hc,wc] each, 0..16 -- what vsr_strokes_cells writes"""
    v, hz = ridges(analysis(frame, F), s, c)
    return cell_counts(v), cell_counts(hz)


def box_sum(plane, wx, wy):
    hc, wc = plane.shape
    p = np.zeros((hc + 2 * wy, wc + 2 * wx), np.int64)
    p[wy:wy + hc, wx:wx + wc] = plane
    out = np.zeros((hc, wc), np.int64)
    for dy in range(2 * wy + 1):
        for dx in range(2 * wx + 1):
            out += p[dy:dy + hc, dx:dx + wc]
    return out


def text_cells(cv, ch, wx=WX, wy=WY, nv=NV, nh=NH):
    """bool [hc,wc] -- what vsr_strokes_text writes as 1.0 / 0.0"""
    return (box_sum(cv, wx, wy) >= nv) & (box_sum(ch, wx, wy) >= nh)


def components(text):
    """rows (label, area, xmin, xmax, ymin, ymax) of the 8-connected components, boxes inclusive, label = the raster index of the
    component's first cell: a flood fill, nothing borrowed"""
    H, W = text.shape
    seen = np.zeros((H, W), bool)
    out = []
    for sy, sx in zip(*np.nonzero(text)):
        if seen[sy, sx]:
            continue
        seen[sy, sx] = True
        stack, area, y0, y1, x0, x1 = [(int(sy), int(sx))], 0, int(sy), int(sy), int(sx), int(sx)
        while stack:
            y, x = stack.pop()
            area += 1
            y0, y1, x0, x1 = min(y0, y), max(y1, y), min(x0, x), max(x1, x)
            for ny in range(max(y - 1, 0), min(y + 2, H)):
                for nx in range(max(x - 1, 0), min(x + 2, W)):
                    if text[ny, nx] and not seen[ny, nx]:
                        seen[ny, nx] = True
                        stack.append((ny, nx))
        out.append((int(sy) * W + int(sx), area, x0, x1, y0, y1))
    return out


def boxes(comps, cv, ch, F, H, W):
    """the choice among the components -> ([(ymin, ymax, xmin, xmax)] in source pixels, float32 scores), sorted by (ymin, xmin)"""
    ink = (np.asarray(cv, np.int64) + np.asarray(ch, np.int64)) >= MINC
    kept = []
    for _, _, xmin, xmax, ymin, ymax in np.asarray(comps, dtype=np.int64).reshape(-1, 6).tolist():
        sub = ink[ymin:ymax + 1, xmin:xmax + 1]
        rows, cols = np.nonzero(sub.any(axis=1))[0], np.nonzero(sub.any(axis=0))[0]
        if len(rows) == 0:
            continue
        y0, y1, x0, x1 = ymin + int(rows[0]), ymin + int(rows[-1]) + 1, xmin + int(cols[0]), xmin + int(cols[-1]) + 1
        hh, ww = (y1 - y0) * CELL, (x1 - x0) * CELL
        inked, count = int(ink[y0:y1, x0:x1].sum()), (y1 - y0) * (x1 - x0)
        if hh >= MIN_H and ww >= 2 * hh and 4 * inked >= count:
            kept.append((y0 * CELL * F, min(y1 * CELL * F, H), x0 * CELL * F, min(x1 * CELL * F, W), np.float32(inked) / np.float32(count)))
    kept.sort(key=lambda b: (b[0], b[2], b[1], b[3]))
    return [b[:4] for b in kept], np.array([b[4] for b in kept], np.float32)


def detect(frame, F=None):
    """the whole definition on a frame -> (boxes, scores)"""
    H, W = frame.shape[:2]
    F = scale(H, W) if F is None else F
    cv, ch = cells(frame, F)
    return boxes(components(text_cells(cv, ch)), cv, ch, F, H, W)


def result(found, scores):
    """the detector's result for one frame: quads [[x0,y0],[x1,y0],[x1,y1],[x0,y1]], so tools/ocr.get_coordinates gives (x0, x1, y0, y1)"""
    polys = np.array([[[x0, y0], [x1, y0], [x1, y1], [x0, y1]] for y0, y1, x0, x1 in found], np.int32).reshape(-1, 4, 2)
    return [{"dt_polys": polys, "dt_scores": np.asarray(scores, np.float32)}]


# ---- the test pictures: 144 x 256 backgrounds of tests/_static_statement.py with a line of 5 x 7 block glyphs ---------------------------
FONT = {"E": "#####/#..../#..../####./#..../#..../#####", "H": "#...#/#...#/#...#/#####/#...#/#...#/#...#",
        "L": "#..../#..../#..../#..../#..../#..../#####", "T": "#####/..#../..#../..#../..#../..#../..#..",
        "O": ".###./#...#/#...#/#...#/#...#/#...#/.###.", "A": ".###./#...#/#...#/#####/#...#/#...#/#...#",
        "N": "#...#/##..#/#.#.#/#.#.#/#..##/#...#/#...#", "I": "#####/..#../..#../..#../..#../..#../#####"}
FG, OUTLINE = 235, 16
CORNER = (100, 20)
TEXTS = {2: "HELLO NATION", 3: "HELLO NATION", 4: "HELLO TOT"}           # k: the text (the frame is 256 wide)
BACKGROUNDS = ("wave", "noise", "desk")


def glyph_mask(text, k, shape, corner=CORNER):
    """bool [H,W]: the foreground of `text`, every font pixel k x k, glyph pitch 6 k, top-left corner at (y, x) = corner"""
    m = np.zeros(shape, bool)
    y0, x0 = corner
    for n, ch in enumerate(text):
        if ch == " ":
            continue
        g = np.array([[c == "#" for c in row] for row in FONT[ch].split("/")])
        g = np.repeat(np.repeat(g, k, axis=0), k, axis=1)
        ys, xs = y0, x0 + n * 6 * k
        ye, xe = min(ys + g.shape[0], shape[0]), min(xs + g.shape[1], shape[1])
        if ye > ys and xe > xs:
            m[ys:ye, xs:xe] |= g[:ye - ys, :xe - xs]
    return m


def dilate3(m):
    p = np.pad(m, 1)
    out = np.zeros_like(m)
    for dy in range(3):
        for dx in range(3):
            out |= p[dy:dy + m.shape[0], dx:dx + m.shape[1]]
    return out


def put_text(frame, text, k, corner=CORNER, outline=2):
    """-> (the frame with the glyphs at FG and an outline of `outline` pixels at OUTLINE, the glyphs' mask)"""
    m = glyph_mask(text, k, frame.shape[:2], corner)
    grown = m
    for _ in range(outline):
        grown = dilate3(grown)
    out = frame.copy()
    out[grown] = OUTLINE
    out[m] = FG
    return out, m


def background(name):
    """uint8 [144,256,3]"""
    if name == "wave":
        return ss.wave(1)[0]
    if name == "noise":
        noise = np.random.default_rng(1).integers(-12, 13, size=(ss.CLIP_H, ss.CLIP_W))
        return np.repeat(np.clip(ss.wave(1)[0][..., 0].astype(np.int64) + noise, 0, 255).astype(np.uint8)[..., None], 3, axis=2)
    if name == "desk":
        return ss.clip_desk_logo()[0]
    raise KeyError(name)


def picture(name, k):
    """-> (frame, glyph mask) of the background `name` with TEXTS[k] at scale k"""
    return put_text(background(name), TEXTS[k], k)


def mask_box(m):
    """(ymin, ymax, xmin, xmax), half-open, of a bool mask"""
    ys, xs = np.nonzero(m.any(axis=1))[0], np.nonzero(m.any(axis=0))[0]
    return int(ys[0]), int(ys[-1]) + 1, int(xs[0]), int(xs[-1]) + 1


def large_picture(k):
    """a 288 x 512 wave with "HELLO NATION" at k = 6 or 5, corner (201, 41), outline 3: the pictures above at F = 2"""
    return put_text(ss.wave(1, 288, 512)[0], "HELLO NATION", k, corner=(201, 41), outline=3)


def text_clip(n=ss.CLIP_N, k=2, first=11, last=29):
    """the moving wave of clip_logo with TEXTS[k] on the 1-based frames first..last -> (clip uint8 [n,144,256,3], the glyphs' mask)"""
    clip = ss.wave(n)
    m = None
    for f in range(first - 1, last):
        clip[f], m = put_text(clip[f], TEXTS[k], k)
    return clip, m
