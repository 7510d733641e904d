"""CPU statement of --inpaint-mode opencv: OpenCV's INPAINT_TELEA (A. Telea, "An image inpainting technique based on the
fast marching method", 2004) restated from the paper and from knowledge of the library -- cv2 is not available to this
project, so parity with cv2.inpaint itself is pinned nowhere but in tests/test_gpu_telea.py::test_matches_cv2_if_present.

(a) `serial(img, mask, radius, dt)`: the algorithm as OpenCV orders it, heap and all, plain Python / numpy, written to be read.
(b) `replay(img, schedule, dt)`: the same arithmetic, all pixels of one *level* of a schedule at once (numpy).  The schedule is the
    statement's own (`serial(...)[1]`) or the C++ plan's (`plan_schedule`, read back through the C-ABI).

What the restatement fixes (everything the result depends on):

* Working arrays are padded by one pixel: rows = H + 2, cols = W + 2; pixel (y, x) of the frame is (y + 1, x + 1) there.
  Flags KNOWN / BAND / INSIDE.  INSIDE = mask != 0 (any non-zero value).  band = dilation of the mask by the 3x3 cross minus
  the mask, with the padding border cleared.  T = 0 on the band and 1e6 everywhere else.  T is stored in float32; the eikonal
  solve runs in double and is rounded to float32 when it is stored (OpenCV's `t` is a CV_32F matrix).
* Outer pass: the ring = dilation of the mask by the (2r+1)x(2r+1) square, minus mask, minus band, border cleared, is marched
  outwards from the band (band pixels pushed in raster order with T = 0; mask pixels count as known with T = 1e6 there, which
  never matters because a ring pixel has no 4-neighbour in the mask).  Every pixel popped in this pass (band included) gets
  T = -T afterwards (so the band holds -0.0).
* Main loop: pop the smallest T; mark it KNOWN; visit its 4 neighbours in the order up, left, down, right; skip those on the
  padding border; an INSIDE neighbour gets T = min of the four quadrant solves (up-left, down-left, up-right, down-right,
  compared as float32), is filled AT THAT MOMENT (not when popped), becomes BAND and is pushed.
* The heap is first in, first out among equal T (OpenCV's queue is a sorted list that inserts behind its equals); the initial
  push of the band is in raster order.  Ties are the rule along a straight mask edge, so this decides the order.
* Quadrant solve on (T1, flag1), (T2, flag2), "known" = not INSIDE: both known and |T1-T2| < 1 -> (T1+T2+sqrt(2-(T1-T2)^2))/2;
  both known otherwise -> 1 + min; one known -> 1 + that one; none -> 1 + min.
* Filling pixel (i, j), per channel, with f and T as they are at that moment:
  gradT from the non-INSIDE 4-neighbours: both -> (T+ - T-)/2, only + -> T+ - T, only - -> T - T-, none -> 0.
  For every tap (k, l), k = i-r..i+r outer, l = j-r..j+r inner, that lies inside the unpadded image, is not INSIDE and has
  (k-i)^2 + (l-j)^2 <= r^2:   r = (j-l, i-k) as (x, y);  dst = 1/(|r| sqrt|r|);  lev = 1/(1 + |T(k,l) - T(i,j)|);
  dir = r.x gradT.x + r.y gradT.y, |dir| <= 0.01 -> 1e-6;  w = |dst lev dir|;
  km = k-1+(k==1), kp = k-1-(k==rows-2), lm = l-1+(l==1), lp = l-1-(l==cols-2)  (OpenCV's clamping, unpadded indices: at the
  first row / column the tap's own value is read one pixel further in -- kept as OpenCV has it);
  gradI.x from the non-INSIDE horizontal neighbours of the tap: both -> (I[km][lp+1] - I[km][lm-1]) * 2, only right ->
  I[km][lp+1] - I[km][lm], only left -> I[km][lp] - I[km][lm-1], none -> 0; gradI.y likewise with (kp+1, km-1, kp, km) rows at
  column lm;   Ia += w I[km][lm];  Jx -= w (gradI.x r.x);  Jy -= w (gradI.y r.y);  s += w.
  value = Ia/s + (Jx+Jy)/(sqrt(Jx^2+Jy^2) + 1e-20) + 0.5, then saturate_cast<uchar>(float): round to nearest, ties to even,
  clamp to 0..255 -- the +0.5 is a bias on top of the rounding, both are kept.
  Precision: in OpenCV w, Ia, Jx, Jy, s, gradT, dir are float and dst, lev are computed in double and rounded to float.  The
  statement for dtype dt does every operation in dt, except dst and lev: double, then cast to dt.  dt = float32 is the
  faithful statement, dt = float64 shows what float32 costs.  I is the uint8 image, differences of pixels are exact integers.
* Masked pixels never reached keep their input value (a mask over the whole frame has no band); an empty mask changes nothing.

Schedule ("plan").  Fill order, T, every flag and every weight depend on the mask alone.  step = index in fill order.
level(p) = 1 + max(level of every masked pixel p reads that is already filled, level of every earlier-filled pixel that read
p's location while p was still unfilled).  The second term exists only because of the clamped indices at the frame edge (there
a tap reads one pixel further in, which may be an unfilled masked pixel: the serial order then reads the INPUT value, so the
writer must come in a later level than that reader); in the interior every read is of a non-INSIDE pixel.  All pixels of one
level are independent of each other; each sums its taps in the serial (k, l) order, so a level replay equals the serial
result bit for bit.
"""
import ctypes as C
import heapq
import math
import struct

import numpy as np

KNOWN, BAND, INSIDE = 0, 1, 2
NEIGHBOURS = ((-1, 0), (0, -1), (1, 0), (0, 1))         # up, left, down, right


def _f32(x):
    return struct.unpack("f", struct.pack("f", x))[0]


def _solve(i1, j1, i2, j2, f, t):
    a11, a22 = t[i1][j1], t[i2][j2]
    m12 = min(a11, a22)
    if f[i1][j1] != INSIDE:
        if f[i2][j2] != INSIDE:
            sol = 1 + m12 if abs(a11 - a22) >= 1.0 else (a11 + a22 + math.sqrt(2 - (a11 - a22) * (a11 - a22))) * 0.5
        else:
            sol = 1 + a11
    elif f[i2][j2] != INSIDE:
        sol = 1 + a22
    else:
        sol = 1 + m12
    return _f32(sol)


def _min4(i, j, f, t):
    return min(_solve(i - 1, j, i, j - 1, f, t), _solve(i + 1, j, i, j - 1, f, t),
               _solve(i - 1, j, i, j + 1, f, t), _solve(i + 1, j, i, j + 1, f, t))


def _clear_border(a):
    a[0] = a[-1] = False
    a[:, 0] = a[:, -1] = False


def setup(mask, radius=3):
    """-> (m bool [H+2,W+2], f flags (lists), t float32 values (lists of python floats), heap, counter): state before the main loop"""
    H, W = mask.shape
    m = np.zeros((H + 2, W + 2), bool)
    m[1:-1, 1:-1] = mask != 0
    d = m.copy()
    d[1:] |= m[:-1]; d[:-1] |= m[1:]; d[:, 1:] |= m[:, :-1]; d[:, :-1] |= m[:, 1:]
    band = d & ~m
    _clear_border(band)
    ring = np.zeros_like(m)
    ys, xs = np.nonzero(m)
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            yy, xx = ys + dy, xs + dx
            ok = (yy >= 0) & (yy < H + 2) & (xx >= 0) & (xx < W + 2)
            ring[yy[ok], xx[ok]] = True
    ring &= ~m & ~band
    _clear_border(ring)
    fo = np.zeros(m.shape, np.int8)
    fo[ring] = INSIDE
    t = np.full(m.shape, 1.0e6, np.float32)
    t[band] = 0
    fo_l, t_l = fo.tolist(), t.astype(np.float64).tolist()
    heap, c = [], 0
    for y, x in zip(*np.nonzero(band)):                                      # raster order
        heap.append((0.0, c, int(y), int(x)))
        c += 1
    h2 = list(heap)
    changed = []
    while h2:
        _, _, ii, jj = heapq.heappop(h2)
        changed.append((ii, jj))
        for dy, dx in NEIGHBOURS:
            i, j = ii + dy, jj + dx
            if i <= 0 or j <= 0 or i >= H + 1 or j >= W + 1:
                continue
            if fo_l[i][j] == INSIDE:
                dist = _min4(i, j, fo_l, t_l)
                t_l[i][j] = dist
                fo_l[i][j] = BAND
                heapq.heappush(h2, (dist, c, i, j))
                c += 1
    for ii, jj in changed:
        t_l[ii][jj] = -t_l[ii][jj]
    f = np.zeros(m.shape, np.int8)
    f[band] = BAND
    f[m] = INSIDE
    return m, f.tolist(), t_l, heap, c


def tap_reads(k, l, rows, cols, a, b, a2, b2):
    """the unpadded (y, x) a tap at padded (k, l) reads, given which of its neighbours are known (right, left, down, up)"""
    km = k - 1 + (k == 1); kp = k - 1 - (k == rows - 2)
    lm = l - 1 + (l == 1); lp = l - 1 - (l == cols - 2)
    r = [(km, lm)]
    if a:
        r += [(km, lp + 1), (km, lm - 1)] if b else [(km, lp + 1)]
    elif b:
        r += [(km, lp), (km, lm - 1)]
    if a2:
        r += [(kp + 1, lm), (km - 1, lm)] if b2 else [(kp + 1, lm)]
    elif b2:
        r += [(kp, lm), (km - 1, lm)]
    return r


def saturate_u8(v):
    """OpenCV's saturate_cast<uchar>(float): round half to even, clamp"""
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def serial(img, mask, radius=3, dt=np.float32):
    """-> (out uint8 [H,W,3], schedule).  schedule: dict(H, W, radius, yx int32 [P,2], T float32 [P], level int32 [P]) in fill
    (= step) order, plus tmap float32 [H+2,W+2] (T after the whole pass)."""
    H, W = mask.shape
    assert img.shape == (H, W, 3) and img.dtype == np.uint8 and H >= 3 and W >= 3
    R = radius
    m, f, t, heap, c = setup(mask, R)
    rows, cols = H + 2, W + 2
    out = img.copy()
    lev = [[0] * cols for _ in range(rows)]
    war = [[0] * cols for _ in range(rows)]
    ml = m.tolist()
    yx, Ts, levels = [], [], []
    d0, d2, half = dt(0), dt(2), dt(0.5)
    while heap:
        _, _, ii, jj = heapq.heappop(heap)
        f[ii][jj] = KNOWN
        for dy, dx in NEIGHBOURS:
            i, j = ii + dy, jj + dx
            if i <= 0 or j <= 0 or i >= rows - 1 or j >= cols - 1:
                continue
            if f[i][j] != INSIDE:
                continue
            dist = _min4(i, j, f, t)
            t[i][j] = dist
            ti = dt(dist)
            if f[i][j + 1] != INSIDE:
                gx = (dt(t[i][j + 1]) - dt(t[i][j - 1])) * half if f[i][j - 1] != INSIDE else dt(t[i][j + 1]) - ti
            else:
                gx = ti - dt(t[i][j - 1]) if f[i][j - 1] != INSIDE else d0
            if f[i + 1][j] != INSIDE:
                gy = (dt(t[i + 1][j]) - dt(t[i - 1][j])) * half if f[i - 1][j] != INSIDE else dt(t[i + 1][j]) - ti
            else:
                gy = ti - dt(t[i - 1][j]) if f[i - 1][j] != INSIDE else d0
            Ia = np.zeros(3, dt); Jx = np.zeros(3, dt); Jy = np.zeros(3, dt); s = d0
            L = war[i][j]
            unfilled_reads = []
            for k in range(i - R, i + R + 1):
                for l in range(j - R, j + R + 1):
                    if k <= 0 or l <= 0 or k >= rows - 1 or l >= cols - 1:
                        continue
                    if f[k][l] == INSIDE or (l - j) * (l - j) + (k - i) * (k - i) > R * R:
                        continue
                    ry, rx = dt(i - k), dt(j - l)
                    vl = np.sqrt(dt(rx * rx + ry * ry))
                    dst = dt(1.0 / (float(vl) * math.sqrt(float(vl))))
                    lv = dt(1.0 / (1.0 + abs(float(dt(t[k][l]) - ti))))
                    dr = rx * gx + ry * gy
                    if abs(float(dr)) <= 0.01:
                        dr = dt(0.000001)
                    w = abs(dst * lv * dr)
                    a, b = f[k][l + 1] != INSIDE, f[k][l - 1] != INSIDE
                    a2, b2 = f[k + 1][l] != INSIDE, f[k - 1][l] != INSIDE
                    km = k - 1 + (k == 1); kp = k - 1 - (k == rows - 2)
                    lm = l - 1 + (l == 1); lp = l - 1 - (l == cols - 2)
                    for y, x in tap_reads(k, l, rows, cols, a, b, a2, b2):
                        if ml[y + 1][x + 1]:
                            if f[y + 1][x + 1] != INSIDE:
                                L = max(L, lev[y + 1][x + 1])
                            else:
                                unfilled_reads.append((y + 1, x + 1))
                    o = lambda y, x: out[y, x].astype(dt)                    # noqa: E731
                    if a:
                        gix = (o(km, lp + 1) - o(km, lm - 1)) * d2 if b else o(km, lp + 1) - o(km, lm)
                    else:
                        gix = o(km, lp) - o(km, lm - 1) if b else np.zeros(3, dt)
                    if a2:
                        giy = (o(kp + 1, lm) - o(km - 1, lm)) * d2 if b2 else o(kp + 1, lm) - o(km, lm)
                    else:
                        giy = o(kp, lm) - o(km - 1, lm) if b2 else np.zeros(3, dt)
                    Ia = Ia + w * o(km, lm)
                    Jx = Jx - w * (gix * rx)
                    Jy = Jy - w * (giy * ry)
                    s = s + w
            sat = Ia / s + (Jx + Jy) / (np.sqrt(Jx * Jx + Jy * Jy) + dt(1.0e-20)) + half
            out[i - 1, j - 1] = saturate_u8(sat)
            L += 1
            lev[i][j] = L
            for y, x in unfilled_reads:
                war[y][x] = max(war[y][x], L)
            yx.append((i - 1, j - 1)); Ts.append(dist); levels.append(L)
            f[i][j] = BAND
            heapq.heappush(heap, (dist, c, i, j))
            c += 1
    sched = dict(H=H, W=W, radius=R, yx=np.array(yx, np.int32).reshape(-1, 2), T=np.array(Ts, np.float32),
                 level=np.array(levels, np.int32), tmap=np.array(t, np.float64).astype(np.float32), mask=m[1:-1, 1:-1].copy())
    return out, sched


def replay(img, sched, dt=np.float32, return_weights=False):
    """Level replay: every pixel of a level at once, taps in the serial (k, l) order, flags rebuilt from the step index
    (a masked pixel is known to the pixel of step n iff its own step is < n).  Reads the image in place, like the kernel."""
    H, W, R = sched["H"], sched["W"], sched["radius"]
    rows, cols = H + 2, W + 2
    yx, level = sched["yx"].astype(np.int64), sched["level"]
    P = len(yx)
    out = img.copy()
    big = np.iinfo(np.int64).max
    st = np.full((rows, cols), -1, np.int64)                                  # unmasked: known to everybody
    st[1:-1, 1:-1][sched["mask"]] = big                                       # masked and never reached: known to nobody
    st[yx[:, 0] + 1, yx[:, 1] + 1] = np.arange(P)
    t = sched["tmap"].astype(dt)
    d0, d2, half = dt(0), dt(2), dt(0.5)
    taps = [(dk, dl) for dk in range(-R, R + 1) for dl in range(-R, R + 1) if dk * dk + dl * dl <= R * R and (dk or dl)]
    weights = np.zeros((len(taps), P), dt) if return_weights else None
    order = np.argsort(level, kind="stable")
    bounds = np.searchsorted(level[order], np.arange(1, (int(level.max()) if P else 0) + 2))
    for li in range(len(bounds) - 1):
        idx = order[bounds[li]:bounds[li + 1]]
        I, J, n = yx[idx, 0] + 1, yx[idx, 1] + 1, idx
        kn = lambda y, x: st[y, x] < n                                       # noqa: E731
        ti = t[I, J]
        a, b = kn(I, J + 1), kn(I, J - 1)
        gx = np.where(a, np.where(b, (t[I, J + 1] - t[I, J - 1]) * half, t[I, J + 1] - ti), np.where(b, ti - t[I, J - 1], d0))
        a, b = kn(I + 1, J), kn(I - 1, J)
        gy = np.where(a, np.where(b, (t[I + 1, J] - t[I - 1, J]) * half, t[I + 1, J] - ti), np.where(b, ti - t[I - 1, J], d0))
        Ia = np.zeros((len(I), 3), dt); Jx = np.zeros_like(Ia); Jy = np.zeros_like(Ia); s = np.zeros(len(I), dt)
        for ti_, (dk, dl) in enumerate(taps):
            K, Lc = I + dk, J + dl
            ok = (K > 0) & (K < rows - 1) & (Lc > 0) & (Lc < cols - 1)
            Kc, Lcc = np.clip(K, 1, rows - 2), np.clip(Lc, 1, cols - 2)
            ok &= kn(Kc, Lcc)
            if not ok.any():
                continue
            ry, rx = dt(-dk), dt(-dl)
            vl = np.sqrt(dt(rx * rx + ry * ry))
            dst = dt(1.0 / (float(vl) * math.sqrt(float(vl))))
            lv = (1.0 / (1.0 + np.abs((t[Kc, Lcc] - ti).astype(np.float64)))).astype(dt)
            dr = rx * gx + ry * gy
            dr = np.where(np.abs(dr.astype(np.float64)) <= 0.01, dt(0.000001), dr)
            w = np.where(ok, np.abs(dst * lv * dr), d0)
            if return_weights:
                weights[ti_, idx] = w
            km = Kc - 1 + (Kc == 1); kp = Kc - 1 - (Kc == rows - 2)
            lm = Lcc - 1 + (Lcc == 1); lp = Lcc - 1 - (Lcc == cols - 2)
            px = lambda y, x: out[y, x].astype(dt)                           # noqa: E731
            a, b = kn(Kc, Lcc + 1)[:, None], kn(Kc, Lcc - 1)[:, None]
            gix = np.where(a, np.where(b, (px(km, lp + 1) - px(km, lm - 1)) * d2, px(km, lp + 1) - px(km, lm)),
                           np.where(b, px(km, lp) - px(km, lm - 1), d0))
            a, b = kn(Kc + 1, Lcc)[:, None], kn(Kc - 1, Lcc)[:, None]
            giy = np.where(a, np.where(b, (px(kp + 1, lm) - px(km - 1, lm)) * d2, px(kp + 1, lm) - px(km, lm)),
                           np.where(b, px(kp, lm) - px(km - 1, lm), d0))
            # a tap that does not count has w = 0: x + 0 * y == x exactly, so it is the serial sum without that tap
            Ia = Ia + w[:, None] * px(km, lm)
            Jx = Jx - w[:, None] * (gix * rx)
            Jy = Jy - w[:, None] * (giy * ry)
            s = s + w
        sat = Ia / s[:, None] + (Jx + Jy) / (np.sqrt(Jx * Jx + Jy * Jy) + dt(1.0e-20)) + half
        out[I - 1, J - 1] = saturate_u8(sat)
    return (out, weights) if return_weights else out


def plan_schedule(lib, handle, mask, radius=3):
    """the C++ plan behind a vsr_telea handle, read back through the C-ABI and put into fill (step) order"""
    H, W = mask.shape
    P = int(lib.vsr_telea_plan_pixels(handle))
    yx = np.zeros((P, 2), np.int32); step = np.zeros(P, np.int32); T = np.zeros(P, np.float32); level = np.zeros(P, np.int32)
    tmap = np.zeros((H + 2, W + 2), np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)                               # noqa: E731
    assert lib.vsr_telea_plan_read(handle, p(yx), p(step), p(T), p(level)) == 0
    assert lib.vsr_telea_plan_tmap(handle, p(tmap)) == 0
    assert np.array_equal(np.sort(step), np.arange(P)), "steps are not a permutation"
    assert np.all(np.diff(level) >= 0), "the plan's pixels are not sorted by level"
    o = np.argsort(step)
    return dict(H=H, W=W, radius=radius, yx=yx[o], T=T[o], level=level[o], tmap=tmap, mask=mask != 0,
                levels=int(lib.vsr_telea_plan_levels(handle)))


# ---------------------------------------------------------------------------------------------------------------------------
# the mask set and images shared by tests/test_telea_plan.py and tests/test_gpu_telea.py
# ---------------------------------------------------------------------------------------------------------------------------
def mask_cases():
    """name -> uint8 [H,W] mask.  The rectangle cases come from the product's own create_mask (coords xmin, xmax, ymin, ymax,
    each widened by config.subtitleAreaDeviationPixel)."""
    from vsr_amd.backend.tools.inpaint_tools import create_mask

    cases = {}
    cases["rect"] = create_mask((48, 72), [(20, 50, 20, 26)])
    cases["two_overlapping"] = create_mask((60, 80), [(15, 60, 18, 24), (30, 68, 30, 40)])
    cases["edge_and_corner"] = create_mask((50, 70), [(0, 12, 20, 28), (55, 69, 44, 49)])      # left edge; bottom-right corner
    hole = create_mask((52, 76), [(16, 58, 18, 32)])
    hole[22:27, 30:36] = 0                                                                      # a known island inside
    cases["hole"] = hole
    line = np.zeros((40, 56), np.uint8)
    line[20, 5:50] = 255
    line[5:35, 30] = 255                                                                        # 1-pixel lines, crossing
    cases["line"] = line
    odd = np.zeros((37, 53), np.uint8)
    odd[8:19, 6:40] = 3                                                                         # non-255 nonzero values
    odd[15:30, 31:47] = 200
    cases["non255"] = odd
    cases["whole_frame"] = np.full((12, 17), 255, np.uint8)                                     # no band: nothing scheduled
    cases["empty"] = np.zeros((12, 17), np.uint8)
    portrait = create_mask((71, 39), [(12, 25, 40, 52)])
    portrait[0:4, 20:39] = 255                                                                  # top edge, into the top-right corner
    cases["portrait_odd"] = portrait
    return cases


def random_image(H, W, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def smooth_image(H, W, seed=1):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    img = np.stack([127 + 90 * np.sin(xx / 37. * (H / 1080. + 1) + c) + 30 * np.cos(yy / 11. * (c + 1)) for c in range(3)], -1)
    return np.clip(img + rng.normal(0, 4, (H, W, 3)), 0, 255).astype(np.uint8)


def benchmark_mask(H=1080, W=1920):
    """the benchmark's subtitle box (950, 1069, 288, 1632) (ymin, ymax, xmin, xmax) widened by create_mask's margin, plus a
    second, overlapping line above it -- scaled from 1080p"""
    from vsr_amd.backend.tools.inpaint_tools import create_mask

    s = H / 1080.
    boxes = [(950, 1069, 288, 1632), (880, 960, 500, 1400)]
    return create_mask((H, W), [(int(x0 * s), int(x1 * s), int(y0 * s), int(y1 * s)) for y0, y1, x0, x1 in boxes])


_serial_cache = {}


def serial_case(name, kind, dt=np.float32):
    """(img, mask, out, schedule) of the serial statement on a case of mask_cases() with a random or smooth image; cached"""
    key = (name, kind, np.dtype(dt).name)
    if key not in _serial_cache:
        mask = mask_cases()[name]
        img = (random_image if kind == "random" else smooth_image)(*mask.shape, seed=len(name))
        _serial_cache[key] = (img, mask) + serial(img, mask, 3, dt)
    return _serial_cache[key]
