"""CPU tests of tests/_sttn_ew_ref.py (the references and input builders of tests/test_gpu_sttn_elementwise.py) and of the launcher
prototypes that file binds.  No GPU."""
import ctypes as C

import numpy as np
import torch
import torch.nn.functional as F

import _sttn_ew_ref as R
from oracle import cv2_restate as cv2r


def test_launcher_prototypes_match_headers(built_lib):
    """every launcher the GPU file binds is declared in csrc/elementwise.h or include/vsr_hip.h with the bound argument kinds and is
    exported by the built library: a changed signature fails here, not as a launch with shifted arguments"""
    decl = R.header_prototypes(set(R.PROTOTYPES))
    missing = sorted(set(R.PROTOTYPES) - set(decl))
    assert not missing, f"bound but declared in neither header: {missing}"
    lib = C.CDLL(built_lib.LIB_PATH)
    for name, sig in R.PROTOTYPES.items():
        assert hasattr(lib, name), f"{name} is not exported by libvsr_hip.so"
        assert sig == decl[name], f"{name}: ctypes prototype {sig} != header {decl[name]}"
    # the parser on declarations whose kinds are known by heart
    internal = R.header_prototypes({"vsr_launch_softmax_dev", "vsr_launch_decode_out_blk", "vsr_launch_upsample2x_fmt"})
    assert internal == {"vsr_launch_softmax_dev": "piip", "vsr_launch_decode_out_blk": "piiipppppip", "vsr_launch_upsample2x_fmt": "piiiipiiip"}


def test_decode_inputs_stay_off_the_truncation_boundaries():
    """the input condition of the bit-exact decode test: every unsaturated input's float64 value lies at least 1/128 from an integer,
    saturated inputs give exactly 0 and 255 in both precisions, all 256 levels occur, and numpy's fp32 evaluation truncates to the
    same level everywhere"""
    rng = np.random.default_rng(31)
    s = R.decode_inputs(rng, (400_000,))
    assert s.dtype == np.float32
    v = R.decode_value64(s)
    sat = np.abs(s) >= 20
    assert 0.03 < sat.mean() < 0.1
    assert set(np.unique(v[sat])) == {0.0, 255.0}
    dist = np.abs(v[~sat] - np.rint(v[~sat]))
    print(f"smallest distance to an integer: {dist.min():.4f}")
    assert dist.min() >= 1.0 / 128
    lv = R.decode_levels(s)
    assert np.array_equal(np.unique(lv), np.arange(256))
    assert np.array_equal(np.unique(R.decode_levels(s[:257])), np.arange(256)), "the first 257 values run through every level"
    t32 = np.tanh(s)
    assert t32.dtype == np.float32
    v32 = (t32 + np.float32(1.0)) / np.float32(2.0) * np.float32(255.0)
    assert v32.dtype == np.float32
    print(f"fp32 evaluation vs float64: {np.abs(v32.astype(np.float64) - v).max():.2e}")
    assert np.abs(v32.astype(np.float64) - v).max() < 1e-4
    assert np.array_equal(v32.astype(np.uint8), lv)
    assert np.all(np.tanh(np.float32([20.0, -20.0])) == np.float32([1.0, -1.0]))
    small = R.decode_inputs(np.random.default_rng(1), (3, 8, 3))         # fewer than 257 values
    assert small.shape == (3, 8, 3) and np.abs(R.decode_value64(small) - np.rint(R.decode_value64(small)))[np.abs(small) < 20].min() >= 1.0 / 128


def test_decode_layouts_and_reference():
    rng = np.random.default_rng(32)
    n, rows, W = 2, 4, 8
    s = rng.standard_normal((n, rows * W, 3)).astype(np.float32)
    y = R.to_blocked(s, rows, W, 40, 9.0)
    assert y.shape == (n * rows * W // 8, 40) and np.all(y[:, 24:] == 9.0)
    for f, yy, xx, ch in [(0, 0, 0, 0), (1, 3, 7, 2), (0, 1, 4, 1), (1, 2, 3, 0)]:      # the layout by its definition, cell by cell
        row = f * (rows * W // 8) + (yy // 2) * (W // 4) + xx // 4
        assert y[row, (yy % 2) * 12 + (xx % 4) * 3 + ch] == s[f, yy * W + xx, ch]
    p = R.to_plain(s, 5, 9.0)
    assert np.array_equal(p[:, :3], s.reshape(-1, 3)) and np.all(p[:, 3:] == 9.0)
    # the reference on values whose levels are known
    s2 = np.zeros((2, 4, 3), np.float32)
    s2[0] = 30.0                      # level 255
    s2[1] = -30.0                     # level 0
    comp0 = np.full((3, 4, 3), 100.0, np.float32)
    in_bgr = np.arange(3 * 4 * 3, dtype=np.uint8).reshape(3, 4, 3)
    mask = np.zeros((3, 4), np.uint8)
    mask[2, 1:] = (1, 128, 255)
    got = R.decode_ref(s2, comp0, [2, 0], [1, 0], 1, 2, in_bgr, mask)
    assert np.all(got[1] == 100.0) and np.all(got[:, 0] == 100.0) and np.all(got[:, 3] == 100.0)       # frame 1, pixels 0 and 3 untouched
    assert np.all(got[2, 1:3] == 255.0)                                                        # first visit, mask non-zero
    assert np.array_equal(got[0, 1:3], 50.0 + 0.5 * in_bgr[0, 1:3, ::-1])                      # average with the swapped input (mask 0)
    outs = R.decode_outcomes(np.float64(100.0), np.float64(0.0), False, np.float64(255.0), True)
    assert sorted(float(o) for o in outs) == [50.0, 127.5, 255.0, 255.0]


def test_upsample_reference_and_bound():
    """align_corners: the corners are copied, the row between two source rows of a 2-row image is their 1/3 : 2/3 mix; torch's own
    fp32 path stays inside the bound for the GPU file's shapes and for 30 x 160"""
    x = np.zeros((1, 2, 1, 4), np.float32)
    x[0, 1] = 3.0
    r = R.upsample_ref(x)
    assert r.shape == (1, 4, 2, 4) and np.allclose(r[0, :, 0, 0], [0.0, 1.0, 2.0, 3.0], atol=1e-15)
    rng = np.random.default_rng(33)
    worst = 0.0
    for H, W, Cc in [(1, 1, 4), (1, 5, 4), (5, 1, 8), (2, 3, 36), (7, 9, 32), (3, 4, 64), (6, 5, 4), (30, 160, 8)]:
        x = rng.standard_normal((2, H, W, Cc)).astype(np.float32)
        ref = R.upsample_ref(x)
        assert np.array_equal(ref[:, 0, 0], x[:, 0, 0]) and np.array_equal(ref[:, -1, -1], x[:, -1, -1])
        t32 = F.interpolate(torch.from_numpy(x).permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=True).permute(0, 2, 3, 1).numpy()
        ratio = np.abs(t32.astype(np.float64) - ref).max() / R.upsample_bound(H, W, np.abs(x).max())
        worst = max(worst, ratio)
    print(f"torch fp32 / bound: {worst:.3f}")
    assert worst <= 0.25
    h = R.with_halo(np.ones((1, 2, 3, 4), np.float32), 2, R.HALO_POISON)
    assert h.shape == (1, 6, 7, 4) and h[0, 1, 3, 0] == R.HALO_POISON and np.all(h[0, 2:4, 2:5] == 1.0)


def test_norm_im2col_reference():
    """the unfold by its definition on single cells, the floor of odd sizes, the fp32 restatement against float64, the premask"""
    rng = np.random.default_rng(34)
    n, ih, iw = 2, 5, 7
    img = rng.integers(0, 256, size=(n, ih, iw, 3), dtype=np.uint8)
    ref = R.norm_im2col_ref(img)
    oh, ow = ih // 2, iw // 2
    assert ref.shape == (n * oh * ow, 32) and np.all(ref[:, 27:] == 0)
    for f, oy, ox, ky, kx, c in [(0, 0, 0, 0, 0, 0), (0, 0, 0, 1, 1, 2), (1, 1, 2, 2, 2, 1), (1, 1, 0, 1, 0, 0), (0, 1, 1, 0, 2, 2)]:
        y, x = 2 * oy - 1 + ky, 2 * ox - 1 + kx
        want = 0.0 if (y < 0 or x < 0) else img[f, y, x, 2 - c] / 255.0 * 2.0 - 1.0
        assert abs(ref[(f * oh + oy) * ow + ox, (ky * 3 + kx) * 3 + c] - want) < 1e-15
    assert 2 * (oh - 1) + 1 < ih - 1 and 2 * (ow - 1) + 1 < iw - 1, "the last row and column are read by no patch"
    r32 = R.norm_im2col_ref(img, dtype=np.float32)
    assert r32.dtype == np.float32 and np.abs(r32.astype(np.float64) - ref).max() <= 3 * R.U32
    mask = rng.choice(np.array([0, 127, 128, 255], np.uint8), size=(n, ih, iw))
    rm = R.norm_im2col_ref(img, mask)
    f, oy, ox, ky, kx = 1, 1, 1, 1, 1
    y, x = 2 * oy, 2 * ox
    cell = rm[(f * oh + oy) * ow + ox, (ky * 3 + kx) * 3:(ky * 3 + kx) * 3 + 3]
    assert np.all(cell == 0) if mask[f, y, x] >= 128 else np.array_equal(cell, ref[(f * oh + oy) * ow + ox, 12:15])
    keep = R.norm_im2col_ref(np.full_like(img, 255), mask)             # 1 where a kept pixel is read, 0 for masked pixels and padding
    assert set(np.unique(keep)) == {0.0, 1.0} and np.array_equal(rm, ref * keep)


def test_split_term_and_the_normalised_levels():
    """The 256 values (u / 255) * 2 - 1 in split format lie within 2^-22 relative of the fp32 value, with no subnormal floor: the
    last subtraction is exact and leaves a multiple of 2^-24, so below 1/8, where the lo half is an fp16 subnormal (a multiple of
    2^-24 itself), hi + lo is the value.  General values need the floor of split_term."""
    v = R.norm_im2col_ref(np.arange(256, dtype=np.uint8).repeat(3).reshape(1, 16, 16, 3), dtype=np.float32)
    v = np.unique(v[v != 0])               # zero is the padding only: no level maps to it
    assert v.size == 256
    hi, lo = R.split_halves(v)
    err = np.abs(hi.astype(np.float64) + lo.astype(np.float64) - v.astype(np.float64))
    assert np.all(err <= 2.0 ** -22 * np.abs(v))
    assert np.all(err[np.abs(v) < 0.125] == 0)
    x = R.to_split_values(np.random.default_rng(3), 64)
    ok = (np.abs(x) <= 65504) & ((np.abs(x) >= 2.0 ** -14) | (x == 0))
    hi, lo = R.split_halves(x)
    with np.errstate(invalid="ignore"):
        e = np.abs(hi.astype(np.float64) + lo.astype(np.float64) - x.astype(np.float64))
    assert np.all(e[ok] <= R.split_term(x[ok]))
    assert np.isinf(hi[np.abs(x) > 65520]).all() and (np.abs(x) > 65520).sum() >= 3 and ((x != 0) & (np.abs(x) < 2.0 ** -14)).sum() >= 4


def test_split_helpers_round_trip():
    rng = np.random.default_rng(35)
    x = rng.standard_normal(96).astype(np.float32)
    buf = R.to_split_whole(x.copy())
    cells = np.array([[0, 5, 31], [32, 64, 95]])
    assert np.all(np.abs(R.split_decode(buf, cells) - x[cells]) <= R.split_term(x[cells]))
    other = buf.copy()
    other.view(np.uint16)[2 * 32 + 7] ^= 1                   # hi half of cell 39
    assert R.split_untouched(buf, buf, cells) and not R.split_untouched(other, buf, cells)
    assert R.split_untouched(other, buf, np.array([39]))
    other.view(np.uint16)[2 * 32 + 32 + 7] ^= 1              # its lo half
    assert R.split_untouched(other, buf, np.array([39])) and not R.split_untouched(other, buf, np.array([38]))


def test_reduce_scatter_reference_and_lsum_planes():
    rng = np.random.default_rng(36)
    for ns, M in [(1, 1), (2, 5), (5, 5), (2, 4100)]:
        l = R.lsum_planes(rng, ns, M, M + 3)
        assert l.shape == (ns, M + 3) and np.all(l[:, M:] == 1e30) and np.all(l[:, :M] > 0)
        exact = l[:, :M].astype(np.float64).sum(0)
        acc = l[0, :M].copy()
        for s in range(1, ns):
            acc = acc + l[s, :M]
        assert acc.dtype == np.float32 and np.array_equal(acc.astype(np.float64), exact), "the fp32 sum of the row sums is exact"
        if M > 1:
            assert exact.min() < 4e-3 and exact.max() > 2.5e2
        if ns > 1:
            assert (l[:, :M].astype(np.float64) / exact).min() > 0.1
    part = rng.standard_normal((3, 4, 32)).astype(np.float32)
    l = R.lsum_planes(rng, 3, 4, 6)
    ref, mag = R.reduce_scatter_ref(part, l[:, :4])
    assert np.allclose(ref, part.astype(np.float64).sum(0) / l[:, :4].astype(np.float64).sum(0)[:, None], rtol=1e-15) and np.all(mag >= np.abs(ref))
    b = R.reduce_scatter_bound(ref, mag, 3, True, False)
    assert np.all(b >= 3 * R.U32 * np.abs(ref)) and np.all(b <= 5 * R.U32 * mag * (1 + 1e-12))
    assert np.all(R.reduce_scatter_bound(ref, mag, 1, False, False) == 0)        # one plane, no divisor: a copy
    cells = R.scatter_cells([64, 0], [32, 0], 64)
    assert cells.shape == (2, 64) and cells[0, 0] == 96 and cells[0, 31] == 127 and cells[0, 32] == 64 and cells[1, 33] == 1


def test_lib_tables_and_blend_reference(built_lib):
    """vsr_cv2_linear_tables at the GPU file's sizes equals the oracle's tables; blend_ref writes the whole strip without a mask
    and nothing where the mask is 0"""
    lib = C.CDLL(built_lib.LIB_PATH)
    lib.vsr_cv2_linear_tables.restype = C.c_int
    lib.vsr_cv2_linear_tables.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    for ssize, dsize, clamp in [(3, 2, 1), (2, 1, 0), (7, 3, 1), (5, 2, 0), (5, 13, 1), (3, 7, 0), (6, 6, 1), (4, 4, 0), (6, 13, 1), (4, 7, 0),
                                (4, 4, 1), (2, 2, 0), (37, 1031, 1), (29, 1021, 0)]:
        ofs, ic, fc = R.lib_tables(lib, ssize, dsize, clamp)
        o2, i2, f2 = cv2r.linear_tables(ssize, dsize, bool(clamp))
        assert np.array_equal(ofs, o2) and np.array_equal(ic, i2.reshape(-1)) and np.array_equal(fc, f2.reshape(-1)), (ssize, dsize, clamp)
    rng = np.random.default_rng(37)
    strip = rng.integers(0, 256, size=(7, 13, 3), dtype=np.uint8)
    comp = rng.integers(0, 256, size=(4, 6, 3)).astype(np.float32)
    full = R.blend_ref(strip, comp, False, None)
    assert np.array_equal(full, cv2r.resize_linear(comp.astype(np.uint8), (13, 7))[:, :, ::-1])
    mask = np.zeros((7, 13), np.uint8)
    mask[2:4, 5:9] = 1
    part = R.blend_ref(strip, comp, False, mask)
    assert np.array_equal(part[mask == 0], strip[mask == 0]) and np.array_equal(part[mask == 1], full[mask == 1])
    compf = comp * np.float32(0.5) + np.float32(0.25)
    fl = R.blend_ref(strip, compf, True, None)
    assert np.array_equal(fl, cv2r.resize_linear(compf, (13, 7)).astype(np.uint8)[:, :, ::-1])


def test_kn_to_nk_reference():
    rng = np.random.default_rng(38)
    K = N = 32
    src = rng.integers(0, 2 ** 16, size=2 * 32 * 40, dtype=np.uint16)
    rowB = (rng.permutation(K + 3)[:K] * 32).astype(np.int64)
    want = R.kn_to_nk_ref(src, rowB, np.array([0]), K, N, 96, np.zeros(2 * N * 96, np.uint16))
    k, n = 5, 9
    assert want[2 * (n * 96) + k] == src[2 * rowB[k] + n] and want[2 * (n * 96) + 32 + k] == src[2 * rowB[k] + 32 + n]
    assert not want.reshape(N, 192)[:, 64:].any()
