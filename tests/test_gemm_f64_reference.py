"""The float64 gather-GEMM reference (tests/_gemm_f64.py) held against the fp32 replay of the descriptor the suite already trusts
(_replay.gemm_reference), its split-format helpers against a round trip, and its fp32 yardstick against the derived worst-case bound.
No GPU: this is the yardstick of tests/test_gpu_gemm_family.py, checked on its own."""
import numpy as np
import pytest

import _gemm_f64 as g64
from test_gpu_kernels import _make_gemm_case, _reference, _to_split_inplace, _written_mask

# (M, N, K, bm, bn, bmode, splitK, bias, act, residual, alpha)
CASES = [
    (300, 200, 96, 128, 128, 0, 1, True, 1, True, 0.5),
    (129, 65, 64, 128, 64, 0, 1, False, 0, False, 1.0),
    (60, 60, 640, 128, 128, 0, 4, False, 0, False, 1.0),          # split-K planes
    (140, 140, 480, 128, 128, 0, 2, False, 0, False, 1.0),         # odd slices: 8 + 7 chunks
    (200, 192, 96, 128, 128, 1, 1, False, 0, False, 1.0),          # KN
    (130, 100, 352, 128, 64, 1, 1, True, 3, True, 0.75),           # KN with an epilogue
    (150, 70, 2304, 256, 64, 0, 1, True, 2, True, 1.0),
] + [(90, 75, 160, 128, 64, 0, 1, True, act | g64.ACT_POST_RELU, True, 1.0) for act in (0, 1, 2, 3)]
IDS = [f"{c[0]}x{c[1]}x{c[2]}-mode{c[5]}-split{c[6]}-act{c[8]:#x}" for c in CASES]
_cache = {}


def _case(i):
    if i not in _cache:
        M, N, K, bm, bn, bmode, splitK, bias, act, res, alpha = CASES[i]
        c = _make_gemm_case(np.random.default_rng(100 + i), M, N, K, bm, bn, bmode, splitK, bias, act, res, alpha)
        _cache[i] = (c, {})
    return _cache[i]


def _ref64(i, variant):
    c, refs = _case(i)
    if variant not in refs:
        refs[variant] = g64.reference64(c, g64.operand_model(variant))
    return c, refs[variant]


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_reference64_agrees_with_the_fp32_replay(i):
    """the fp32 model in float64 and torch's fp32 evaluation of the same descriptor: the same cells, apart by no more than an fp32
    evaluation may be (the derived bound on every cell; twice the yardstick's own error on its rows)"""
    c, r = _ref64(i, 3)
    replay = _reference(c)
    assert np.array_equal(np.sort(r.cells.reshape(-1)), np.flatnonzero(_written_mask(c)))
    assert np.all(replay[~_written_mask(c)] == g64.SENTINEL)
    err = np.abs(replay[r.cells].astype(np.float64) - r.ref)
    assert np.all(err <= g64.bound(r)), f"replay beyond the derived bound by {np.max(err / g64.bound(r)):.2f}x"
    rows = g64.yardstick_rows(c)
    yerr = np.abs(g64.yardstick32(c, g64.operand_model(3), rows).astype(np.float64) - r.ref[:, rows])
    assert rows.size * c.N >= min(4096, c.M * c.N)
    assert err[:, rows].max() <= 2 * yerr.max()
    assert np.sqrt(np.mean(err[:, rows] ** 2)) <= 2 * np.sqrt(np.mean(yerr ** 2))
    assert err.max() > 0          # two evaluations, not one compared with itself


@pytest.mark.parametrize("variant", [3, 4, 6])
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_yardstick_stays_inside_the_derived_bound(i, variant):
    """acc = fl(acc + fl(a_k b_k)) one product at a time is the longest chain of roundings a correct fp32 kernel can have:
    (K + 4) 2^-24 S bounds it on every operand model"""
    c, r = _ref64(i, variant)
    rows = g64.yardstick_rows(c)
    y = g64.yardstick32(c, g64.operand_model(variant), rows)
    assert y.dtype == np.float32 and y.shape == r.ref[:, rows].shape
    err = np.abs(y.astype(np.float64) - r.ref[:, rows])
    b = g64.bound(r)[:, rows]
    assert np.all(err <= b), f"yardstick beyond the bound by {np.max(err / b):.2f}x"
    assert err.max() > 0


def test_operand_models_differ_as_documented():
    """the split-half model drops lo.lo: it differs from the exact product, and the fp16 model from both, by what the formats say"""
    c, r32 = _ref64(0, 3)
    _, r22 = _ref64(0, 4)
    _, r11 = _ref64(0, 6)
    d22, d11 = np.abs(r22.ref - r32.ref), np.abs(r11.ref - r32.ref)
    assert 0 < d22.max() <= 2.0 ** -20 * r32.S.max()           # 2 * 2^-22 per product (the lo halves' own rounding) + 2^-22 (lo.lo)
    assert d22.max() < d11.max() <= 2.0 ** -10 * r32.S.max()   # two fp16 roundings per product
    with pytest.raises(ValueError):
        g64.operand_model(9)
    assert g64.operand_model(5).split_tensors and g64.operand_model(6).split_tensors
    assert not g64.operand_model(4).split_tensors and not g64.operand_model(7).split_tensors
    assert g64.operand_model("narrow").kind == g64.operand_model(1).kind == "fp32"


def test_split_format_round_trip():
    rng = np.random.default_rng(11)
    x = (rng.standard_normal(32 * 64) * np.exp(rng.uniform(-4, 6, 32 * 64))).astype(np.float32)
    buf, old = x.copy(), x.copy()
    starts = np.arange(0, x.size, 64)                     # every other chunk
    g64.to_split_inplace(buf, starts)
    _to_split_inplace(old, starts)
    assert np.array_equal(buf.view(np.uint32), old.view(np.uint32))          # the layout the suite's other tests write
    cells = (starts[:, None] + np.arange(32)[None, :]).reshape(-1)
    hi, lo = g64.split_halves(x[cells])
    back = g64.from_split(buf, cells)
    assert np.array_equal(back, hi.astype(np.float64) + lo.astype(np.float64))
    assert np.all(np.abs(back - x[cells]) <= 2.0 ** -22 * np.abs(x[cells]) + 2.0 ** -25)   # lo may be an fp16 subnormal
    other = np.setdiff1d(np.arange(x.size), cells)
    assert np.array_equal(buf[other].view(np.uint32), x[other].view(np.uint32))
    hi_i, lo_i = g64.split_positions(cells)
    assert np.array_equal(np.sort(np.concatenate([hi_i, lo_i])), np.sort(np.concatenate([2 * cells, 2 * cells + 1])))


@pytest.mark.parametrize("bm,bn,bmode", [(128, 128, 1), (128, 64, 1), (256, 32, 0), (256, 64, 0), (128, 128, 0)],
                         ids=["128x128-KN", "128x64-KN", "256x32-NK", "256x64-NK", "128x128-NK"])
def test_make_case_on_every_tile_and_layout_the_gpu_tests_use(bm, bn, bmode):
    """make_case / physical / reference64 at the epilogue matrix's shape (M = 2 bm + 44, N = 2 bn + 8, K = 96) on the tiles and
    layouts tests/test_gpu_gemm_family.py launches: the written cells are the descriptor's, the float64 reference agrees with the
    fp32 replay inside the derived bound, every table entry -- the padded rows a tile reads but never stores included -- addresses
    32 floats inside its buffer, and the split-format image holds hi / lo halves in exactly the chunks the tables address (KN: the K
    rows of B times the n chunks)."""
    rng = np.random.default_rng(bm + bn + bmode)
    M, N, K = 2 * bm + 44, 2 * bn + 8, 96
    c = g64.make_case(rng, M, N, K, bm, bn, bmode, bias=True, act=1, residual=True)
    assert (c.tilesM, c.tilesN) == (3, 3) and len(c.rowA) == len(c.rowC) == len(c.rowR) == 3 * bm and len(c.colC) == 3 * bn // 32
    assert len(c.rowB) == (K if bmode else 3 * bn) and len(c.colB) == (3 * bn // 32 if bmode else K // 32)
    for rows, cols, buf in ((c.rowA, c.colA, c.Abuf), (c.rowB, c.colB, c.Bbuf), (c.rowC, c.colC, c.Cbuf), (c.rowR, c.colC, c.Rbuf)):
        assert rows.min() >= 0 and cols.min() >= 0 and rows.max() + cols.max() + 32 <= buf.size
        assert np.all(rows % 4 == 0) and np.all(cols % 32 == 0)
    r = g64.reference64(c, g64.operand_model(3))
    assert np.array_equal(np.sort(r.cells.reshape(-1)), np.flatnonzero(_written_mask(c)))
    replay = _reference(c)
    err = np.abs(replay[r.cells].astype(np.float64) - r.ref)
    assert np.all(err <= g64.bound(r)) and err.max() > 0
    p = g64.physical(c, g64.operand_model(5))
    for buf, orig, rows, cols in ((p.A, c.Abuf, c.rowA, c.colA), (p.B, c.Bbuf, c.rowB, c.colB), (p.R, c.Rbuf, c.rowR[:M], c.colC)):
        starts = np.unique(g64.chunk_starts(rows, cols))
        cells = (starts[:, None] + np.arange(32)[None, :]).reshape(-1)
        hi, lo = g64.split_halves(orig[cells])
        h16 = buf.view(np.uint16)[(2 * starts[:, None] + np.arange(64)[None, :])]         # a chunk: 32 hi halves, then 32 lo halves
        assert np.array_equal(h16[:, :32].reshape(-1), hi.view(np.uint16)) and np.array_equal(h16[:, 32:].reshape(-1), lo.view(np.uint16))
        other = np.setdiff1d(np.arange(orig.size), cells)
        assert np.array_equal(buf[other].view(np.uint32), orig[other].view(np.uint32))
    poisoned = g64.make_case(np.random.default_rng(bm + bn + bmode), M, N, K, bm, bn, bmode, bias=True, act=1, residual=True, poison=True)
    assert np.all(poisoned.Abuf[poisoned.rowA[M:, None] + poisoned.colA[None, :]] == 1e6) and np.array_equal(poisoned.rowA[:M], c.rowA[:M])
    assert poisoned.rowA.max() + poisoned.colA.max() + 32 <= poisoned.Abuf.size
    assert np.array_equal(g64.reference64(poisoned, g64.operand_model(3)).ref, r.ref)


def test_physical_buffers_and_footprint_helpers():
    """physical() writes split format exactly where a split-format variant reads it; untouched() sees one stray uint16"""
    rng = np.random.default_rng(12)
    c = g64.make_case(rng, 70, 40, 64, 128, 64, 0, bias=True, act=1 | g64.ACT_OUT_SPLIT, inplace=True)
    assert np.array_equal(g64.physical(c, g64.operand_model(4)).A, c.Abuf)
    p = g64.physical(c, g64.operand_model(5))
    assert p.A is not c.Abuf and p.C is not c.Cbuf and not np.array_equal(p.A.view(np.uint32), c.Abuf.view(np.uint32))
    r = g64.reference64(c, g64.operand_model(5))
    res = g64.from_split(p.C, r.cells[0])                  # the in-place residual, as the kernel reads it
    hi, lo = g64.split_halves(c.Cbuf[r.cells[0]])
    assert np.array_equal(res, hi.astype(np.float64) + lo.astype(np.float64))
    got = p.C.copy()
    assert g64.untouched(c, got, p.C, r.cells)
    stray = got.view(np.uint16)
    pos = 2 * int(c.rowC[0] + c.colC[1]) + 32 + 9          # lo half of column 41 >= N
    stray[pos] ^= 1
    assert not g64.untouched(c, got, p.C, r.cells)
    odd = g64.make_case(rng, 256, 128, 32, 128, 64, 0, odd=True)
    assert odd.baseC == 1 and np.all(odd.rowC % 2 == 1) and np.all(odd.rowR % 2 == 1) and np.all(odd.colC % 32 == 0)
