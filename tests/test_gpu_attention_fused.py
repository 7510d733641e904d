"""The two kernels of the fused attention one launch at a time against float64 (tests/_attn_f64.py): the row maxima the score GEMM
leaves (VSR_ACT_ROW_MAX, gather_gemm_v3.h), the P.V GEMM that exponentiates its scores (VSR_ACT_A_EXP, gather_gemm_pvx.h), the chain
score GEMM -> P.V -> reduce against softmax(Q K^T / sqrt(D)) V at a readable size, and the refusals of the kernel-level entry points.

Conventions (tests/test_gpu_gemm_family.py, tests/test_gpu_sttn_elementwise.py): one launch per case; C, the row-maximum array and
the row-sum array are pre-filled and compared WHOLE; the inputs of a launch stay alive until after the synchronisation (_Launch.keep,
Side); no launch leaves its kernel's contract.  Every bound is derived beside its assertion or in _attn_f64 / _gemm_f64, before
anything was measured; the `RATIO` and `HANDOVER` lines are kept in profiles/attention_f64_ratios.md.

tests/test_attn_f64_reference.py checks the reference, the bound and the descriptor mirror without a GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

import _attn_f64 as a64
import _gemm_f64 as g64
import _sttn_ew_ref as R
from test_gpu_gemm_family import TILES, _Launch, _check, _same_bytes

pytestmark = pytest.mark.gpu

ROW_MAX, A_EXP, V_AEXP = a64.ACT_ROW_MAX, a64.ACT_A_EXP, 1 | a64.VARIANT_A_EXP
U32 = g64.U32
SENT_U32 = np.uint32(0xA5A5A5A5)            # pre-fill of the cells of a row-maximum array that no row owns
TAIL = 8                                    # cells behind the last tile's rows in every side array
WAVES_N = {"128x64": 2, "128x128": 2, "256x64": 1, "256x32": 1}


# ---- side arrays and launching ------------------------------------------------------------------------------------------------------
class Side:
    """a row-maximum (uint32) or row-sum (fp32) array on the device with the bytes it held before the launch"""

    def __init__(self, device, before):
        self.before = np.ascontiguousarray(before)
        self.t = torch.from_numpy(self.before.view(np.int32 if self.before.dtype == np.uint32 else np.float32).copy()).to(device)

    def ptr(self):
        return self.t.data_ptr()

    def get(self):
        torch.cuda.synchronize()
        return self.t.cpu().numpy().view(self.before.dtype)

    def reset(self):
        self.t.copy_(torch.from_numpy(self.before.view(np.int32 if self.before.dtype == np.uint32 else np.float32).copy()))
        torch.cuda.synchronize()


def _rowmax_side(device, c, bm, prefill=None):
    """tilesM * bm + TAIL cells: rows m < M hold `prefill` (default 0, the engine's memset), the rest SENT_U32"""
    a = np.full(c.tilesM * bm + TAIL, SENT_U32, np.uint32)
    a[:c.M] = 0 if prefill is None else prefill
    return Side(device, a)


def _attach_rowmax(L, i, side):
    L.probs[i].R, L.probs[i].rowR = side.ptr(), None
    L.probs[i].act = L.cases[i].act | ROW_MAX


def _detach_rowmax(L, i):
    L.probs[i].R = L.probs[i].rowR = None
    L.probs[i].act = L.cases[i].act & ~ROW_MAX


def _check_rowmax(c, got, side, what, prefill=None):
    """the array holds ordered(max of the STORED row) for m < M -- or the pre-fill where that is larger -- bit for bit, and its
    pre-fill everywhere else"""
    after = side.get()
    want = a64.ordered(a64.rowmax_ref(c, got))
    if prefill is not None:
        want = np.maximum(want, prefill)
    bad = np.flatnonzero(after[:c.M] != want)
    assert bad.size == 0, (f"{what}: {bad.size} row maxima differ, first at row {bad[0]}: got {a64.from_ordered(after[bad[:1]])[0]!r} "
                           f"want {a64.from_ordered(want[bad[:1]])[0]!r}")
    assert np.array_equal(after[c.M:], side.before[c.M:]), f"{what}: cells of rows m >= M or the tail of the array were written"


# =====================================================================================================================================
# 2. VSR_ACT_ROW_MAX
# =====================================================================================================================================
def _poison30(c):
    """the table rows m >= M of A and n >= N of B point at operand rows of 1e30 (make_case(poison=True) put 1e6 there)"""
    assert c.M < len(c.rowA) and c.N < len(c.rowB)
    c.Abuf[c.rowA[c.M]:] = 1e30
    c.Bbuf[c.rowB[c.N]:] = 1e30
    assert np.all(c.rowA[:c.M] < c.rowA[c.M]) and np.all(c.rowB[:c.N] < c.rowB[c.N])


def _planted_case(rng, bm, bn, alpha=1.0, bias=False, cols=None, offsets=None, zero_rows=()):
    """M = 2 bm - 37, N = 2 bn + 8, K = 64.  Row m of alpha A B^T peaks at column cols[m] (default 37 m mod N): operand column 0 is a
    constant (B) times a per-row offset (A), columns 1 .. 62 are cos / sin of 31 frequencies of the column angle -- the product is
    the Dirichlet kernel D31(theta_c - theta_n): 31 at n = c, at most 31 - 2.9 one column away (N <= 264), below 8 elsewhere --,
    every operand carries noise of 2e-3.  zero_rows: A rows of zeros but for the offset."""
    M, N, K = 2 * bm - 37, 2 * bn + 8, 64
    c = g64.make_case(rng, M, N, K, bm, bn, 0, bias=bias, act=0, residual=False, alpha=alpha, poison=True)
    _poison30(c)
    cols = (37 * np.arange(M)) % N if cols is None else np.asarray(cols)
    f = np.arange(1, 32)[None, :]

    def feats(idx):
        th = 2 * np.pi * np.asarray(idx)[:, None] / N
        out = np.zeros((len(idx), K))
        out[:, 1:63:2], out[:, 2:63:2] = np.cos(f * th), np.sin(f * th)
        return out

    A, B = feats(cols), feats(np.arange(N))
    A += 2e-3 * rng.standard_normal(A.shape)
    B += 2e-3 * rng.standard_normal(B.shape)
    if alpha < 0:
        A = -A
    B[:, 0] = 1.0
    A[:, 0] = 0.0 if offsets is None else offsets
    for m in zero_rows:
        A[m, 1:] = 0.0
    from _replay import _scatter

    _scatter(c.Abuf, 0, c.rowA[:M], c.colA, K, A.astype(np.float32))
    _scatter(c.Bbuf, 0, c.rowB[:N], c.colB, K, B.astype(np.float32))
    c.cols = cols
    return c


_planted = {}


def _planted_cases(bm, bn):
    """four problems of one launch: plain (with an all-negative row, an all-equal row, maxima in column N - 1), with a bias,
    alpha < 0, alpha < 0 with a bias whose row 5 has -0.0 as its maximum"""
    if (bm, bn) not in _planted:
        rng = np.random.default_rng(20 + bm + bn)
        M, N = 2 * bm - 37, 2 * bn + 8
        cols = (37 * np.arange(M)) % N
        cols[11] = cols[M - 1] = N - 1                          # the last valid column, in an interior and in the ragged M tile
        off = np.zeros(M)
        off[3], off[7] = -100.0, 2.5                            # row 3: every value negative; row 7 (a zero row): every value 2.5
        plain = _planted_case(rng, bm, bn, cols=cols, offsets=off, zero_rows=(7,))
        biased = _planted_case(rng, bm, bn, bias=True)
        biased.biasv[:] = (12 * rng.standard_normal(biased.biasv.size)).astype(np.float32)      # beyond the peak's margin at every N
        neg = _planted_case(rng, bm, bn, alpha=-0.5, cols=(37 * (np.arange(M) + M)) % N)      # the walk goes on where `plain` ended
        negb = _planted_case(rng, bm, bn, alpha=-0.5, bias=True, zero_rows=(5,))
        negb.biasv[:] = -(1 + np.abs(rng.standard_normal(negb.biasv.size))).astype(np.float32)
        negb.biasv[negb.cols[5]] = -0.0                         # acc = +0, alpha acc = -0, -0 + -0 = -0; every other cell < 0
        _planted.clear()
        _planted[(bm, bn)] = [plain, biased, neg, negb]
    return _planted[(bm, bn)]


def _lane_slots(cols, bn, wn_count):
    """(wn, ni, hi, r) of the accumulator register that holds column `cols` of its tile (gather_gemm_v3.h: a lane owns a row; register
    r of block ni is column (r & 3) + 8 (r >> 2) + 4 hi of the wave's ni-th 32-block)"""
    lc = np.asarray(cols) % bn
    wtn = bn // wn_count
    c32 = lc % 32
    return set(zip((lc // wtn).tolist(), ((lc % wtn) // 32).tolist(), ((c32 >> 2) & 1).tolist(), ((c32 & 3) + 4 * (c32 >> 3)).tolist()))


ROWMAX_TILES = ["128x64", "128x128", "256x64", "256x32"]


@pytest.mark.parametrize("tile", ROWMAX_TILES)
def test_rowmax_planted(built_lib, gpu_device, tile):
    """Row m has its maximum at column 37 m mod N: over the rows every wave column, half-wave and accumulator register holds some
    row's maximum (asserted).  One launch of four problems; the table rows behind M and N point at operands of 1e30.  C is inside
    the family's bound and byte-identical to the same launch without the flag, the maxima are ordered(max of the stored row) bit
    for bit, the cells of rows m >= M and the array's tail keep their pre-fill."""
    cfg, bm, bn = TILES[tile]
    cases = _planted_cases(bm, bn)
    plain = cases[0]
    M, N = plain.M, plain.N
    # host-side facts about the operands, in float64
    r = g64.reference64(plain, g64.operand_model(3)).ref[0]
    top2 = np.sort(r, axis=1)[:, -2:]
    ordinary = np.setdiff1d(np.arange(M), [7])
    assert np.array_equal(np.argmax(r, axis=1)[ordinary], plain.cols[ordinary]) and np.all(top2[ordinary, 1] - top2[ordinary, 0] > 1.0)
    assert np.all(r[3] < -60) and np.all(r[7] == 2.5) and plain.cols[11] == N - 1 == plain.cols[M - 1]
    wn_count = WAVES_N[tile]
    # (2 BM - 37 rows do not reach every one of the 2 BN + 8 columns of the 128x128 tile: the alpha < 0 problem continues the walk)
    assert _lane_slots(np.concatenate([plain.cols[ordinary], cases[2].cols]), bn, wn_count) == {(w, ni, h, rr) for w in range(wn_count) for ni in range(bn // wn_count // 32)
                                                               for h in range(2) for rr in range(16)}
    assert set((plain.cols[ordinary] // bn).tolist()) == {0, 1, 2}, "interior tile, second tile and the border of 8 columns"
    rb = g64.reference64(cases[1], g64.operand_model(3)).ref[0]
    moved = np.argmax(rb, axis=1) != np.argmax(rb - cases[1].biasv[None, :N].astype(np.float64), axis=1)
    assert moved.sum() >= 10, "the bias decides the maximum of some rows"
    r3 = g64.reference64(cases[3], g64.operand_model(3)).ref[0]
    assert np.all(np.delete(r3[5], cases[3].cols[5]) < -0.9) and r3[5, cases[3].cols[5]] == 0 and np.signbit(r3[5, cases[3].cols[5]])
    assert np.argmax(g64.reference64(cases[2], g64.operand_model(3)).ref[0][40]) == cases[2].cols[40], "alpha < 0: the maximum of alpha acc"

    L = _Launch(built_lib, gpu_device, cases, 3)
    sides = [_rowmax_side(gpu_device, c, bm) for c in cases]
    for i, s in enumerate(sides):
        _attach_rowmax(L, i, s)
    outs = L.run(cfg, 0)
    for i, (c, got, s) in enumerate(zip(cases, outs, sides)):
        what = f"row-max planted {tile} problem {i}"
        _check(c, 3, got, L.before[i], what, key=f"v3 {tile} NK ROW_MAX", b2=False)          # B1 and B3 of the family
        _check_rowmax(c, got, s, what)
    got5 = a64.stored_rows(cases[3], outs[3])[5]
    assert got5.max() == 0 and np.signbit(got5.max()) and sides[3].get()[5] == 0x7FFFFFFF, "-0.0 is the maximum of row 5"
    assert sides[0].get()[7] == a64.ordered(np.array([2.5], np.float32))[0]
    L.reset()
    for i in range(len(cases)):
        _detach_rowmax(L, i)
    for i, (a, b) in enumerate(zip(outs, L.run(cfg, 0))):
        assert _same_bytes(a, b), f"row-max planted {tile} problem {i}: C differs from the launch without the flag"


@pytest.mark.parametrize("tile", ["128x64", "128x128"])
def test_rowmax_joins_a_running_maximum(built_lib, gpu_device, tile):
    """the array is a RUNNING maximum (atomic max over the N tiles, and over whatever it held): pre-filled per row with
    ordered(x), x five above the row's maximum for even rows and five below for odd rows, every cell ends as the larger of the two"""
    cfg, bm, bn = TILES[tile]
    c = _planted_cases(bm, bn)[0]
    true = g64.reference64(c, g64.operand_model(3)).ref[0].max(axis=1)
    x = (true + np.where(np.arange(c.M) % 2 == 0, 5.0, -5.0)).astype(np.float32)
    pre = a64.ordered(x)
    L = _Launch(built_lib, gpu_device, [c], 3)
    side = _rowmax_side(gpu_device, c, bm, prefill=pre)
    _attach_rowmax(L, 0, side)
    got = L.run(cfg, 0)[0]
    _check_rowmax(c, got, side, f"running maximum {tile}", prefill=pre)
    after = side.get()[:c.M]
    assert np.array_equal(after[0::2], pre[0::2]) and np.all(after[1::2] > pre[1::2])
    assert np.array_equal(after[1::2], a64.ordered(a64.rowmax_ref(c, got))[1::2])


# K, ROW_MAX, bias, act, residual, splitK, chunksPerSplit: row-max tiles of one chunk, a plain tile with its own epilogue, row-max
# tiles of three chunks, split-K planes, one-chunk row-max tiles again
HANDOVER_PROBLEMS = [(32, True, False, 0, False, 1, None), (64, False, True, 1, True, 1, None), (96, True, True, 0, False, 1, None),
                     (96, False, False, 0, False, 2, 2), (32, True, False, 0, False, 1, None)]
_handover_cases = {}


def _handover(bm, bn, wide, need):
    key = (bm, bn, wide, need)
    if key not in _handover_cases:
        _handover_cases.clear()                                    # one launch's worth of buffers at a time
        rng = np.random.default_rng(900 + bm + 3 * bn + 100 * wide)
        cases = []
        for i, (K, rowmax, bias, act, res, splitK, cps) in enumerate(HANDOVER_PROBLEMS):
            n = 4 * bn + 8 if (wide and i == 0) else bn + 8
            tilesN = -(-n // bn)
            tilesM = int(np.ceil(need / 5 / tilesN / splitK)) + 1
            M = tilesM * bm - 37 - 8 * i                           # a ragged last tile
            c = g64.make_case(rng, M, n, K, bm, bn, 0, splitK=splitK, chunksPerSplit=cps, bias=bias, act=act, residual=res, poison=True)
            c.rowmax = rowmax
            cases.append(c)
        _handover_cases[key] = cases
    return _handover_cases[key]


@pytest.mark.parametrize("tile", ["128x64", "128x128"])
@pytest.mark.parametrize("wide", [0, 1], ids=["xcd-queues", "single-queue"])
def test_rowmax_tile_handover(built_lib, gpu_device, tile, wide):
    """The row-max epilogue's LDS scratch is written again by the next tile of the same persistent workgroup, with only that tile's
    chunk loop in between: ROW_MAX problems of ONE chunk (K = 32) and of three, a plain problem with residual and LeakyReLU and a
    split-K problem of 2 + 1 chunks follow one another in one launch of at least 2.5 tiles per resident workgroup, once on the
    per-XCD queues and once (a problem of five N tiles) on the single queue.  Every problem is checked as in the planted test."""
    cfg, bm, bn = TILES[tile]
    resident = built_lib.lib.vsr_gg_resident_blocks(cfg, 0, 3)
    assert resident > 0, built_lib.last_error()
    cases = _handover(bm, bn, wide, int(np.ceil(2.5 * resident)))
    assert all(c.tilesN <= 4 for c in cases[1:]) and cases[0].tilesN == (5 if wide else 2)
    L = _Launch(built_lib, gpu_device, cases, 3)
    ratio = L.tiles() / resident
    print(f"HANDOVER ROW_MAX v3 {tile} wide{wide}: {L.tiles()} tiles / {resident} resident workgroups = {ratio:.2f}")
    assert ratio >= 2.5
    sides = {i: _rowmax_side(gpu_device, c, bm) for i, c in enumerate(cases) if c.rowmax}
    for i, s in sides.items():
        _attach_rowmax(L, i, s)
    outs = L.run(cfg, 0)
    for i, (c, got) in enumerate(zip(cases, outs)):
        what = f"row-max hand-over {tile} wide{wide} problem {i} ({c.M}x{c.N}x{c.K} split {c.splitK})"
        _check(c, 3, got, L.before[i], what, key=f"v3 {tile} NK ROW_MAX hand-over", b2=not c.rowmax)
        if c.rowmax:
            _check_rowmax(c, got, sides[i], what)
    L.reset()
    for i in sides:
        _detach_rowmax(L, i)
    for i, (a, b) in enumerate(zip(outs, L.run(cfg, 0))):
        assert _same_bytes(a, b), f"row-max hand-over {tile} wide{wide} problem {i}: C differs from the launch without the flag"


# =====================================================================================================================================
# 3. VSR_ACT_A_EXP
# =====================================================================================================================================
def _attach_aexp(L, i, maxima_ptr, sums):
    L.probs[i].bias = maxima_ptr
    L.probs[i].R, L.probs[i].rowR = (sums.ptr() if sums is not None else None), None
    L.probs[i].act = A_EXP


def _host_maxima(device, c, bm, mx):
    """ordered(mx) for rows m < M, 0 for the rows of the padded last tile: they decode to NaN, as after the engine's memset"""
    a = np.zeros(c.tilesM * bm, np.uint32)
    a[:c.M] = a64.ordered(mx)
    return Side(device, a)


def _device_maxima(built_lib, device, c, bm, bn, cfg):
    """the maxima as a ROW_MAX launch leaves them: the score GEMM S I (NK, variant 3, K = N = the keys) stores the scores of `c`
    bit for bit -- products with 1 and 0 and sums with 0 are exact -- and its row-maximum array, zeroed as the engine zeroes it and
    padded to tilesM * bm, is what the P.V launch reads"""
    S = a64.scores_of(c)
    keys = c.K
    rng = np.random.default_rng(5)
    sc = g64.make_case(rng, c.M, keys, keys, bm, bn, 0, bias=False, act=0, residual=False)
    from _replay import _scatter

    _scatter(sc.Abuf, 0, sc.rowA[:c.M], sc.colA, keys, S)
    _scatter(sc.Bbuf, 0, sc.rowB[:keys], sc.colB, keys, np.eye(keys, dtype=np.float32))
    L = _Launch(built_lib, device, [sc], 3)
    side = Side(device, np.zeros(sc.tilesM * bm, np.uint32))
    _attach_rowmax(L, 0, side)
    got = L.run(cfg, 0)[0]
    assert _same_bytes(a64.stored_rows(sc, got), S), "S I is not S"
    return side


def _regime_rows(rows):
    return {reg: np.array([j for j, m in enumerate(rows) if a64.regime_of(m) == reg], dtype=np.int64) for reg in a64.REGIMES}


def _b2(what, key, gerr, yerr):
    """B2 of the family on one group of cells: max and rms of the kernel's error at most twice the yardstick's (the factor is the
    family's: the yardstick adds one product at a time and its exp2 is correctly rounded, the kernel adds 2 products per MFMA and
    its v_exp_f32 is good to 1 ulp -- fewer roundings against a coarser one)"""
    gmax, ymax, grms, yrms = gerr.max(), yerr.max(), np.sqrt(np.mean(gerr ** 2)), np.sqrt(np.mean(yerr ** 2))
    rmax, rrms = gmax / ymax if ymax > 0 else 0.0, grms / yrms if yrms > 0 else 0.0
    print(f"RATIO | {key} | {what} | max {gmax:.3e}/{ymax:.3e} = {rmax:.3f} | rms {grms:.3e}/{yrms:.3e} = {rrms:.3f}")
    return gmax <= 2 * ymax and grms <= 2 * yrms, f"{what}: max {gmax:.3e} vs yardstick {ymax:.3e}, rms {grms:.3e} vs {yrms:.3e}"


def _check_aexp(c, bm, r, yard, got, before, sums, what, key):
    """every assertion of section 3 on one fused problem.  r: aexp_ref64 on the maxima the kernel was handed; yard: aexp_yardstick32"""
    cells = g64.written_cells(c)
    vals = got[cells].astype(np.float64)                                   # [splitK][M][N]
    assert not np.isnan(vals).any(), f"{what}: NaN in a written cell (the pad rows' maxima decode to NaN)"
    assert g64.untouched(c, got, before, cells), f"{what}: bytes outside the written cells changed"
    ref, bnd = (r.unsplit[None], r.bound[None]) if c.splitK == 1 else (r.planes, r.plane_bound)      # derived in _attn_f64
    err = np.abs(vals - ref)
    worst = np.unravel_index(np.argmax(err - bnd), err.shape)
    print(f"RATIO | {key} | {what} B1 | max err {err.max():.3e} | got/bound {np.max(err / bnd):.3f}")
    assert np.all(err <= bnd), (f"{what}: |got - ref64| = {err[worst]:.3e} > bound {bnd[worst]:.3e} at (plane, m, n) = {worst} "
                                f"({a64.regime_of(worst[1])} row)")
    S = a64.scores_of(c)
    hot = np.array([m for m in range(c.M) if a64.regime_of(m) == "one-hot"])
    khot = np.argmax(S[hot], axis=1)
    want_hot = a64.values_of(c)[khot] * np.float32(c.alpha)                # 2^0 = 1, every other weight 0, the sum 1: no rounding
    for j, m in enumerate(hot):
        plane = 0 if c.splitK == 1 else khot[j] // (32 * c.chunksPerSplit)
        assert _same_bytes(got[cells[plane, m]], want_hot[j]), f"{what}: one-hot row {m} is not alpha times row {khot[j]} of B, bit for bit"
    if c.splitK > 1:
        ls = sums.get()
        n = c.tilesM * bm
        assert np.all(ls[c.splitK * n:] == g64.SENTINEL), f"{what}: the row-sum array was written beyond splitK * tilesM * BM"
        lrows = ls[:c.splitK * n].reshape(c.splitK, n)[:, :c.M].astype(np.float64)
        serr = np.abs(lrows - r.sums)
        w = np.unravel_index(np.argmax(serr - r.sum_bound), serr.shape)
        print(f"RATIO | {key} | {what} row sums | max relative err {np.max(serr / r.sums):.3e} | got/bound {np.max(serr / r.sum_bound):.3f}")
        assert np.all(serr <= r.sum_bound), (f"{what}: row sum of (split, m) = {w} off by {serr[w]:.3e} (relative {serr[w] / r.sums[w]:.3e}), "
                                             f"bound {r.sum_bound[w]:.3e} (relative {r.sum_bound[w] / r.sums[w]:.3e})")
        for j, m in enumerate(hot):
            assert np.array_equal(ls[:c.splitK * n].reshape(c.splitK, n)[:, m], np.eye(c.splitK, dtype=np.float32)[khot[j] // (32 * c.chunksPerSplit)])
    rows, yun, ypl, ysm = yard
    assert rows.size * c.N >= 4096
    yerr = np.abs((yun[None] if c.splitK == 1 else ypl).astype(np.float64) - ref[:, rows])
    # numpy keeps denormal weights, products and results, v_exp_f32 and the matrix cores may flush each of them: what the bound
    # allows for that (the PHI terms of _attn_f64, with l >= 1) is taken off the kernel's error before the two are compared
    flush = abs(float(c.alpha)) * a64.PHI * (np.abs(a64.values_of(c)).sum(axis=0)[None, None, :] + 2 * c.K + 2)
    berr = np.maximum(err - flush, 0.0)
    fails = []
    for reg, idx in _regime_rows(rows).items():
        ok, msg = _b2(f"{what} {reg}", key, berr[:, rows[idx]], yerr[:, idx])
        if not ok:
            fails.append(msg)
    assert not fails, "; ".join(fails)


AEXP_MATRIX = [(tile, wide, K, sk, cps) for tile in ("128x64", "128x128") for wide in (0, 1) for K, sk, cps in a64.KSPLITS]
_aexp_refs = {}


def _aexp_reference(bm, bn, wide, K, sk, cps, alpha):
    """case, host maxima, float64 reference and yardstick: computed once, shared by the two ways of feeding the maxima"""
    key = (bm, bn, wide, K, sk, cps, alpha)
    if key not in _aexp_refs:
        if len(_aexp_refs) > 8:
            _aexp_refs.clear()
        c = a64.aexp_case(bm, bn, wide, K, sk, cps, alpha)
        mx = a64.host_rowmax(c)
        _aexp_refs[key] = (c, mx, a64.aexp_ref64(c, mx), a64.aexp_yardstick32(c, mx))
    return _aexp_refs[key]


@pytest.mark.parametrize("feed", ["host-maxima", "rowmax-launch"])
@pytest.mark.parametrize("alpha", [1.0, 0.5])
@pytest.mark.parametrize("tile,wide,K,sk,cps", AEXP_MATRIX, ids=[f"{t}-N{'2bn' if w else 'bn+8'}-K{K}-split{sk}" for t, w, K, sk, cps in AEXP_MATRIX])
def test_aexp_matrix(built_lib, gpu_device, tile, wide, K, sk, cps, alpha, feed):
    """M = BM + 37 (a ragged second M tile whose pad rows' maxima decode to NaN), two N tiles (the tiles with tn != 0 skip the sums
    of a split product), 1, 3 and 5 chunks unsplit and cut 2 + 1 and 2 + 2 + 1 (the kcEnd clamp), alpha 1 and 0.5, seven score
    regimes as the rows of one matrix, the maxima computed on the host or left by a ROW_MAX launch on the same scores.  C (or
    every plane) and the row sums inside their derived per-cell bounds, B2 per regime, one-hot rows bit for bit, no NaN, nothing
    outside the store set, the same bytes from a second launch."""
    cfg, bm, bn = TILES[tile]
    c, mx, r, yard = _aexp_reference(bm, bn, wide, K, sk, cps, alpha)
    if feed == "host-maxima":
        maxima = _host_maxima(gpu_device, c, bm, mx)
    else:
        maxima = _device_maxima(built_lib, gpu_device, c, bm, bn, cfg)
        left = maxima.get()
        assert np.array_equal(left[:c.M], a64.ordered(mx)) and not left[c.M:].any(), "the ROW_MAX launch left other maxima than the host computes"
    sums = Side(gpu_device, np.full(sk * c.tilesM * bm + TAIL, g64.SENTINEL, np.float32)) if sk > 1 else None
    L = _Launch(built_lib, gpu_device, [c], 1)
    _attach_aexp(L, 0, maxima.ptr(), sums)
    got = L.run(cfg, 1, V_AEXP)[0]
    what = f"A_EXP {tile} {c.M}x{c.N}x{K} split {sk} alpha {alpha} {feed}"
    _check_aexp(c, bm, r, yard, got, L.before[0], sums, what, f"aexp {tile} KN")
    first_sums = sums.get().copy() if sums is not None else None
    L.reset()
    if sums is not None:
        sums.reset()
    again = L.run(cfg, 1, V_AEXP)[0]
    assert _same_bytes(got, again), f"{what}: a second launch wrote other bytes"
    if sums is not None:
        live = np.ones(first_sums.size, dtype=bool)                      # rows [M, tilesM * BM) of every split are the kernel's own (NaN)
        for s in range(sk):
            live[s * c.tilesM * bm + c.M:(s + 1) * c.tilesM * bm] = False
        assert _same_bytes(first_sums[live], sums.get()[live]), f"{what}: a second launch wrote other row sums"


@pytest.mark.parametrize("tile", ["128x64", "128x128"])
def test_aexp_beside_plain_problems(built_lib, gpu_device, tile):
    """a plain KN problem (bias, residual, ReLU) before and after a fused one under the A_EXP variant: the plain ones byte-identical
    to variant 1 without the variant flag; the fused one inside its bound -- its `bias` pointer is the maxima, which the kernel
    must not add"""
    cfg, bm, bn = TILES[tile]
    rng = np.random.default_rng(31 + bn)
    mk = lambda M, N, K: g64.make_case(rng, M, N, K, bm, bn, 1, bias=True, act=2, residual=True)
    c, mx, r, yard = _aexp_reference(bm, bn, 0, 96, 1, None, 1.0)
    cases = [mk(150, bn + 8, 64), c, mk(bm + 5, 40, 96)]
    L = _Launch(built_lib, gpu_device, cases, 1)
    maxima = _host_maxima(gpu_device, c, bm, mx)
    _attach_aexp(L, 1, maxima.ptr(), None)
    outs = L.run(cfg, 1, V_AEXP)
    _check_aexp(c, bm, r, yard, outs[1], L.before[1], None, f"A_EXP {tile} between plain problems", f"aexp {tile} KN mixed")
    for i in (0, 2):
        _check(cases[i], 1, outs[i], L.before[i], f"plain problem {i} under the A_EXP variant {tile}", key=f"aexp {tile} KN plain")
    plainL = _Launch(built_lib, gpu_device, [cases[0], cases[2]], 1)
    for i, b in zip((0, 2), plainL.run(cfg, 1)):
        assert _same_bytes(outs[i], b), f"plain problem {i} differs between variant 1 | VSR_VARIANT_A_EXP and variant 1"


# =====================================================================================================================================
# 4. the chain at a readable size
# =====================================================================================================================================
def _dense(x, ld):
    out = np.zeros((x.shape[0], ld), np.float32)
    out[:, :x.shape[1]] = x
    return out


@pytest.mark.parametrize("tile", ["128x64", "128x128"])
def test_attention_chain(built_lib, gpu_device, tile):
    """score GEMM (NK, variant 3, alpha = log2(e) / sqrt(D), ROW_MAX into a zeroed array) -> A_EXP P.V unsplit and cut 2 + 2 + 1 ->
    reduce-scatter with the row sums, against float64 softmax(Q K^T / sqrt(D)) V of the RAW Q, K, V; D = 96, 160 tokens,
    M = BM + 37.  The unfused device path (plain scores, k_softmax_rows, plain KN P.V) runs on the same inputs."""
    cfg, bm, bn = TILES[tile]
    D, T, M = 96, 160, bm + 37
    rng = np.random.default_rng(41 + bn)
    Q, Kt, V = (rng.standard_normal(s).astype(np.float32) for s in ((M, D), (T, D), (T, D)))
    alpha = float(np.float32(np.log2(np.e) / np.sqrt(D)))
    from _replay import _scatter

    # 1. scores
    sc = g64.make_case(rng, M, T, D, bm, bn, 0, bias=False, act=0, residual=False, alpha=alpha)
    _scatter(sc.Abuf, 0, sc.rowA[:M], sc.colA, D, Q)
    _scatter(sc.Bbuf, 0, sc.rowB[:T], sc.colB, D, Kt)
    Ls = _Launch(built_lib, gpu_device, [sc], 3)
    maxima = Side(gpu_device, np.zeros(sc.tilesM * bm, np.uint32))
    _attach_rowmax(Ls, 0, maxima)
    got_s = Ls.run(cfg, 0)[0]
    _check(sc, 3, got_s, Ls.before[0], f"chain {tile} scores", key=f"chain {tile} scores")
    S = a64.stored_rows(sc, got_s)
    left = maxima.get()
    assert np.array_equal(left[:M], a64.ordered(S.max(axis=1))) and not left[M:].any()
    mx = a64.from_ordered(left[:M])

    # float64 of the raw operands
    q64, k64, v64 = Q.astype(np.float64), Kt.astype(np.float64), V.astype(np.float64)
    z = (q64 @ k64.T) / np.sqrt(D)
    w = np.exp(z - z.max(axis=1, keepdims=True))
    w /= w.sum(axis=1, keepdims=True)
    want = w @ v64
    # THE BOUND.  |got - want| <= |got - ref(stored scores)| + |ref(stored scores) - want|.
    #  first term: the derived bound of the P.V kernel on the scores it read (_attn_f64; for the split product: the planes' and the
    #    sums' bounds carried through (sum planes) / (sum sums) -- d(P / l) = dP / l - (P / l) dl / l --, the reduce pass' own
    #    nsplit - 1 additions in numerator and denominator, one reciprocal and one product: (2 (nsplit - 1) + 3) u mag).
    #  second term: a stored score differs from alpha q.k by delta_s <= (D + 4) u alpha sum_d |q_d| |k_d| (the family's B1: D
    #    roundings of the sum, alpha's own rounding and its use); every weight moves by the factor 2^delta_s, numerator and
    #    denominator each by at most ln2 max_k delta_s relative: 2 ln2 max_k delta_s[m] mag[m][n].
    delta = (D + 4) * U32 * alpha * (np.abs(q64) @ np.abs(k64).T)
    mag = w @ np.abs(v64)
    prop = 2 * a64.LN2 * delta.max(axis=1)[:, None] * mag

    def pv_case(splitK, cps):
        c = g64.make_case(np.random.default_rng(43 + splitK), M, D, T, bm, bn, 1, splitK=splitK, chunksPerSplit=cps, bias=False, act=0, residual=False)
        a64.set_scores(c, S)
        a64.set_values(c, V)
        c.act = A_EXP
        return c

    results = {}
    # 2a. unsplit
    c1 = pv_case(1, None)
    r1 = a64.aexp_ref64(c1, mx)
    L1 = _Launch(built_lib, gpu_device, [c1], 1)
    _attach_aexp(L1, 0, maxima.ptr(), None)
    got1 = L1.run(cfg, 1, V_AEXP)[0]
    assert g64.untouched(c1, got1, L1.before[0], g64.written_cells(c1))
    results["fused unsplit"] = (got1[g64.written_cells(c1)[0]].astype(np.float64), r1.bound + prop)
    # 2b + 3. split 2 + 2 + 1 and the reduce pass
    c3 = pv_case(3, 2)
    r3 = a64.aexp_ref64(c3, mx)
    n = c3.tilesM * bm
    sums = Side(gpu_device, np.full(3 * n + TAIL, g64.SENTINEL, np.float32))
    L3 = _Launch(built_lib, gpu_device, [c3], 1)
    _attach_aexp(L3, 0, maxima.ptr(), sums)
    got3 = L3.run(cfg, 1, V_AEXP)[0]
    assert g64.untouched(c3, got3, L3.before[0], g64.written_cells(c3))
    planes = np.ascontiguousarray(got3[g64.written_cells(c3)])                    # [3][M][D] dense, as the engine's planes lie
    assert np.all(np.abs(planes - r3.planes) <= r3.plane_bound)
    ew = C.CDLL(built_lib.LIB_PATH)
    fn = ew.vsr_launch_reduce_scatter_fmt
    fn.restype, fn.argtypes = C.c_int, [{"p": C.c_void_p, "i": C.c_int, "l": C.c_int64}[ch] for ch in R.PROTOTYPES["vsr_launch_reduce_scatter_fmt"]]
    dpart = torch.from_numpy(planes.reshape(-1)).to(gpu_device)
    rowC = torch.from_numpy((rng.permutation(M + 3)[:M] * 128).astype(np.int32)).to(gpu_device)
    colC = torch.from_numpy((rng.permutation(4)[:3] * 32).astype(np.int32)).to(gpu_device)
    before = np.full((M + 3) * 128, g64.SENTINEL, np.float32)
    dout = torch.from_numpy(before).to(gpu_device)
    torch.cuda.synchronize()
    rc = fn(dpart.data_ptr(), 3, M * D, M, D, rowC.data_ptr(), colC.data_ptr(), dout.data_ptr(), 0, sums.ptr(), n, None)
    torch.cuda.synchronize()
    assert rc == 0
    out = dout.cpu().numpy()
    cells = R.scatter_cells(rowC.cpu().numpy(), colC.cpu().numpy(), D)
    rest = np.ones(out.size, dtype=bool)
    rest[cells.reshape(-1)] = False
    assert np.all(out[rest] == g64.SENTINEL), "the reduce pass wrote outside its scatter"
    l3 = r3.sums.sum(0)[:, None]
    b3 = r3.plane_bound.sum(0) / l3 + r3.mag * (r3.sum_bound.sum(0)[:, None] / l3) + (2 * 2 + 3) * U32 * r3.mag
    results["fused split 2+2+1 + reduce"] = (out[cells].astype(np.float64), b3 + prop)

    # the unfused device path: plain scores (alpha = 1), softmax rows with the scale 1 / sqrt(D), plain KN P.V
    su = g64.make_case(np.random.default_rng(47), M, T, D, bm, bn, 0, bias=False, act=0, residual=False)
    _scatter(su.Abuf, 0, su.rowA[:M], su.colA, D, Q)
    _scatter(su.Bbuf, 0, su.rowB[:T], su.colB, D, Kt)
    Lu = _Launch(built_lib, gpu_device, [su], 3)
    Su = np.ascontiguousarray(a64.stored_rows(su, Lu.run(cfg, 0)[0]))
    sm = (built_lib.SMProblem * 1)()
    dS, dP = torch.from_numpy(Su.reshape(-1)).to(gpu_device), torch.full((M * T,), 9.0, device=gpu_device)
    sm[0].S, sm[0].P, sm[0].M, sm[0].N, sm[0].ldS, sm[0].ldP = dS.data_ptr(), dP.data_ptr(), M, T, T, T
    sm[0].nsplit, sm[0].scale, sm[0].flags, sm[0].splitStride = 1, 1.0 / np.sqrt(D), 0, M * T
    torch.cuda.synchronize()
    built_lib.check(built_lib.lib.vsr_run_softmax(sm, 1, None))
    torch.cuda.synchronize()
    P = dP.cpu().numpy().reshape(M, T)
    cu = g64.make_case(np.random.default_rng(48), M, D, T, bm, bn, 1, bias=False, act=0, residual=False)
    a64.set_scores(cu, P)
    a64.set_values(cu, V)
    Lp = _Launch(built_lib, gpu_device, [cu], 1)
    gotu = Lp.run(cfg, 1)[0]
    unf = np.abs(gotu[g64.written_cells(cu)[0]].astype(np.float64) - want)
    print(f"RATIO | chain {tile} | unfused device path | max {unf.max():.3e} | rms {np.sqrt(np.mean(unf ** 2)):.3e} | "
          f"got/bound {np.max(unf / (r1.bound + prop)):.3f}")
    assert np.all(unf <= r1.bound + prop), "the unfused device path leaves the bound"
    for name, (vals, bnd) in results.items():
        err = np.abs(vals - want)
        print(f"RATIO | chain {tile} | {name} | max {err.max():.3e}/{unf.max():.3e} = {err.max() / unf.max():.3f} | "
              f"rms {np.sqrt(np.mean(err ** 2)):.3e}/{np.sqrt(np.mean(unf ** 2)):.3e} = {np.sqrt(np.mean(err ** 2) / np.mean(unf ** 2)):.3f} | "
              f"got/bound {np.max(err / bnd):.3f}")
        assert np.all(err <= bnd), f"chain {tile} {name}: {np.max(err / bnd):.2f} x the bound"
        assert err.max() <= 2 * unf.max() and np.mean(err ** 2) <= 4 * np.mean(unf ** 2), f"chain {tile} {name}: more than twice the unfused path's error"


# =====================================================================================================================================
# 5. refusals instead of misuse
# =====================================================================================================================================
def test_fused_flags_are_refused_where_no_kernel_reads_them(built_lib, gpu_device):
    """ROW_MAX outside variant 3 / NK / splitK 1 / with R, A_EXP without the variant flag, without maxima or (split) without a
    row-sum array, the A_EXP variant on NK problems or other tiles: VSR_ERR_ARG before anything is launched -- C, the row-maximum
    and the row-sum arrays still hold their pre-fill"""
    lib = built_lib.lib
    cfg, bm, bn = TILES["128x64"]
    rng = np.random.default_rng(61)
    nk = g64.make_case(rng, 70, 40, 64, bm, bn, 0, bias=False, act=0, residual=False)
    nk2 = g64.make_case(rng, 70, 40, 64, bm, bn, 0, splitK=2, chunksPerSplit=1)
    kn = g64.make_case(rng, 70, 40, 64, bm, bn, 1, bias=False, act=0, residual=False)
    kn2 = g64.make_case(rng, 70, 40, 64, bm, bn, 1, splitK=2, chunksPerSplit=1)
    side = Side(gpu_device, np.full(2 * bm + TAIL, SENT_U32, np.uint32))
    launches = []

    def refused(case, bmode, variant, tile_cfg=cfg, flagged=False, plan=False, **fields):
        L = _Launch(built_lib, gpu_device, [case], 1)
        for k, v in fields.items():
            setattr(L.probs[0], k, v)
        if plan:
            handle = C.c_void_p()
            rc = lib.vsr_gemm_plan_create(L.probs, 1, tile_cfg, bmode, variant, C.byref(handle))
            assert handle.value is None
        elif flagged:
            flag = C.c_uint32(7)
            rc = lib.vsr_run_gather_gemm_flagged(L.probs, 1, tile_cfg, bmode, variant, C.byref(flag), None)
            assert flag.value == 7
        else:
            rc = lib.vsr_run_gather_gemm_variant(L.probs, 1, tile_cfg, bmode, variant, None)
        assert rc == built_lib.VSR_ERR_ARG, f"{fields} variant {variant:#x} bmode {bmode}: returned {rc}, expected VSR_ERR_ARG"
        launches.append(L)

    for v in (1, 2, 4, 5, 6, 7, V_AEXP):                                                    # ROW_MAX with variant != 3
        refused(kn if v == V_AEXP else nk, 1 if v == V_AEXP else 0, v, act=ROW_MAX, R=side.ptr())
    for v in (4, 5, 6, 7):
        refused(nk, 0, v, flagged=True, act=ROW_MAX, R=side.ptr())
    for v in (1, 2, 4):
        refused(nk, 0, v, plan=True, act=ROW_MAX, R=side.ptr())
    refused(kn, 1, 3, act=ROW_MAX, R=side.ptr())                                            # ROW_MAX with bmode != NK
    refused(nk2, 0, 3, act=ROW_MAX, R=side.ptr())                                           # ... splitK > 1
    refused(nk, 0, 3, act=ROW_MAX, R=None)                                                  # ... a null R
    refused(nk, 0, 3, plan=True, act=ROW_MAX, R=None)
    for v in (1, 3):                                                                        # A_EXP without VSR_VARIANT_A_EXP
        refused(kn, 1, v, act=A_EXP, bias=side.ptr())
        refused(kn, 1, v, plan=True, act=A_EXP, bias=side.ptr())
    refused(kn, 1, V_AEXP, act=A_EXP, bias=None)                                            # A_EXP with null maxima
    refused(kn2, 1, V_AEXP, act=A_EXP, bias=side.ptr(), R=None)                             # A_EXP, splitK > 1, null R
    refused(nk, 0, V_AEXP)                                                                  # the A_EXP variant with NK
    for t in ("256x32", "256x64", "256x128", "256x256"):                                    # ... or another tile
        other = g64.make_case(rng, 70, 40, 64, TILES[t][1], TILES[t][2], 1, bias=False, act=0, residual=False)
        refused(other, 1, V_AEXP, tile_cfg=TILES[t][0])
    torch.cuda.synchronize()
    for L in launches:
        assert _same_bytes(L.outputs()[0], L.before[0]), "a refused launch wrote to C"
    assert np.array_equal(side.get(), side.before), "a refused launch wrote to the side array"
    # the launches the kernels do serve still run
    L = _Launch(built_lib, gpu_device, [nk], 3)
    ok = _rowmax_side(gpu_device, nk, bm)
    _attach_rowmax(L, 0, ok)
    _check_rowmax(nk, L.run(cfg, 0)[0], ok, "served ROW_MAX launch")
