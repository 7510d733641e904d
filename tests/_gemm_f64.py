"""Float64 reference of the gather-GEMM descriptor (include/vsr_hip.h, GGProblem) with the operand model of every kernel variant, the
fp32 one-product-at-a-time yardstick of the same model, and the derived element-wise bound.  CPU only: numpy and tests/_replay.py.

A *case* describes one problem in LOGICAL fp32 values (the layout of test_gpu_kernels._make_gemm_case, which this module also reads):
Abuf / Bbuf / Rbuf / Cbuf / biasv with the offset tables rowA .. rowR.  Optional fields: baseC / baseR (floats the C / R pointer lies
past the start of its buffer), inplace (R and rowR are C and rowC: the residual is the pre-launch content of C).  `physical()` turns
a case into the bytes a variant reads (split format where it reads split format); `reference64()` never looks at those."""
from types import SimpleNamespace

import numpy as np
import torch

from _replay import _gather, _scatter

ACT_OUT_SPLIT, ACT_POST_RELU = 0x100, 0x200
SENTINEL = np.float32(-7.0)
U32 = 2.0 ** -24            # unit roundoff of fp32


# ---- split format: a 32-float chunk holds [32 fp16 hi | 32 fp16 lo] ------------------------------------------------------------------
def split_halves(x):
    """hi = fp16(x), lo = fp16(x - hi) of fp32 values, as the kernels and vsr_launch_to_split form them"""
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))      # torch: the same IEEE conversions, several times faster
    hi = t.to(torch.float16)
    lo = (t - hi.to(torch.float32)).to(torch.float16)
    return hi.numpy(), lo.numpy()


def _widen(h, dtype=np.float64):
    """fp16 -> dtype, exactly (through torch: numpy converts halves one at a time)"""
    return torch.from_numpy(np.ascontiguousarray(h)).to(torch.float64 if dtype == np.float64 else torch.float32).numpy()


def to_split_inplace(buf, starts):
    """fp32 -> split format on the 32-float chunks of `buf` that start at `starts`"""
    starts = np.unique(np.asarray(starts, dtype=np.int64))
    if starts.size == 0:
        return
    win = np.lib.stride_tricks.sliding_window_view(buf, 32, writeable=True)      # one index per chunk (see _replay._gather)
    hi, lo = split_halves(win[starts])
    win[starts] = np.ascontiguousarray(np.concatenate([hi, lo], axis=1)).view(np.float32)


def split_positions(cells):
    """uint16 positions (hi, lo) of the logical cells `cells` (float indices chunk + n % 32) of a split-format buffer"""
    cells = np.asarray(cells, dtype=np.int64)
    chunk, lane = cells - cells % 32, cells % 32
    return 2 * chunk + lane, 2 * chunk + 32 + lane


def from_split(buf, cells):
    """float64 hi + lo of the logical cells of a split-format buffer (chunks 32-float aligned in the buffer)"""
    h16 = np.ascontiguousarray(buf).view(np.uint16)
    hi_i, lo_i = split_positions(cells)
    with np.errstate(invalid="ignore"):
        return _widen(h16[hi_i].view(np.float16)) + _widen(h16[lo_i].view(np.float16))


def chunk_starts(rows, cols, base=0):
    return (base + np.asarray(rows, np.int64)[:, None] + np.asarray(cols, np.int64)[None, :]).reshape(-1)


# ---- how a variant sees its operands ------------------------------------------------------------------------------------------------
def operand_model(variant):
    """kind: 'fp32' the values as given (variants 1, 3, narrow); 'split' hi = fp16(x), lo = fp16(x - hi) and the product
    a_hi b_hi + a_hi b_lo + a_lo b_hi (4, 5); 'half' fp16(x) alone (6, 7).  split_tensors: A, B and R lie in split format in memory
    (5, 6 on every tile, the 256 x 256 tile included) -- the residual is then hi + lo of R."""
    v = "narrow" if variant in ("narrow", 8) else int(variant)
    if v in (1, 2, 3, "narrow"):
        return SimpleNamespace(kind="fp32", split_tensors=False)
    if v in (4, 5):
        return SimpleNamespace(kind="split", split_tensors=v == 5)
    if v in (6, 7):
        return SimpleNamespace(kind="half", split_tensors=v == 6)
    raise ValueError(f"no operand model for variant {variant!r}")


def _terms(A, B, kind, dtype):
    """the (a, b) factor pairs whose products the variant accumulates, in its order per k"""
    if kind == "fp32":
        return [(A.astype(dtype), B.astype(dtype))]
    ah, al = split_halves(A)
    bh, bl = split_halves(B)
    if kind == "half":
        return [(_widen(ah, dtype), _widen(bh, dtype))]
    ah, al, bh, bl = (_widen(x, dtype) for x in (ah, al, bh, bl))
    return [(ah, bh), (ah, bl), (al, bh)]


def _get(case, name, default):
    return getattr(case, name, default)


def _operands(case, rows=None):
    """A [M or rows][K], B [K][N] gathered in fp32"""
    M, N, K = case.M, case.N, case.K
    rowA = np.asarray(case.rowA[:M], np.int64)
    if rows is not None:
        rowA = rowA[rows]
    A = _gather(case.Abuf, 0, rowA, case.colA, K)
    if case.bmode == 0:
        B = _gather(case.Bbuf, 0, np.asarray(case.rowB[:N], np.int64), case.colB, K).T
    else:
        B = _gather(case.Bbuf, 0, np.asarray(case.rowB[:K], np.int64), case.colB, N)
    return A, B


def _residual(case, model, rows=None):
    """the residual the kernel adds, as exact fp32 values in float64 ([M or rows][N]); None without one"""
    if not case.use_res or case.splitK > 1:
        return None
    M, N = case.M, case.N
    if _get(case, "inplace", False):
        buf, rowR = case.Cbuf, np.asarray(case.rowC[:M], np.int64)
    else:
        buf, rowR = case.Rbuf, np.asarray(case.rowR[:M], np.int64)
    if rows is not None:
        rowR = rowR[rows]
    R = _gather(buf, 0, rowR, case.colC, N)
    if model.split_tensors:
        hi, lo = split_halves(R)
        return _widen(hi) + _widen(lo)
    return R.astype(np.float64)


def _slices(case):
    """(plane, first k, end k) of every split-K slice; one slice of all K without split-K"""
    if case.splitK == 1:
        yield 0, 0, case.K
        return
    for s in range(case.splitK):
        k0 = s * case.chunksPerSplit * 32
        yield s, k0, min(case.K, k0 + case.chunksPerSplit * 32)


def written_cells(case):
    """[splitK][M][N] float indices into Cbuf of the cells the descriptor writes"""
    n = np.arange(case.N)
    col = np.asarray(case.colC, np.int64)[n // 32] + n % 32
    cell = np.asarray(case.rowC[:case.M], np.int64)[:, None] + col[None, :]
    if case.splitK == 1:
        return cell[None]
    return np.stack([cell + s * case.splitStride for s in range(case.splitK)])


def _epilogue(v, case, R, dtype):
    """act(alpha * v + bias) + R, POST_RELU: in `dtype`, one rounded operation after the other.  Works in place on v (a fresh
    accumulator of that dtype).  (x * 1 is x and max(x, slope x) is the leaky ReLU for 0 < slope < 1: no step is skipped.)"""
    partial = case.splitK > 1
    assert v.dtype == dtype
    if case.alpha != 1.0:
        v *= dtype(case.alpha)
    if case.use_bias and not partial:
        v += case.biasv[:case.N].astype(dtype)[None, :]
    act = 0 if partial else case.act & 0xff
    if act in (1, 3):
        np.maximum(v, dtype(np.float32(0.2 if act == 1 else 0.1)) * v, out=v)
    elif act == 2:
        np.maximum(v, dtype(0), out=v)
    if R is not None:
        v += R
        if case.act & ACT_POST_RELU:
            np.maximum(v, dtype(0), out=v)
    return v


def _pairs64(A, B, kind):
    """the model's products as float64 matrix pairs whose products add up to the exact sum -- a_hi b_hi + a_hi b_lo + a_lo b_hi is
    a_hi (b_hi + b_lo) + a_lo b_hi, and b_hi + b_lo is exact in float64 -- and the same for the sum of magnitudes"""
    if kind == "fp32":
        A, B = A.astype(np.float64), B.astype(np.float64)
        return [(A, B)], [(np.abs(A), np.abs(B))]
    ah, al = (_widen(x) for x in split_halves(A))
    bh, bl = (_widen(x) for x in split_halves(B))
    if kind == "half":
        return [(ah, bh)], [(np.abs(ah), np.abs(bh))]
    return [(ah, bh + bl), (al, bh)], [(np.abs(ah), np.abs(bh) + np.abs(bl)), (np.abs(al), np.abs(bh))]


def reference64(case, model):
    """The descriptor formula in float64 on the variant's operand model.  Returns ref [splitK][M][N] (unnormalised planes for
    split-K), cells (the same shape: float indices into Cbuf -- exactly the written set), S = |alpha| sum |a_k b_k| + |bias| + |R|
    over the products the model forms, and kn = products accumulated per plane ([splitK])."""
    A, B = _operands(case)
    pairs, mpairs = _pairs64(A, B, model.kind)
    R = _residual(case, model)
    refs, mags, kn = [], [], []
    for s, k0, k1 in _slices(case):
        acc = pairs[0][0][:, k0:k1] @ pairs[0][1][k0:k1, :]
        mag = mpairs[0][0][:, k0:k1] @ mpairs[0][1][k0:k1, :]
        for (a, b), (ma, mb) in zip(pairs[1:], mpairs[1:]):
            acc += a[:, k0:k1] @ b[k0:k1, :]
            mag += ma[:, k0:k1] @ mb[k0:k1, :]
        if case.alpha != 1.0:
            mag *= abs(float(case.alpha))
        if case.use_bias and case.splitK == 1:
            mag += np.abs(case.biasv[:case.N].astype(np.float64))[None, :]
        if R is not None:
            mag += np.abs(R)
        refs.append(_epilogue(acc, case, R, np.float64))
        mags.append(mag)
        kn.append(k1 - k0)
    one = case.splitK == 1
    return SimpleNamespace(ref=refs[0][None] if one else np.stack(refs), cells=written_cells(case),
                           S=mags[0][None] if one else np.stack(mags), kn=np.asarray(kn))


def bound(r64, out_split=False):
    """|got - ref64| <= (K + 4) 2^-24 S: K - 1 additions and one product rounding on the longest path of a sum of K products, then
    alpha, bias, the activation's slope and the residual, each at most one rounding of a value no larger than S (first order in
    2^-24; an order of summation that rounds less often only does better).  OUT_SPLIT stores fp16(v) + fp16(v - fp16(v)):
    2^-22 |v| at most, twice that allowed."""
    b = (r64.kn[:, None, None] + 4) * U32 * r64.S
    if out_split:
        b = b + 2.0 ** -21 * np.abs(r64.ref)
    return b


def yardstick_rows(case, min_cells=4096):
    """the fixed subsample of output rows: evenly spread over M, first and last row included, at least min_cells cells"""
    n = min(case.M, max(2, -(-min_cells // case.N)))
    return np.unique(np.linspace(0, case.M - 1, n).round().astype(np.int64))


def yardstick32(case, model, rows, out_split=False):
    """The same model in fp32, one product at a time: acc = fl(acc + fl(a_k b_k)), no FMA, then the epilogue one fp32 operation at a
    time -- the least favourable correct fp32 order.  out_split: the value as it is read back from split format, hi + lo (exact
    in fp32).  Returns [splitK][len(rows)][N] fp32."""
    A, B = _operands(case, rows)
    terms = _terms(A, B, model.kind, np.float32)
    R = _residual(case, model, rows)
    out = []
    with np.errstate(over="ignore", invalid="ignore"):
        for s, k0, k1 in _slices(case):
            acc = np.zeros((len(rows), case.N), np.float32)
            for k in range(k0, k1):
                for a, b in terms:
                    acc = acc + a[:, k, None] * b[None, k, :]          # numpy rounds the product to fp32, then the sum
            v = _epilogue(acc, case, None if R is None else R.astype(np.float32), np.float32)
            if out_split:
                hi, lo = split_halves(v)
                v = hi.astype(np.float32) + lo.astype(np.float32)
            out.append(v)
    return np.stack(out)


# ---- bytes on the device ------------------------------------------------------------------------------------------------------------
def physical(case, model):
    """the buffers the variant reads and writes, as fp32 arrays of the case's layout: A, B and the residual in split format where
    the variant reads split format; C as it lies before the launch (an in-place residual of an OUT_SPLIT problem lies there in
    split format)"""
    if not model.split_tensors:            # the case's own arrays: nobody writes to them
        return SimpleNamespace(A=case.Abuf, B=case.Bbuf, R=case.Rbuf, C=case.Cbuf, bias=case.biasv)
    out = SimpleNamespace(A=case.Abuf.copy(), B=case.Bbuf.copy(), R=case.Rbuf.copy(), C=case.Cbuf.copy(), bias=case.biasv)
    to_split_inplace(out.A, chunk_starts(case.rowA, case.colA))
    to_split_inplace(out.B, chunk_starts(case.rowB, case.colB))
    if case.use_res and case.splitK == 1:
        if _get(case, "inplace", False):
            assert case.act & ACT_OUT_SPLIT, "a split-format residual can only alias a split-format output"
            to_split_inplace(out.C, chunk_starts(case.rowC[:case.M], case.colC))
        else:
            to_split_inplace(out.R, chunk_starts(case.rowR[:case.M], case.colC))
    return out


def decode_output(case, got, cells):
    """the values a launch left in the written cells, float64 (hi + lo for an OUT_SPLIT problem)"""
    if case.act & ACT_OUT_SPLIT and case.splitK == 1:
        return from_split(got, cells)
    return got[cells].astype(np.float64)


def untouched(case, got, before, cells):
    """True when every byte outside the written cells is what it was before the launch (uint16 granularity in split format)"""
    if case.act & ACT_OUT_SPLIT and case.splitK == 1:
        g, b = np.ascontiguousarray(got).view(np.uint16), np.ascontiguousarray(before).view(np.uint16)
        where = np.concatenate(split_positions(cells.reshape(-1)))
    else:
        g, b = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(before).view(np.uint32)
        where = cells.reshape(-1)
    changed = np.flatnonzero(g != b)
    written = np.zeros(g.shape[0], dtype=bool)
    written[where] = True
    return g.shape == b.shape and bool(np.all(written[changed]))


# ---- cases --------------------------------------------------------------------------------------------------------------------------
def make_case(rng, M, N, K, bm, bn, bmode, splitK=1, chunksPerSplit=None, bias=True, act=0, residual=True, alpha=1.0, tilesM=None,
              odd=False, inplace=False, poison=False):
    """A random problem with scattered rows and chunks.  A, B rows and every chunk offset keep 16-byte alignment.
    odd: the C and R pointers lie one float past a 16-byte boundary and the C / R row offsets are odd numbers of floats (plain fp32
    C and R only).  inplace: R is C.  poison: the table rows m >= M of A and n >= N of B (NK) point at rows of 1e6.
    tilesM (256 x 256 tile only): more M tiles than ceil(M / 256)."""
    tilesM = tilesM if tilesM is not None else -(-M // bm)
    tilesN = -(-N // bn)
    rowsT = min(bm, -(-(-(-M // tilesM)) // 32) * 32)           # rows of one tile
    Mp, Np, kc = max(tilesM * rowsT, -(-M // bm) * bm), tilesN * bn, K // 32
    colA = (rng.permutation(kc + 3)[:kc] * 32).astype(np.int64)
    strideA = (kc + 3) * 32 + 4
    rowA = (rng.permutation(Mp + 5)[:Mp] * strideA).astype(np.int64)
    Abuf = rng.standard_normal((Mp + 6) * strideA + 64).astype(np.float32)
    rowA[M:] = rowA[0]
    if poison:
        rowA[M:] = (Mp + 5) * strideA
        Abuf[(Mp + 5) * strideA:] = 1e6
    ncc = Np // 32
    if bmode == 0:
        colB = (rng.permutation(kc + 2)[:kc] * 32).astype(np.int64)
        strideB = (kc + 2) * 32 + 8
        rowB = (rng.permutation(Np + 3)[:Np] * strideB).astype(np.int64)
        Bbuf = rng.standard_normal((Np + 4) * strideB + 64).astype(np.float32)
        rowB[N:] = rowB[0]
        if poison:
            rowB[N:] = (Np + 3) * strideB
            Bbuf[(Np + 3) * strideB:] = 1e6
    else:
        colB = (rng.permutation(ncc + 2)[:ncc] * 32).astype(np.int64)
        strideB = (ncc + 2) * 32 + 4
        rowB = (rng.permutation(K + 3)[:K] * strideB).astype(np.int64)
        Bbuf = rng.standard_normal((K + 3) * strideB + 64).astype(np.float32)
    colC = (rng.permutation(ncc + 1)[:ncc] * 32).astype(np.int64)
    strideC = (ncc + 1) * 32 + (2 if odd else 0)
    shift = 1 if odd else 0
    rowC = (rng.permutation(Mp + 2)[:Mp] * strideC + shift).astype(np.int64)
    rowC[M:] = rowC[0]
    plane = (Mp + 2) * strideC + 32
    Cbuf = np.full(plane * splitK + 64, SENTINEL, dtype=np.float32)
    rowR = (rng.permutation(Mp + 2)[:Mp] * strideC + shift).astype(np.int64)
    Rbuf = rng.standard_normal(plane + 64).astype(np.float32)
    partial = splitK > 1
    cps = chunksPerSplit if chunksPerSplit is not None else -(-kc // splitK)
    assert (splitK - 1) * cps < kc <= splitK * cps
    c = SimpleNamespace(
        M=M, N=N, K=K, tilesM=tilesM, tilesN=tilesN, splitK=splitK, chunksPerSplit=cps, splitStride=plane,
        alpha=alpha, act=0 if partial else act, bmode=bmode, Abuf=Abuf, Bbuf=Bbuf, Cbuf=Cbuf, Rbuf=Rbuf,
        biasv=rng.standard_normal(Np).astype(np.float32), rowA=rowA, colA=colA, rowB=rowB, colB=colB, rowC=rowC, colC=colC, rowR=rowR,
        use_bias=bias and not partial, use_res=(residual or inplace) and not partial, baseC=shift, baseR=shift,
        inplace=inplace and not partial)
    if c.inplace:       # the residual lies where the output goes
        _scatter(c.Cbuf, 0, rowC[:M], colC, N, rng.standard_normal((M, N)).astype(np.float32))
    return c
