"""Float64 references of the two halves of the fused attention (include/vsr_hip.h: VSR_ACT_ROW_MAX on the score GEMM, VSR_ACT_A_EXP on
the P.V GEMM), the fp32 one-operation-at-a-time yardstick of the second half and the derived element-wise bounds.  CPU only: numpy,
torch on the CPU and tests/_gemm_f64.py, whose cases (make_case), device bytes (physical), store set (written_cells) and plain-GEMM
bound (bound) are used for everything that is a plain GEMM.

An A_EXP *case* is a KN case of _gemm_f64: its A operand holds the SCORES s[m][k] (K = keys), its B operand V.  The kernel is handed
fp32 row maxima mx[m] and forms

    e[m][k] = 2^(s[m][k] - mx[m])                       C[m][n] = alpha * sum_k e[m][k] b[k][n] / l[m],   l[m] = sum_k e[m][k]

(splitK > 1: the planes alpha * sum_{k in slice} e b stay unnormalised and the slices' sums l_s[m] go to the row-sum array).

THE BOUND (u = 2^-24, first order in u, derived before anything was measured)

  one weight.  The kernel computes x' = fl(s - mx) and e' = v_exp_f32(x').
    * |x' - x| <= u |x| (one fp32 subtraction), and d/dx 2^x = ln2 2^x: the weight moves by a factor ln2 u |x|;
    * v_exp_f32 is accurate to 1 ulp, i.e. 2 u relative ("V_EXP_F32: base-2 exponential, 1 ULP accuracy, denormals flushed" -- AMD
      GCN3 / Vega / CDNA instruction set architecture reference guides, VOP1 opcode table; the same figure LLVM's AMDGPU backend
      relies on when it lowers exp2 to the instruction for results that are not denormal);
    * a result below 2^-126 is flushed to zero: an absolute PHI = 2^-126 on the weight.
    So |e' - e| <= eta e + PHI with eta = (ln2 |x| + 2) u.
  a row sum of Ks weights, in any order of addition: every one of the Ks - 1 additions rounds a partial sum no larger than l, so
    |l' - l| <= sum_k (eta_k e_k + PHI) + (Ks - 1) u l                                                     (sum_bound)
  a plane (or the numerator of an unsplit product) of Ks products: the weights' own errors times |b|, then the family's
    accumulation term -- Ks - 1 additions and one product rounding on the longest path, alpha, the factor 1 / l, and the one
    division that forms it: Ks + 3 <= Ks + 4 roundings of values no larger than the sum of magnitudes.  A product or a result below
    2^-126 may be flushed: (Ks + 1) PHI absolute.
    |P' - P| <= |alpha| [ sum_k (eta_k e_k + PHI) |b_k| + (Ks + 4) u sum_k e_k |b_k| + (Ks + 1) PHI ]        (plane_bound)
  the quotient C = P / l (unsplit): d(P / l) = dP / l - (P / l) dl / l, and |P / l| <= |alpha| mag with mag = sum e |b| / l:
    |C' - C| <= plane_bound / l + |alpha| mag sum_bound / l                                                  (bound)
  (the division's own rounding is inside the K + 4 above).

All three scale with per-cell magnitudes of the row in question, so a row of small values beside a row of large ones is held to its
own scale, and a wrong maximum, a lane's share missing from l or another tile's sums are far outside."""
from types import SimpleNamespace

import numpy as np
import torch

import _gemm_f64 as g64
from _replay import _gather, _scatter

ACT_ROW_MAX, ACT_A_EXP, VARIANT_A_EXP = 0x400, 0x800, 0x100
U32 = g64.U32
PHI = 2.0 ** -126
LN2 = float(np.log(2.0))
EXP_ULPS = 1            # v_exp_f32: 1 ulp = 2 u relative (see the module text)


# ---- the kernels' monotone unsigned image of a float (csrc/gather_gemm.hip f32_ordered / f32_from_ordered) ------------------------
def ordered(f):
    b = np.ascontiguousarray(f, dtype=np.float32).view(np.uint32)
    return np.where((b & np.uint32(0x80000000)) != 0, ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def from_ordered(u):
    u = np.ascontiguousarray(u).view(np.uint32)
    return np.where((u & np.uint32(0x80000000)) != 0, u & np.uint32(0x7FFFFFFF), ~u).astype(np.uint32).view(np.float32)


# ---- ROW_MAX ------------------------------------------------------------------------------------------------------------------------
def stored_rows(case, got):
    """[M][N] fp32: the cells of the problem as they lie in `got` (plane 0)"""
    return got[g64.written_cells(case)[0]]


def rowmax_ref(case, got):
    """[M] fp32: the maximum over n < N of the stored fp32 C cell of every row m < M (bias included: the cell is what the epilogue
    formed).  The kernel's array must hold exactly ordered() of these."""
    return stored_rows(case, got).max(axis=1)


# ---- A_EXP --------------------------------------------------------------------------------------------------------------------------
def scores_of(case):
    return _gather(case.Abuf, 0, np.asarray(case.rowA[:case.M], np.int64), case.colA, case.K)


def values_of(case):
    return _gather(case.Bbuf, 0, np.asarray(case.rowB[:case.K], np.int64), case.colB, case.N)


def set_scores(case, S):
    _scatter(case.Abuf, 0, np.asarray(case.rowA[:case.M], np.int64), case.colA, case.K, S)


def set_values(case, V):
    _scatter(case.Bbuf, 0, np.asarray(case.rowB[:case.K], np.int64), case.colB, case.N, V)


def aexp_ref64(case, rowmax):
    """float64 evaluation of an A_EXP case on the stored fp32 scores and the fp32 maxima handed to the kernel (rowmax [M]).
    Returns unsplit [M][N], planes [splitK][M][N] (unnormalised, alpha applied), sums [splitK][M], mag [M][N] = sum e |b| / sum e,
    and the derived bounds: bound [M][N] (unsplit), plane_bound [splitK][M][N], sum_bound [splitK][M] (absolute; divide by sums for
    the relative form)."""
    S = scores_of(case).astype(np.float64)
    B = values_of(case).astype(np.float64)
    a = abs(float(case.alpha))
    x = S - np.asarray(rowmax, np.float32).astype(np.float64)[:, None]
    E = np.exp2(x)
    eta = (LN2 * np.abs(x) + 2 * EXP_ULPS) * U32
    dE = eta * E + PHI                                        # |e' - e| of every weight
    absB = np.abs(B)
    planes, sums, pb, sb = [], [], [], []
    for s, k0, k1 in g64._slices(case):
        ks = k1 - k0
        Es, Bs = E[:, k0:k1], B[k0:k1]
        planes.append(float(case.alpha) * (Es @ Bs))
        sums.append(Es.sum(1))
        pb.append(a * (dE[:, k0:k1] @ absB[k0:k1] + (ks + 4) * U32 * (Es @ absB[k0:k1]) + (ks + 1) * PHI))
        sb.append(dE[:, k0:k1].sum(1) + (ks - 1) * U32 * sums[-1])
    K = case.K
    l = E.sum(1)
    num_mag = E @ absB
    mag = num_mag / l[:, None]
    whole_pb = a * (dE @ absB + (K + 4) * U32 * num_mag + (K + 1) * PHI)
    whole_sb = dE.sum(1) + (K - 1) * U32 * l
    return SimpleNamespace(unsplit=float(case.alpha) * (E @ B) / l[:, None], planes=np.stack(planes), sums=np.stack(sums), mag=mag,
                           bound=whole_pb / l[:, None] + a * mag * (whole_sb / l)[:, None],
                           plane_bound=np.stack(pb), sum_bound=np.stack(sb), E=E, B=B)


def aexp_yardstick32(case, rowmax, rows=None):
    """The same formula one fp32 operation at a time: x = fl(s - mx), e = fp32 exp2(x), acc = fl(acc + fl(e_k b_k)) one product after
    the other, l = fl(l + e_k) in sequence, then fl(acc * alpha) and ONE division by l (splitK 1); planes fl(acc * alpha) and the
    slices' sums otherwise.  rows: the row subsample (default yardstick_rows: at least 4096 cells).
    Returns (rows, unsplit [rows][N] or None, planes [splitK][rows][N], sums [splitK][rows]), all fp32."""
    rows = yardstick_rows(case) if rows is None else np.asarray(rows, np.int64)
    S = scores_of(case)[rows]
    B = values_of(case)
    mx = np.asarray(rowmax, np.float32)[rows]
    alpha = np.float32(case.alpha)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        x = S - mx[:, None]
        E = np.exp2(x)
        assert x.dtype == np.float32 and E.dtype == np.float32
        planes, sums = [], []
        for s, k0, k1 in g64._slices(case):
            acc = np.zeros((len(rows), case.N), np.float32)
            l = np.zeros(len(rows), np.float32)
            for k in range(k0, k1):
                acc = acc + E[:, k, None] * B[None, k, :]
                l = l + E[:, k]
            planes.append(acc * alpha)
            sums.append(l)
        unsplit = planes[0] / sums[0][:, None] if case.splitK == 1 else None
    return rows, unsplit, np.stack(planes), np.stack(sums)


def yardstick_rows(case, min_cells=4096):
    """every row while the problem is small (the cases of the suite), else _gemm_f64's evenly spread subsample of >= min_cells cells"""
    if case.M * case.N <= 16 * min_cells:
        return np.arange(case.M)
    return g64.yardstick_rows(case, min_cells)


# ---- the case matrix of tests/test_gpu_attention_fused.py section 3 (built here so that the CPU test holds the yardstick and the
# mutations against the same cases) ------------------------------------------------------------------------------------------------
REGIMES = ("smooth", "equal", "one-hot", "offset", "flush", "max-first", "max-last")
KSPLITS = [(32, 1, None), (96, 1, None), (160, 1, None), (96, 2, 2), (160, 3, 2)]          # K, splitK, chunksPerSplit


def regime_of(m):
    return REGIMES[m % len(REGIMES)]


def regime_scores(rng, M, K):
    """[M][K] fp32 scores, row m in regime m % 7 (every regime meets both M tiles and many staging lanes):
    smooth: N(0, 3^2).  equal: one value.  one-hot: N(0, 1) with one score 200 above the rest (2^-195: every other weight is
    exactly 0).  offset: +-30000 + N(0, 2^2) (wrong at once if the maximum is not subtracted in fp32 before the exponential).
    flush: one score 0, the others in [-149, -120] (weights around the flush threshold 2^-126).  max-first / max-last: smooth
    with the maximum planted in the first chunk / in the last chunk (of the last slice)."""
    S = (rng.standard_normal((M, K)) * 3).astype(np.float32)
    for m in range(M):
        r = regime_of(m)
        if r == "equal":
            S[m] = np.float32(1.25 + m / 64.0)
        elif r == "one-hot":
            S[m] = rng.standard_normal(K).astype(np.float32)
            S[m, (5 * m + 3) % K] = np.float32(S[m].max() + 200.0)
        elif r == "offset":
            S[m] = (np.float32(30000.0 if (m // len(REGIMES)) % 2 else -30000.0) + rng.standard_normal(K) * 2).astype(np.float32)
        elif r == "flush":
            S[m] = rng.uniform(-149.0, -120.0, K).astype(np.float32)
            S[m, (3 * m + 1) % K] = 0.0
        elif r == "max-first":
            S[m, (m // len(REGIMES)) % 32] = np.float32(S[m].max() + 8.0)
        elif r == "max-last":
            S[m, K - 1 - (m // len(REGIMES)) % 32] = np.float32(S[m].max() + 8.0)
    return S


def aexp_case(bm, bn, wideN, K, splitK, cps, alpha, seed=0):
    """one case of the matrix: M = bm + 37 (a ragged second M tile), N = bn + 8 or 2 bn (two N tiles), regime scores"""
    rng = np.random.default_rng(7000 + bm + 3 * bn + 11 * K + 101 * splitK + 1009 * wideN + seed)
    M, N = bm + 37, (2 * bn if wideN else bn + 8)
    c = g64.make_case(rng, M, N, K, bm, bn, 1, splitK=splitK, chunksPerSplit=cps, bias=False, act=0, residual=False, alpha=alpha)
    set_scores(c, regime_scores(rng, M, K))
    c.act = ACT_A_EXP
    return c


def host_rowmax(case):
    """[M] fp32: the exact maximum of the stored scores of every row"""
    return scores_of(case).max(axis=1)


def softmax64(case):
    """torch's float64 softmax(S ln2) @ B times alpha: the operation itself, for the self-check of aexp_ref64.  The row's first
    score is taken off before the product with ln2 (exact in float64, and softmax does not see it): at scores of 30000 the
    rounding of S ln2 alone is 3e-12 of every weight, which is the check's own error and not the reference's."""
    S = torch.from_numpy(scores_of(case)).double()
    S = S - S[:, :1]
    return float(case.alpha) * (torch.softmax(S * LN2, -1) @ torch.from_numpy(values_of(case)).double()).numpy()
