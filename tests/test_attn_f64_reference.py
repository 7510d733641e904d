"""tests/_attn_f64.py on its own, without a GPU: the ordered-uint image of a float against the kernels' definition, the float64
reference of the fused P.V against torch's float64 softmax, its fp32 yardstick against the derived bound on every case shape of
tests/test_gpu_attention_fused.py, reference-side mutations against the same bound, and the descriptor / flag values the GPU tests
bind against the headers."""
import os
import re

import numpy as np
import pytest

import _attn_f64 as a64
import _gemm_f64 as g64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILES = [(128, 64), (128, 128)]
MATRIX = [(bm, bn, wide, K, sk, cps, alpha) for bm, bn in TILES for wide in (0, 1) for K, sk, cps in a64.KSPLITS for alpha in (1.0, 0.5)]
MATRIX_IDS = [f"{bm}x{bn}-N{'2bn' if w else 'bn+8'}-K{K}-split{sk}-alpha{al}" for bm, bn, w, K, sk, cps, al in MATRIX]
_cases = {}


def _case(i):
    if i not in _cases:
        c = a64.aexp_case(*MATRIX[i])
        mx = a64.host_rowmax(c)
        _cases[i] = (c, mx, a64.aexp_ref64(c, mx))
    return _cases[i]


# ---- ordered / from_ordered ---------------------------------------------------------------------------------------------------------
def test_ordered_is_the_kernels_definition():
    """csrc/gather_gemm.hip f32_ordered / f32_from_ordered, restated here, must still read as they did"""
    src = open(os.path.join(ROOT, "video-subtitle-remover_amd", "csrc", "gather_gemm.hip")).read()
    assert re.search(r"f32_ordered\(float f\)\s*\{\s*const unsigned int b = __float_as_uint\(f\);\s*"
                     r"return \(b & 0x80000000u\) \? ~b : \(b \| 0x80000000u\);", src)
    assert re.search(r"f32_from_ordered\(unsigned int e\)\s*\{\s*return __uint_as_float\(\(e & 0x80000000u\) \? \(e & 0x7fffffffu\) : ~e\);", src)


def test_ordered_round_trip_and_order():
    rng = np.random.default_rng(1)
    special = np.array([0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45, 1.1754942e-38, -1.1754942e-38, 1.0, -1.0, 3.4028235e38, -3.4028235e38],
                       np.float32)
    bits = rng.integers(0, 1 << 32, 20000, dtype=np.uint64).astype(np.uint32)
    x = np.concatenate([special, bits.view(np.float32)])
    back = a64.from_ordered(a64.ordered(x))
    assert np.array_equal(back.view(np.uint32), x.view(np.uint32))                     # every bit pattern, NaN payloads included
    assert np.array_equal(a64.ordered(a64.from_ordered(bits)), bits)
    finite = np.unique(x[np.isfinite(x) | np.isinf(x)])                               # sorted, no NaN; -0.0 == 0.0 collapses to one
    finite = finite[finite != 0]
    finite = np.sort(np.concatenate([finite, np.array([-0.0], np.float32)]))
    u = a64.ordered(finite).astype(np.int64)
    assert np.all(np.diff(u) > 0), "ordered() is not strictly increasing over increasing floats"
    one = lambda v: int(a64.ordered(np.array([v], np.float32))[0])
    assert one(-0.0) + 1 == one(0.0)                                                  # -0.0 sorts just below +0.0
    assert one(-np.inf) == 0x007FFFFF > 0                                              # 0 lies below the image of every number
    assert np.isnan(a64.from_ordered(np.zeros(1, np.uint32)))[0], "0 (the engine's memset) decodes to a NaN"
    assert np.all(a64.ordered(x[~np.isnan(x)]) >= one(-np.inf))


def test_descriptor_and_flags_match_the_header():
    """what the GPU tests bind: the GGProblem mirror of vsr_amd._lib field by field, the flag values, the entry points"""
    hdr = open(os.path.join(ROOT, "include", "vsr_hip.h")).read()
    body = re.search(r"typedef struct GGProblem \{(.*?)\} GGProblem;", hdr, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        m = re.match(r"(const float\*|float\*|const int32_t\*|int32_t|int64_t|float) (.+)", decl)
        assert m, decl
        kind = "p" if "*" in m.group(1) else {"int32_t": "i", "int64_t": "l", "float": "f"}[m.group(1)]
        fields += [(n.strip(), kind) for n in m.group(2).split(",")]
    import ctypes as C

    from vsr_amd import _lib

    kinds = {C.c_void_p: "p", C.c_int32: "i", C.c_int64: "l", C.c_float: "f"}
    assert [(n, kinds[t]) for n, t in _lib.GGProblem._fields_] == fields
    assert re.search(r"VSR_ACT_ROW_MAX = 0x400, VSR_ACT_A_EXP = 0x800", hdr) and (a64.ACT_ROW_MAX, a64.ACT_A_EXP) == (0x400, 0x800)
    assert re.search(r"#define VSR_VARIANT_A_EXP 0x100\b", hdr) and a64.VARIANT_A_EXP == 0x100
    assert (g64.ACT_OUT_SPLIT, g64.ACT_POST_RELU) == (0x100, 0x200)
    for proto in ("int vsr_run_gather_gemm_variant(const GGProblem* probs, int nprobs, int tile_cfg, int bmode, int variant, void* stream);",
                  "int vsr_run_gather_gemm_flagged(const GGProblem* probs, int nprobs, int tile_cfg, int bmode, int variant, uint32_t* range_flag_out,",
                  "int vsr_gemm_plan_create(const GGProblem* probs, int nprobs, int tile_cfg, int bmode, int variant, vsr_gemm_plan_t** out);",
                  "int vsr_gg_resident_blocks(int tile_cfg, int bmode, int variant);", "int vsr_run_softmax(const SMProblem* probs, int nprobs, void* stream);"):
        assert proto in " ".join(hdr.split()), proto


# ---- ROW_MAX ------------------------------------------------------------------------------------------------------------------------
def test_rowmax_ref_reads_the_stored_cells():
    rng = np.random.default_rng(2)
    c = g64.make_case(rng, 150, 72, 64, 128, 64, 0, bias=True, residual=False)
    got = c.Cbuf.copy()
    vals = rng.standard_normal((c.M, c.N)).astype(np.float32)
    vals[3] = -np.abs(vals[3]) - 1
    vals[3, 17] = -0.0
    got[g64.written_cells(c)[0]] = vals
    got[got == g64.SENTINEL] = 1e30                                     # cells outside the problem never count
    rm = a64.rowmax_ref(c, got)
    assert rm.shape == (c.M,) and np.array_equal(rm, vals.max(1))
    assert rm[3] == 0 and np.signbit(rm[3]) and a64.ordered(rm[3:4])[0] == 0x7FFFFFFF


# ---- A_EXP --------------------------------------------------------------------------------------------------------------------------
def test_regimes_are_what_they_say():
    c, mx, r = _case(MATRIX.index((128, 64, 0, 160, 3, 2, 1.0)))
    S = a64.scores_of(c).astype(np.float64)
    x = S - mx[:, None]
    seen = set()
    for m in range(c.M):
        reg = a64.regime_of(m)
        seen.add(reg)
        others = np.delete(x[m], np.argmax(S[m]))
        if reg == "equal":
            assert np.all(x[m] == 0)
        elif reg == "one-hot":
            assert others.max() < -195 and np.float32(2.0) ** np.float32(others.max()) == 0
        elif reg == "offset":
            assert abs(abs(mx[m]) - 30000) < 20 and others.min() > -30
        elif reg == "flush":
            assert mx[m] == 0 and others.max() <= -120 and others.min() >= -149 and (others < -126).any() and (others > -126).any()
        elif reg == "max-first":
            assert np.argmax(S[m]) < 32
        elif reg == "max-last":
            assert np.argmax(S[m]) >= c.K - 32
    assert seen == set(a64.REGIMES)
    assert {a64.regime_of(m) for m in range(128, c.M)} == set(a64.REGIMES), "the ragged second tile holds every regime"


@pytest.mark.parametrize("i", range(len(MATRIX)), ids=MATRIX_IDS)
def test_aexp_ref64_is_softmax_and_recombines(i):
    c, mx, r = _case(i)
    want = a64.softmax64(c)
    assert np.all(np.abs(r.unsplit - want) <= 1e-12 * np.maximum(1.0, np.abs(want)))
    whole = r.planes.sum(0) / r.sums.sum(0)[:, None]
    assert np.all(np.abs(whole - r.unsplit) <= 1e-12 * np.maximum(1.0, np.abs(want)))
    assert r.planes.shape == (c.splitK, c.M, c.N) and r.sums.shape == (c.splitK, c.M) and np.all(r.sums.sum(0) >= 1.0)
    assert np.all(r.mag * (1 + 1e-12) >= np.abs(r.unsplit) / abs(c.alpha))
    assert np.all(r.bound > 0) and np.all(r.plane_bound > 0) and np.all(r.sum_bound > 0)


@pytest.mark.parametrize("i", range(len(MATRIX)), ids=MATRIX_IDS)
def test_aexp_yardstick_stays_inside_the_bound(i):
    """the longest chain of roundings a correct fp32 evaluation can have lies inside the derived bound, cell by cell; the one-hot
    rows are exact"""
    c, mx, r = _case(i)
    rows, unsplit, planes, sums = a64.aexp_yardstick32(c, mx)
    assert rows.size * c.N >= 4096 and planes.dtype == np.float32 and sums.dtype == np.float32
    perr = np.abs(planes.astype(np.float64) - r.planes[:, rows])
    assert np.all(perr <= r.plane_bound[:, rows]), f"planes beyond the bound by {np.max(perr / r.plane_bound[:, rows]):.2f}x"
    serr = np.abs(sums.astype(np.float64) - r.sums[:, rows])
    assert np.all(serr <= r.sum_bound[:, rows]), f"sums beyond the bound by {np.max(serr / r.sum_bound[:, rows]):.2f}x"
    if c.splitK == 1:
        err = np.abs(unsplit.astype(np.float64) - r.unsplit[rows])
        assert np.all(err <= r.bound[rows]), f"yardstick beyond the bound by {np.max(err / r.bound[rows]):.2f}x"
        assert err.max() > 0
        hot = [j for j, m in enumerate(rows) if a64.regime_of(m) == "one-hot"]
        k = np.argmax(a64.scores_of(c)[rows[hot]], axis=1)
        assert np.array_equal(unsplit[hot], a64.values_of(c)[k] * np.float32(c.alpha))


def _exceeds(err, bound):
    return bool(np.any(~(err <= bound)))           # a NaN exceeds


def test_reference_side_mutations_leave_the_bound():
    """what a subtly wrong kernel would produce, formed on the reference side, is outside the bound on at least one case each --
    and for the sums of a split product on every case"""
    hits = {"chunk-missing-from-sum": 0, "neighbour-row-maximum": 0, "neighbour-row-maximum-sums": 0, "sums-of-N-tile-1": 0}
    for i in range(len(MATRIX)):
        c, mx, r = _case(i)
        E, B = r.E, r.B
        # one 32-chunk (the first) left out of a row sum
        if c.K > 32:
            l = E[:, 32:].sum(1)
            mut = float(c.alpha) * (E @ B) / l[:, None]
            hits["chunk-missing-from-sum"] += _exceeds(np.abs(mut - r.unsplit), r.bound)
            assert _exceeds(E[:, :32].sum(1), r.sum_bound[0])          # the first slice's sum is short by exactly that chunk
        # the maximum of the neighbouring row: the quotient cancels it wherever nothing overflows, planes and sums do not
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            r2 = a64.aexp_ref64(c, np.roll(mx, 1))
        hits["neighbour-row-maximum"] += _exceeds(np.abs(r2.unsplit - r.unsplit), r.bound)
        if c.splitK > 1:
            bad = _exceeds(np.abs(r2.sums - r.sums), r.sum_bound) and _exceeds(np.abs(r2.planes - r.planes), r.plane_bound)
            hits["neighbour-row-maximum-sums"] += bad
            assert bad
            # the sums of N-tile 1 of a split product: that tile never formed them
            hits["sums-of-N-tile-1"] += _exceeds(np.abs(np.zeros_like(r.sums) - r.sums), r.sum_bound)
    assert all(v > 0 for v in hits.values()), hits


# ---- the refusals of the kernel-level entry points: argument errors come before the device is asked for ---------------------------
def test_fused_flag_misuse_is_an_argument_error(built_lib):
    """every misuse tests/test_gpu_attention_fused.py tries on the GPU, here with descriptors whose pointers are never followed:
    VSR_ERR_ARG whether or not a device is present; the same descriptors without the misuse get past the argument checks"""
    import ctypes as C

    lib, T = built_lib.lib, built_lib
    V_AEXP = 1 | a64.VARIANT_A_EXP

    def prob(**kw):
        p = T.GGProblem()
        p.M, p.N, p.K, p.tilesM, p.tilesN, p.splitK, p.chunksPerSplit, p.alpha = 70, 40, 64, 1, 1, 1, 2, 1.0
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def rc(p, tile, bmode, variant):
        return lib.vsr_run_gather_gemm_variant(C.byref(p), 1, tile, bmode, variant, None)

    fake = 0x1000
    served = T.VSR_ERR_NOGPU if lib.vsr_device_count() <= 0 else None
    for v in (1, 2, 4, 5, 6, 7):
        assert rc(prob(act=a64.ACT_ROW_MAX, R=fake), T.TILE_128x64, 0, v) == T.VSR_ERR_ARG
    assert rc(prob(act=a64.ACT_ROW_MAX, R=fake), T.TILE_128x64, 1, 3) == T.VSR_ERR_ARG
    assert rc(prob(act=a64.ACT_ROW_MAX, R=fake, splitK=2, chunksPerSplit=1), T.TILE_128x64, 0, 3) == T.VSR_ERR_ARG
    assert rc(prob(act=a64.ACT_ROW_MAX, R=None), T.TILE_128x64, 0, 3) == T.VSR_ERR_ARG
    assert "ROW_MAX" in T.last_error()
    for v in (1, 3, 4):
        assert rc(prob(act=a64.ACT_A_EXP, bias=fake), T.TILE_128x64, 1, v) == T.VSR_ERR_ARG
    assert rc(prob(act=a64.ACT_A_EXP, bias=None), T.TILE_128x64, 1, V_AEXP) == T.VSR_ERR_ARG
    assert rc(prob(act=a64.ACT_A_EXP, bias=fake, R=None, splitK=2, chunksPerSplit=1), T.TILE_128x64, 1, V_AEXP) == T.VSR_ERR_ARG
    assert "A_EXP" in T.last_error()
    assert rc(prob(), T.TILE_128x64, 0, V_AEXP) == T.VSR_ERR_ARG
    for tile in (T.TILE_256x32, T.TILE_256x64, T.TILE_256x128, T.TILE_256x256):
        assert rc(prob(), tile, 1, V_AEXP) == T.VSR_ERR_ARG
    flag, plan = C.c_uint32(7), C.c_void_p()
    assert lib.vsr_run_gather_gemm_flagged(C.byref(prob(act=a64.ACT_ROW_MAX, R=fake)), 1, T.TILE_128x64, 0, 4, C.byref(flag), None) == T.VSR_ERR_ARG
    for v in (1, 2, 4):
        assert lib.vsr_gemm_plan_create(C.byref(prob(act=a64.ACT_ROW_MAX, R=fake)), 1, T.TILE_128x64, 0, v, C.byref(plan)) == T.VSR_ERR_ARG
    assert lib.vsr_gemm_plan_create(C.byref(prob(act=a64.ACT_A_EXP, bias=fake)), 1, T.TILE_128x64, 1, 1, C.byref(plan)) == T.VSR_ERR_ARG
    assert flag.value == 7 and plan.value is None
    if served is not None:              # without a device the well-formed launches get as far as the device check, and no further
        assert rc(prob(act=a64.ACT_ROW_MAX, R=fake), T.TILE_128x64, 0, 3) == served
        assert rc(prob(act=a64.ACT_A_EXP, bias=fake), T.TILE_128x64, 1, V_AEXP) == served
        assert rc(prob(act=a64.ACT_A_EXP, bias=fake, R=fake, splitK=2, chunksPerSplit=1), T.TILE_128x128, 1, V_AEXP) == served
