"""The gather-GEMM family one launch at a time against a float64 reference (tests/_gemm_f64.py): tile hand-over inside a persistent
workgroup, every branch of the hand-written epilogues, the range guard, the resident launch list and the softmax rows.

What every GEMM test asserts about every problem of its launch (`_check`):
  B1  |got - ref64| <= (K + 4) 2^-24 S on every written cell (+ 2^-21 |ref64| in split format) -- derived, see _gemm_f64.bound;
  B2  on a fixed subsample of rows, max and rms of |got - ref64| are at most twice those of the fp32 one-product-at-a-time
      evaluation of the same operand model (the matrix cores add 2 or 16 products before they touch the accumulator: they round
      less often).  The measured ratios are printed (`RATIO ...`) and kept in profiles/gemm_f64_ratios.md;
  B3  every byte outside the written cells is what it was before the launch."""
import ctypes as C

import numpy as np
import pytest
import torch

import _gemm_f64 as g64

pytestmark = pytest.mark.gpu

OUT_SPLIT, POST_RELU = g64.ACT_OUT_SPLIT, g64.ACT_POST_RELU
TILES = {"128x128": (0, 128, 128), "256x32": (1, 256, 32), "256x64": (2, 256, 64), "128x64": (3, 128, 64), "256x128": (4, 256, 128),
         "256x256": (5, 256, 256)}


# ---- launching ----------------------------------------------------------------------------------------------------------------------
class _Launch:
    """the device side of a list of cases for one variant: buffers as the variant reads them, descriptors, C before and after"""

    def __init__(self, lib, device, cases, variant):
        self.lib, self.cases, self.variant = lib, cases, variant
        model = g64.operand_model(variant)
        self.probs = (lib.GGProblem * len(cases))()
        self.keep, self.dC, self.before = [], [], []
        for p, c in zip(self.probs, cases):
            ph = g64.physical(c, model)

            def dev(a, base=0):          # `base` floats in front: the pointer handed over lies 4 * base bytes past a 16-byte boundary
                t = torch.from_numpy(np.concatenate([np.zeros(base, np.float32), a]) if base else a).to(device)
                assert t.data_ptr() % 16 == 0
                return t

            def tab(a):
                return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(device)

            dA, dB, dC, dbias = dev(ph.A), dev(ph.B), dev(ph.C, c.baseC), dev(ph.bias)
            t = {k: tab(getattr(c, k)) for k in ("rowA", "colA", "rowB", "colB", "rowC", "colC", "rowR")}
            p.A, p.B, p.C = dA.data_ptr(), dB.data_ptr(), dC.data_ptr() + 4 * c.baseC
            p.bias = dbias.data_ptr() if c.use_bias else None
            p.rowA, p.colA, p.rowB, p.colB = (t[k].data_ptr() for k in ("rowA", "colA", "rowB", "colB"))
            p.rowC, p.colC = t["rowC"].data_ptr(), t["colC"].data_ptr()
            p.R = p.rowR = None
            if c.use_res and c.inplace:
                p.R, p.rowR = p.C, p.rowC
            elif c.use_res:
                dR = dev(ph.R, c.baseR)
                self.keep.append(dR)
                p.R, p.rowR = dR.data_ptr() + 4 * c.baseR, t["rowR"].data_ptr()
            p.M, p.N, p.K, p.tilesM, p.tilesN = c.M, c.N, c.K, c.tilesM, c.tilesN
            p.splitK, p.chunksPerSplit, p.act, p.alpha, p.splitStride = c.splitK, c.chunksPerSplit, c.act, c.alpha, c.splitStride
            self.keep += [dA, dB, dbias, t]
            self.dC.append(dC)
            self.before.append(ph.C)
        torch.cuda.synchronize()

    def tiles(self):
        return sum(c.tilesM * c.tilesN * c.splitK for c in self.cases)

    def outputs(self):
        torch.cuda.synchronize()
        return [d.cpu().numpy()[c.baseC:] for d, c in zip(self.dC, self.cases)]

    def reset(self):
        for d, c, b in zip(self.dC, self.cases, self.before):
            d[c.baseC:].copy_(torch.from_numpy(b))
        torch.cuda.synchronize()

    def run(self, tile_cfg, bmode, variant=None):
        v = self.variant if variant is None else variant
        self.lib.check(self.lib.lib.vsr_run_gather_gemm_variant(self.probs, len(self.cases), tile_cfg, bmode, v, None))
        return self.outputs()

    def run_flagged(self, tile_cfg, bmode):
        flag = C.c_uint32(0xFFFFFFFF)
        self.lib.check(self.lib.lib.vsr_run_gather_gemm_flagged(self.probs, len(self.cases), tile_cfg, bmode, self.variant, C.byref(flag), None))
        return self.outputs(), flag.value


def _same_bytes(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _check(c, variant, got, before, what, key=None, b2=True):
    """B1, B2, B3 of one problem; `key` names the kernel in the printed ratio line"""
    model = g64.operand_model(variant)
    r = g64.reference64(c, model)
    out_split = bool(c.act & OUT_SPLIT) and c.splitK == 1
    err = np.abs(g64.decode_output(c, got, r.cells) - r.ref)
    b = g64.bound(r, out_split)
    worst = np.unravel_index(np.argmax(err - b), err.shape)
    assert np.all(err <= b), f"{what}: |got - ref64| = {err[worst]:.3e} > bound {b[worst]:.3e} at (plane, m, n) = {worst}"
    rows = g64.yardstick_rows(c)
    assert rows.size * c.N >= min(4096, c.M * c.N)
    yerr = np.abs(g64.yardstick32(c, model, rows, out_split).astype(np.float64) - r.ref[:, rows])
    gerr = err[:, rows]
    gmax, ymax, grms, yrms = gerr.max(), yerr.max(), np.sqrt(np.mean(gerr ** 2)), np.sqrt(np.mean(yerr ** 2))
    rmax, rrms = gmax / ymax if ymax > 0 else 0.0, grms / yrms if yrms > 0 else 0.0
    print(f"RATIO | {key or what} | {what} | max {gmax:.3e}/{ymax:.3e} = {rmax:.3f} | rms {grms:.3e}/{yrms:.3e} = {rrms:.3f}")
    if b2:
        assert gmax <= 2 * ymax, f"{what}: max error {gmax:.3e} > 2 x yardstick {ymax:.3e}"
        assert grms <= 2 * yrms, f"{what}: rms error {grms:.3e} > 2 x yardstick {yrms:.3e}"
    assert g64.untouched(c, got, before, r.cells), f"{what}: bytes outside the written cells changed"


def _check_all(L, outs, what, key=None):
    for i, (c, got, before) in enumerate(zip(L.cases, outs, L.before)):
        _check(c, L.variant, got, before, f"{what} problem {i} ({c.M}x{c.N}x{c.K} act {c.act:#x} split {c.splitK})", key)


# ---- D1: tile hand-over -------------------------------------------------------------------------------------------------------------
HANDOVER = [(3, "128x64", 0), (4, "128x64", 0), (7, "128x64", 0), (5, "128x64", 0), (6, "128x64", 0), (3, "128x64", 1), (5, "128x64", 1),
            (3, "128x128", 0), (3, "256x64", 0), (3, "256x32", 0), (6, "256x128", 0), (5, "256x256", 0), (6, "256x256", 0),
            # what the engines launch besides (tests/test_gemm_launch_census.py holds this list to their plans): the generator's fp16 mode on
            # 128x128, LaMa's Fourier stages (KN 128x128), the narrow and first / last convs (256x64, 256x32), P.V in every arithmetic
            (4, "128x128", 0), (4, "256x64", 0), (4, "256x32", 0), (4, "128x64", 1), (4, "128x128", 1),
            (7, "128x128", 0), (7, "256x64", 0), (7, "256x32", 0), (7, "128x64", 1), (7, "128x128", 1),
            (5, "256x64", 0), (5, "256x32", 0), (6, "256x64", 0), (6, "256x32", 0), (6, "128x128", 0), (6, "128x64", 1),
            (3, "128x128", 1)]
# K (chunks 1, 2, 3, 5 and 3 cut 2 + 1), bias, act, residual, alpha, splitK, chunksPerSplit
EPILOGUES = [(32, False, 0, False, 1.0, 1, None), (64, True, 1, True, 1.0, 1, None), (96, True, 2, False, 0.5, 1, None),
             (160, False, POST_RELU, True, 1.0, 1, None), (96, False, 0, False, 1.0, 2, 2)]
_handover_cases = {}


def _handover(bm, bn, bmode, wide, need):
    """five problems of at least `need` tiles together; wide: the first one has five N tiles (the launch takes the single queue)"""
    key = (bm, bn, bmode, wide, need)
    if key not in _handover_cases:
        _handover_cases.clear()                                    # one launch's worth of buffers at a time
        rng = np.random.default_rng(bm * 7 + bn * 3 + bmode + 100 * wide)
        N = bn + 8                                                 # two N tiles: interior tiles and a border of 8 columns
        cases = []
        heights = (32, 64, 96, 160, 256)                           # 256 x 256 tile: tiles of 32 .. 256 rows
        for i, (K, bias, act, res, alpha, splitK, cps) in enumerate(EPILOGUES):
            n = 4 * bn + 8 if (wide and i == 0) else N
            tilesN = -(-n // bn)
            if bm == 256 and bn == 256:                            # equal rows per problem, tilesM above ceil(M / 256)
                per_row = sum(1.0 / h for h in heights)
                rows = need / per_row / tilesN
                tilesM = int(np.ceil(rows / heights[i] / splitK)) + 1
                M = tilesM * heights[i] - 5
            else:
                tilesM = int(np.ceil(need / 5 / tilesN / splitK)) + 1
                M = tilesM * bm - 37 - 8 * i                       # a ragged last tile
            cases.append(g64.make_case(rng, M, n, K, bm, bn, bmode, splitK=splitK, chunksPerSplit=cps, bias=bias, act=act, residual=res,
                                       alpha=alpha, tilesM=tilesM))
        _handover_cases[key] = cases
    return _handover_cases[key]


@pytest.mark.parametrize("variant,tile,bmode", HANDOVER, ids=[f"v{v}-{t}-{'KN' if m else 'NK'}" for v, t, m in HANDOVER])
@pytest.mark.parametrize("wide", [0, 1], ids=["xcd-queues", "single-queue"])     # the outer loop: kernels of one geometry share cases
def test_tile_handover(built_lib, gpu_device, variant, tile, bmode, wide):
    """Every persistent workgroup takes several tiles: problems of 1, 2, 3 and 5 K chunks with four different epilogues and a split-K
    problem of 2 + 1 chunks follow one another in one grouped launch of at least 2.5 tiles per resident workgroup -- the
    double-buffer parity, the control block fetched a tile ahead, the row-table slot and the queue claim are all carried across
    tiles of different problems.  Once with every tilesN <= 4 (per-XCD ranges with stealing), once with a problem of five N tiles
    (the single queue)."""
    cfg, bm, bn = TILES[tile]
    resident = built_lib.lib.vsr_gg_resident_blocks(cfg, bmode, variant)
    assert resident > 0, built_lib.last_error()
    need = int(np.ceil(2.5 * resident))
    cases = _handover(bm, bn, bmode, wide, need)
    assert all(c.tilesN <= 4 for c in cases[1:]) and cases[0].tilesN == (5 if wide else min(4, cases[0].tilesN))
    L = _Launch(built_lib, gpu_device, cases, variant)
    ratio = L.tiles() / resident
    print(f"HANDOVER v{variant} {tile} mode{bmode} wide{wide}: {L.tiles()} tiles / {resident} resident workgroups = {ratio:.2f}")
    assert ratio >= 2.5
    outs = L.run(cfg, bmode)
    _check_all(L, outs, f"hand-over v{variant} {tile} mode{bmode} wide{wide}", key=f"v{variant} {tile} {'KN' if bmode else 'NK'}")
    if variant == 3:        # the one-workgroup-per-tile kernel runs the same MFMA sequence and epilogue: the same bits
        L.reset()
        for a, b in zip(outs, L.run(cfg, bmode, 1)):
            assert _same_bytes(a, b), "variant 3 and variant 1 differ on the same launch"


# ---- D2: epilogue matrix ------------------------------------------------------------------------------------------------------------
EPI_KERNELS = [(1, "128x64", 0, 0), (1, "128x64", 1, 0), (3, "128x64", 0, 0), (3, "128x64", 1, 0), (4, "128x64", 0, 0), (7, "128x64", 0, 0),
               (7, "128x64", 1, 0), (5, "128x64", 0, 0), (5, "128x64", 0, 1), (6, "128x64", 0, 0), (6, "128x64", 0, 1),
               (6, "256x128", 0, 0), (6, "256x128", 0, 1), (5, "256x256", 0, 0), (5, "256x256", 0, 1), (6, "256x256", 0, 0),
               (6, "256x256", 0, 1),
               # (see HANDOVER)
               (4, "128x128", 0, 0), (4, "256x64", 0, 0), (4, "256x32", 0, 0), (4, "128x64", 1, 0), (4, "128x128", 1, 0),
               (7, "128x128", 0, 0), (7, "256x64", 0, 0), (7, "256x32", 0, 0), (7, "128x128", 1, 0),
               (5, "256x64", 0, 0), (5, "256x64", 0, 1), (5, "256x32", 0, 0), (5, "256x32", 0, 1), (5, "128x64", 1, 0), (5, "128x64", 1, 1),
               (6, "256x64", 0, 0), (6, "256x64", 0, 1), (6, "256x32", 0, 0), (6, "256x32", 0, 1), (6, "128x128", 0, 0),
               (6, "128x128", 0, 1), (6, "128x64", 1, 0), (6, "128x64", 1, 1),
               (1, "128x128", 0, 0), (1, "256x64", 0, 0), (1, "256x32", 0, 0), (1, "128x128", 1, 0),
               (3, "128x128", 0, 0), (3, "256x64", 0, 0), (3, "256x32", 0, 0), (3, "128x128", 1, 0)]


def _epilogue_cases(bm, bn, bmode, split_tensors, out_split):
    rng = np.random.default_rng(bm + 5 * bn + bmode + 1000 * out_split)
    M, N, K = 2 * bm + 44, 2 * bn + 8, 96                 # interior tiles and both borders
    osp = OUT_SPLIT if out_split else 0
    mk = lambda **kw: g64.make_case(rng, kw.pop("M", M), kw.pop("N", N), K, bm, bn, bmode, **kw)
    cases = [mk(bias=True, act=a | osp, residual=res) for a in (0, 1, 2, 3) for res in (False, True)]
    cases += [mk(bias=True, act=a | POST_RELU | osp, residual=True) for a in (0, 2)]
    if out_split or not split_tensors:                    # a split-format residual can alias a split-format output only
        cases.append(mk(bias=True, act=1 | POST_RELU | osp, inplace=True))
        cases.append(mk(bias=False, act=0 | POST_RELU | osp, inplace=True))          # LaMa's use: NONE | POST_RELU in place
    cases.append(mk(bias=True, act=osp, residual=False, alpha=0.5))
    cases.append(mk(bias=False, act=1 | osp, residual=True))
    if not out_split:
        # interior tiles only, the C (and fp32 R) pointer 4 bytes past a 16-byte boundary, odd row offsets: the scalar path for
        # alignment alone.  Split-format tensors stay chunk-aligned, so the split-format variants get no residual here.
        cases.append(mk(M=2 * bm, N=2 * bn, bias=True, act=1, residual=not split_tensors, odd=True))
        cases.append(mk(M=2 * bm, N=2 * bn, bias=False, act=2 | (0 if split_tensors else POST_RELU), residual=not split_tensors, odd=True))
        if not split_tensors:
            cases.append(mk(M=2 * bm, N=2 * bn, bias=True, act=3 | POST_RELU, inplace=True, odd=True))
    return cases


@pytest.mark.parametrize("variant,tile,bmode,out_split", EPI_KERNELS,
                         ids=[f"v{v}-{t}-{'KN' if m else 'NK'}{'-outsplit' if o else ''}" for v, t, m, o in EPI_KERNELS])
def test_epilogue_matrix(built_lib, gpu_device, variant, tile, bmode, out_split):
    """every activation with and without a residual, POST_RELU on act 0 and act 2, an in-place residual under POST_RELU, alpha with
    a bias, no bias, split-format output where the variant has it, and interior tiles that are unaligned only -- on each hand-written
    copy of the epilogue"""
    cfg, bm, bn = TILES[tile]
    cases = _epilogue_cases(bm, bn, bmode, g64.operand_model(variant).split_tensors, out_split)
    L = _Launch(built_lib, gpu_device, cases, variant)
    outs = L.run(cfg, bmode)
    _check_all(L, outs, f"epilogue v{variant} {tile} mode{bmode} out_split{out_split}", key=f"v{variant} {tile} {'KN' if bmode else 'NK'} epilogues")
    if variant == 3:
        L.reset()
        for i, (a, b) in enumerate(zip(outs, L.run(cfg, bmode, 1))):
            assert _same_bytes(a, b), f"variant 3 and variant 1 differ on problem {i}"
    if tile == "256x256":   # same k order, same MFMAs: the bytes of the 128 x 64 tile of the same variant
        L.reset()
        for p, c in zip(L.probs, cases):
            p.tilesM, p.tilesN = -(-c.M // 128), -(-c.N // 64)
        for i, (a, b) in enumerate(zip(outs, L.run(TILES["128x64"][0], 0))):
            assert _same_bytes(a, b), f"the 256x256 tile and the 128x64 tile differ on problem {i}"


def test_variant7_is_served_where_its_kernels_exist(built_lib, gpu_device):
    rng = np.random.default_rng(70)
    c = g64.make_case(rng, 40, 40, 32, 256, 128, 0, bias=False, residual=False)
    L = _Launch(built_lib, gpu_device, [c], 7)
    for tile in ("256x128", "256x256"):
        with pytest.raises(built_lib.VsrError):
            L.run(TILES[tile][0], 0)
        assert built_lib.lib.vsr_gg_resident_blocks(TILES[tile][0], 0, 7) == built_lib.VSR_ERR_ARG
    assert built_lib.lib.vsr_gg_resident_blocks(TILES["128x64"][0], 0, 1) == 0
    assert built_lib.lib.vsr_gg_resident_blocks(TILES["128x64"][0], 0, 8) == built_lib.VSR_ERR_ARG
    flag = C.c_uint32(0)
    assert built_lib.lib.vsr_run_gather_gemm_flagged(L.probs, 1, TILES["128x64"][0], 0, 3, C.byref(flag), None) == built_lib.VSR_ERR_ARG


# ---- D3: range guard ----------------------------------------------------------------------------------------------------------------
GUARDED = [(4, "128x64", 0), (7, "128x64", 0), (5, "128x64", 0), (6, "128x64", 0), (6, "256x128", 0), (5, "256x256", 0), (6, "256x256", 0),
           # (see HANDOVER)
           (4, "128x128", 0), (4, "256x64", 0), (4, "256x32", 0), (7, "128x128", 0), (7, "256x64", 0), (7, "256x32", 0),
           (5, "256x64", 0), (5, "256x32", 0), (6, "256x64", 0), (6, "256x32", 0), (6, "128x128", 0),
           (4, "128x64", 1), (4, "128x128", 1), (7, "128x64", 1), (7, "128x128", 1), (5, "128x64", 1), (6, "128x64", 1)]


def _guard_case(bm, bn, bmode, seed, **kw):
    return g64.make_case(np.random.default_rng(seed), 2 * bm + 44, 2 * bn + 8, 96, bm, bn, bmode, bias=True, act=kw.pop("act", 1), residual=True, **kw)


def _poke_A(c, m, k, value):
    c.Abuf[c.rowA[m] + c.colA[k // 32] + k % 32] = value


@pytest.mark.parametrize("variant,tile,bmode", GUARDED, ids=[f"v{v}-{t}{'-KN' if m else ''}" for v, t, m in GUARDED])
def test_range_guard(built_lib, gpu_device, variant, tile, bmode):
    """The range flag of the reduced-precision kernels, through vsr_run_gather_gemm_flagged: (i) benign operands leave it 0 and the
    flagged launch writes the unflagged launch's bytes; (ii) one operand of 1e6 (hi half inf) in a stored row raises it, in an
    interior and in a border tile; (iii) a finite result beyond 65504 raises it in split format only; (iv) 1e6 in the padding
    rows of A and B -- table rows m >= M, n >= N (KN: of A alone, B has no row per n), which the tiles read but never store -- leaves
    it 0 and every output byte alone."""
    cfg, bm, bn = TILES[tile]
    seed = 300 + variant + bn
    has_split = g64.operand_model(variant).split_tensors
    what = f"guard v{variant} {tile}{' KN' if bmode else ''}"
    # (i)
    benign = _guard_case(bm, bn, bmode, seed)
    L = _Launch(built_lib, gpu_device, [benign], variant)
    plain = L.run(cfg, bmode)[0]
    L.reset()
    outs, flag = L.run_flagged(cfg, bmode)
    assert flag == 0, f"{what} (i): benign operands raised the flag ({flag})"
    assert _same_bytes(outs[0], plain)
    _check(benign, variant, outs[0], L.before[0], f"{what} (i)")
    # (ii)
    for where, m in (("interior", 5), ("border", benign.M - 1)):
        c = _guard_case(bm, bn, bmode, seed)
        _poke_A(c, m, 40, 1e6)
        _, flag = _Launch(built_lib, gpu_device, [c], variant).run_flagged(cfg, bmode)
        assert flag & 1, f"{what} (ii): 1e6 in row {m} ({where} tile) left the flag at {flag}"
    # (iii)
    for osp in ((0, OUT_SPLIT) if has_split else (0,)):
        c = _guard_case(bm, bn, bmode, seed, act=1 | osp)
        c.biasv[:] = 1e5
        L3 = _Launch(built_lib, gpu_device, [c], variant)
        outs, flag = L3.run_flagged(cfg, bmode)
        assert flag == (1 if osp else 0), f"{what} (iii): results of 1e5 with out_split={bool(osp)} gave flag {flag}"
        if not osp:
            _check(c, variant, outs[0], L3.before[0], f"{what} (iii)")
    # (iv)
    c = _guard_case(bm, bn, bmode, seed, poison=True)
    assert np.array_equal(c.Cbuf, benign.Cbuf) and np.array_equal(c.rowC, benign.rowC)
    L4 = _Launch(built_lib, gpu_device, [c], variant)
    outs, flag = L4.run_flagged(cfg, bmode)
    assert _same_bytes(outs[0], plain), f"{what} (iv): operands behind the padding rows changed stored bytes"
    _check(c, variant, outs[0], L4.before[0], f"{what} (iv)")
    assert flag == 0, f"{what} (iv): 1e6 where nothing is stored raised the flag ({flag})"


# ---- D4: the resident launch list ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,bmode", [(1, 0), (3, 0), (4, 0), (3, 1)], ids=["v1-NK", "v3-NK", "v4-NK", "v3-KN"])
def test_gemm_plan_runs_and_reruns(built_lib, gpu_device, variant, bmode):
    """vsr_gemm_plan_*: a grouped list with a multi-tile problem, run on a stream of the caller's; the queue the plan zeroes itself
    must be as good on the second run as on the first, and both runs write what vsr_run_gather_gemm_variant writes"""
    cfg, bm, bn = TILES["128x64"]
    rng = np.random.default_rng(400 + variant + bmode)
    cases = [g64.make_case(rng, 60, 60, 64, bm, bn, bmode, bias=True, act=1, residual=False),
             g64.make_case(rng, 700, 200, 96, bm, bn, bmode, bias=True, act=2 | POST_RELU, residual=True, alpha=0.5),
             g64.make_case(rng, 300, 100, 160, bm, bn, bmode, splitK=2, chunksPerSplit=3)]
    L = _Launch(built_lib, gpu_device, cases, variant)
    want = L.run(cfg, bmode)
    L.reset()
    plan = C.c_void_p()
    built_lib.check(built_lib.lib.vsr_gemm_plan_create(L.probs, len(cases), cfg, bmode, variant, C.byref(plan)))
    try:
        stream = torch.cuda.Stream(device=gpu_device)
        runs = []
        for _ in range(2):
            built_lib.check(built_lib.lib.vsr_gemm_plan_run(plan, C.c_void_p(stream.cuda_stream)))
            stream.synchronize()
            runs.append(L.outputs())
            L.reset()                                  # C back to its pre-launch bytes
    finally:
        built_lib.lib.vsr_gemm_plan_destroy(plan)
    _check_all(L, runs[0], f"plan v{variant} mode{bmode}")
    for i in range(len(cases)):
        assert _same_bytes(runs[0][i], runs[1][i]), f"second run of the plan differs on problem {i}"
        assert _same_bytes(runs[0][i], want[i]), f"the plan and vsr_run_gather_gemm_variant differ on problem {i}"


# ---- D5: softmax rows ---------------------------------------------------------------------------------------------------------------
def _softmax(built_lib, device, specs):
    """specs: dicts S [nsplit][M][ldS] fp32, N, ldP, scale, flags, offS / offP (floats the pointers lie past 16-byte alignment).
    Returns per problem the P buffer [M][ldP] as fp32 words.  float64 reference: _softmax64."""
    probs = (built_lib.SMProblem * len(specs))()
    keep = []
    for p, s in zip(probs, specs):
        S = s["S"]
        ns, M, ldS = S.shape
        offS, offP = s.get("offS", 0), s.get("offP", 0)
        dS = torch.from_numpy(np.concatenate([np.zeros(offS, np.float32), S.reshape(-1)])).to(device)
        dP = torch.full((offP + M * s["ldP"] + 64,), 9.0, device=device)
        assert dS.data_ptr() % 16 == 0 and dP.data_ptr() % 16 == 0
        keep.append((dS, dP))
        p.S, p.P = dS.data_ptr() + 4 * offS, dP.data_ptr() + 4 * offP
        p.M, p.N, p.ldS, p.ldP, p.nsplit, p.scale, p.flags, p.splitStride = M, s["N"], ldS, s["ldP"], ns, s["scale"], s.get("flags", 0), M * ldS
    torch.cuda.synchronize()
    built_lib.check(built_lib.lib.vsr_run_softmax(probs, len(specs), None))
    torch.cuda.synchronize()
    outs = []
    for (dS, dP), s in zip(keep, specs):
        full = dP.cpu().numpy()
        offP, n = s.get("offP", 0), s["S"].shape[1] * s["ldP"]
        assert np.all(full[:offP] == 9.0) and np.all(full[offP + n:] == 9.0), "softmax wrote outside its rows"
        outs.append(full[offP:offP + n].reshape(s["S"].shape[1], s["ldP"]))
    return outs


def _softmax64(s):
    x = s["S"].astype(np.float64).sum(0)[:, :s["N"]] * float(np.float32(s["scale"]))
    e = np.exp(x - x.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


def _check_softmax(s, out, what):
    N, ldP = s["N"], s["ldP"]
    ref = _softmax64(s)
    if s.get("flags", 0) & 1:
        assert ldP % 32 == 0
        h16 = np.ascontiguousarray(out).view(np.uint16).reshape(out.shape[0], ldP // 32, 2, 32)
        vals = (h16[:, :, 0, :].view(np.float16).astype(np.float64) + h16[:, :, 1, :].view(np.float16).astype(np.float64)).reshape(out.shape[0], ldP)
        pad = h16.transpose(0, 1, 3, 2).reshape(out.shape[0], ldP, 2)[:, N:, :]
        assert np.all(pad == 0), f"{what}: cells [N, ldP) must hold zeros in both halves"
        got = vals[:, :N]
    else:
        got = out[:, :N].astype(np.float64)
        assert np.all(out[:, N:] == 0), f"{what}: cells [N, ldP) must hold zeros"
    err = np.abs(got - ref).max()
    assert err < 2e-6, f"{what}: max |P - softmax64| = {err:.3e}"
    assert np.abs(got.sum(1) - 1).max() < 1e-5, f"{what}: rows do not sum to one"


def _scores(rng, ns, M, N, ldS):
    return (rng.standard_normal((ns, M, ldS)) * 3).astype(np.float32)


SM_SCALE = 1.0 / np.sqrt(960.0)


@pytest.mark.parametrize("trigger", ["long-row", "ld-not-multiple-of-4", "ldS-below-ldP", "S-4-bytes-off", "P-4-bytes-off"])
def test_softmax_three_pass_path(built_lib, gpu_device, trigger):
    """each condition that sends k_softmax_rows off its register path, on its own"""
    rng = np.random.default_rng(51)
    M, ns = 6, 2
    N, ldS, ldP, offS, offP = {"long-row": (5200, 5216, 5216, 0, 0), "ld-not-multiple-of-4": (61, 62, 62, 0, 0),
                               "ldS-below-ldP": (100, 100, 128, 0, 0), "S-4-bytes-off": (100, 128, 128, 1, 0),
                               "P-4-bytes-off": (100, 128, 128, 0, 1)}[trigger]
    s = dict(S=_scores(rng, ns, M, N, ldS), N=N, ldP=ldP, scale=SM_SCALE, offS=offS, offP=offP)
    _check_softmax(s, _softmax(built_lib, gpu_device, [s])[0], f"softmax {trigger}")


@pytest.mark.parametrize("path", ["register", "three-pass"])
def test_softmax_split_format_output(built_lib, gpu_device, path):
    """flags = 1: P leaves in split format; N is no multiple of 32 and the padding cells hold zeros in both halves"""
    rng = np.random.default_rng(52)
    specs = []
    for M, N, ns in ((5, 75, 1), (7, 1441, 3), (1, 40, 2)):
        ldP = -(-N // 32) * 32
        ldS = ldP if path == "register" else ldP - 4          # ldS < ldP: the three-pass path
        specs.append(dict(S=_scores(rng, ns, M, N, ldS), N=N, ldP=ldP, scale=SM_SCALE, flags=1))
    for i, (s, out) in enumerate(zip(specs, _softmax(built_lib, gpu_device, specs))):
        _check_softmax(s, out, f"softmax split-format {path} problem {i}")


def test_softmax_split_planes_and_row_lookup(built_lib, gpu_device):
    """nsplit 1 .. 5 and problems of 1, 5 and 7 rows in one launch: four rows share a workgroup, so every problem boundary falls
    inside one"""
    rng = np.random.default_rng(53)
    specs = []
    for i, (M, N) in enumerate(((1, 60), (5, 375), (7, 129), (5, 64), (1, 1441), (7, 33))):
        ld = -(-N // 32) * 32
        specs.append(dict(S=_scores(rng, i % 5 + 1, M, N, ld), N=N, ldP=ld, scale=SM_SCALE))
    assert {s["S"].shape[0] for s in specs} == {1, 2, 3, 4, 5}
    for i, (s, out) in enumerate(zip(specs, _softmax(built_lib, gpu_device, specs))):
        _check_softmax(s, out, f"softmax planes problem {i}")


@pytest.mark.parametrize("path", ["register", "three-pass"])
def test_softmax_extreme_rows(built_lib, gpu_device, path):
    """scaled scores of +-80 (the scale a power of two, so the fp32 product is exact), an all-equal row, one dominant score"""
    rng = np.random.default_rng(54)
    M, N = 8, 200
    ldP = 224
    ldS = ldP if path == "register" else 200
    S = np.zeros((1, M, ldS), np.float32)
    S[0, 0, :N] = np.where(rng.random(N) < 0.5, 640.0, -640.0)
    S[0, 0, 3], S[0, 0, 4] = 640.0, -640.0
    S[0, 1, :N] = np.where(rng.random(N) < 0.5, 640.0, -640.0) + rng.integers(-8, 9, N)
    S[0, 2, :N] = 2.5
    S[0, 3, :N] = -640.0
    S[0, 4, :N] = rng.standard_normal(N)
    S[0, 4, 77] = 400.0
    S[0, 5, :N] = 640.0
    S[0, 6, :N] = rng.standard_normal(N) * 8
    S[0, 7, :N] = -640.0
    S[0, 7, N - 1] = 640.0
    s = dict(S=S, N=N, ldP=ldP, scale=0.125)
    out = _softmax(built_lib, gpu_device, [s])[0]
    _check_softmax(s, out, f"softmax extreme rows {path}")
    assert out[4, 77] == 1.0 and out[7, N - 1] == 1.0
    assert np.all(out[2, :N] == out[2, 0]) and abs(float(out[2, 0]) * N - 1) < 1e-6
