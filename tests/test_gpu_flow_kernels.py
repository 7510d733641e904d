"""The flow, ProPainter and LaMa kernels one launch at a time against float64 references.

Kernels of csrc/flow_kernels.hip, pp_kernels.hip / pp_gen_kernels.hip, pp_attn_kernels.hip and lama_kernels.hip are bound here
through a ctypes handle of this module (they are internal: include/vsr_hip.h and _lib.SIGNATURES do not list them).  Every case
fills its outputs with a sentinel, launches once, and compares with a reference that restates the operation (torch.nn.functional
in float64, the oracle's own functions, np.pad): never the kernel's own loop.  Cells outside a kernel's store set must still hold
the sentinel.  Each tolerance is derived from the kernel's arithmetic next to its assertion and printed with the error.

test_launcher_prototypes_match_headers runs without a GPU: a changed kernel signature fails there, not as a launch with shifted
arguments."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "video-subtitle-remover_amd", "csrc")

U32 = 2.0 ** -24        # fp32 unit roundoff
U16 = 2.0 ** -11        # fp16 unit roundoff
SENT = -7.0             # sentinel of every output buffer
LN2 = math.log(2.0)

# ---- prototypes, copied from the headers: p = pointer, i = int, l = int64_t, f = float (all return int) -------------------------
PROTOTYPES = {
    # flow_kernels.h
    "vsr_raft_launch_im2col7_u8": "piiiipp",
    "vsr_raft_launch_inorm_stats": "piiiiippp",
    "vsr_raft_launch_inorm_apply": "piiiiipipip",
    "vsr_raft_launch_ctx_split": "ppiiiiipp",
    "vsr_raft_launch_flow_update": "pipppiiiiiiip",
    "vsr_raft_launch_im2col7_flow": "piiipp",
    "vsr_raft_launch_avgpool2": "pliipp",
    "vsr_raft_launch_corr_transpose": "ppiip",
    "vsr_raft_launch_corr_lookup": "pppplipp",
    "vsr_raft_launch_gru_rh": "ppiiiiiiip",
    "vsr_raft_launch_gru_update": "pppiiiiiip",
    "vsr_raft_launch_convex_up": "ppiiipp",
    "vsr_rfc_launch_im2col5": "pppiiipp",
    "vsr_rfc_launch_deform_cols": "pppifiiiiipp",
    "vsr_rfc_launch_combine": "pipppiiippp",
    # pp_kernels.h
    "vsr_pp_launch_mask_f32": "plpp",
    "vsr_pp_launch_mask_u8": "plpp",
    "vsr_pp_launch_imgprop": "ppppppiiiippp",
    "vsr_pp_launch_im2col3": "pppiiipp",
    "vsr_pp_launch_ds_flow": "piiipp",
    "vsr_pp_launch_ds_mask": "ppiiipiip",
    "vsr_pp_launch_featprop_prep": "ppppiiiippp",
    "vsr_pp_launch_deform_cols": "ppipfiiiipp",
    "vsr_pp_launch_layernorm": "pppiiiiiipp",
    "vsr_pp_launch_pool": "pppiiiiiipp",
    "vsr_pp_launch_fold": "piiiiiiiiipp",
    "vsr_pp_launch_unfold_gelu": "piiiiiiipp",
    "vsr_pp_launch_tanh_out": "piiiipp",
    "vsr_pp_launch_fold_gelu": "piiiiiiiiipp",
    "vsr_pp_launch_unfold_plain": "piiiiiiipp",
    # pp_attn.h
    "vsr_pp_launch_flash_attn": "piiipp",
    # lama_kernels.h
    "vsr_lama_launch_im2col7": "ppiiiiipp",
    "vsr_lama_launch_halo": "piiiiip",
    "vsr_lama_launch_add_halo": "pppiiiiiip",
    "vsr_lama_launch_out": "pppiiiiipp",
}
_CT = {"p": C.c_void_p, "i": C.c_int, "l": C.c_int64, "f": C.c_float}


class PpAttnProblem(C.Structure):
    """mirror of struct PpAttnProblem (pp_attn.h)"""
    _fields_ = [("Q", C.c_void_p), ("K", C.c_void_p), ("V", C.c_void_p), ("O", C.c_void_p),
                ("qrow", C.c_void_p), ("krow", C.c_void_p), ("orow", C.c_void_p),
                ("M", C.c_int32), ("nk", C.c_int32), ("tileStart", C.c_int32), ("scale", C.c_float)]


HEADERS = ("flow_kernels.h", "pp_kernels.h", "pp_attn.h", "lama_kernels.h")


def _header_prototypes():
    """{name: type string} of every vsr_* declaration in the four kernel headers, comments stripped"""
    out = {}
    for h in HEADERS:
        src = open(os.path.join(CSRC, h)).read()
        src = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
        for name, args in re.findall(r"\bint\s+(vsr_[a-z0-9_]+)\s*\(([^)]*)\)", src):
            sig = ""
            for a in (x.strip() for x in args.split(",")):
                if "*" in a:
                    sig += "p"
                elif a.startswith("int64_t"):
                    sig += "l"
                elif a.startswith("float"):
                    sig += "f"
                elif a.startswith("int") or a.startswith("unsigned"):
                    sig += "i"
                else:
                    raise AssertionError(f"{h}: unparsed argument {a!r} of {name}")
            out[name] = sig
    return out


def _struct_fields():
    src = open(os.path.join(CSRC, "pp_attn.h")).read()
    body = re.search(r"struct\s+PpAttnProblem\s*\{(.*?)\};", src, flags=re.S).group(1)
    fields = []
    for line in body.splitlines():
        line = line.split("//")[0].strip()
        if not line:
            continue
        decl = line.rstrip(";")
        kind = "p" if "*" in decl else ("f" if decl.startswith("float") else "i")
        names = decl.replace("*", " ").split(None, 1)[1] if not decl.startswith("const") else decl.replace("*", " ").split(None, 2)[2]
        fields += [(n.strip(), kind) for n in names.split(",")]
    return fields


def test_launcher_prototypes_match_headers(built_lib):
    """host check (no GPU): every launcher bound here is exported and its ctypes prototype is the header's; the problem mirror
    has pp_attn.h's field order and kinds"""
    decl = _header_prototypes()
    missing = sorted(set(PROTOTYPES) - set(decl))
    assert not missing, f"bound here but declared in none of {HEADERS}: {missing}"
    lib = C.CDLL(built_lib.LIB_PATH)
    for name, sig in PROTOTYPES.items():
        assert hasattr(lib, name), f"{name} is not exported by libvsr_hip.so"
        assert sig == decl[name], f"{name}: ctypes prototype {sig} != header {decl[name]}"
    kinds = {C.c_void_p: "p", C.c_int32: "i", C.c_float: "f"}
    assert [(n, kinds[t]) for n, t in PpAttnProblem._fields_] == _struct_fields()
    assert C.sizeof(PpAttnProblem) == 72


# ---- binding and helpers ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def K(built_lib, gpu_device):
    lib = C.CDLL(built_lib.LIB_PATH)
    for name, sig in PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.restype = C.c_int
        fn.argtypes = [_CT[ch] for ch in sig]
    return lib


_KEEP = []         # inputs of the next launch: a pointer taken from a temporary tensor would point into a block the caching allocator
                  # hands to the next tensor at once (two inputs of one launch aliased); launch() releases them after synchronising


def dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    _KEEP.append(t)
    return t


def sent(n, extra=0):
    return torch.full((int(n) + extra,), SENT, dtype=torch.float32, device="cuda")


def ptr(t, off=0):
    return C.c_void_p(t.data_ptr() + off * t.element_size())


def launch(fn, *args):
    rc = fn(*args, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, f"launch returned {rc}"
    torch.cuda.synchronize()
    _KEEP.clear()


def check(what, err, bound):
    print(f"{what}: max err {err:.3e} bound {bound:.3e}")
    assert err <= bound, f"{what}: {err:.3e} > {bound:.3e}"


def untouched(buf, mask, what):
    """cells where mask is True must still hold the sentinel"""
    got = buf[mask]
    assert np.all(got == SENT), f"{what}: {int((got != SENT).sum())} cells outside the store set were written"


def halo_mask(n, H, W, Cc, halo):
    m = np.ones((n, H + 2 * halo, W + 2 * halo, Cc), dtype=bool)
    m[:, halo:halo + H, halo:halo + W, :] = False
    return m


def with_halo(x, halo, fill=SENT):
    """[n,H,W,C] -> [n,H+2h,W+2h,C] with `fill` in the halo"""
    n, H, W, Cc = x.shape
    out = np.full((n, H + 2 * halo, W + 2 * halo, Cc), fill, dtype=np.float32)
    out[:, halo:halo + H, halo:halo + W] = x
    return out


def bilinear_bound(vmax, dpos):
    """|bilinear(v, p) - bilinear(v, p')| for |p - p'| <= dpos per axis: the interpolant's slope is at most 2 vmax per axis (zero
    padding included), plus the fp32 weights (two products, four terms): 8 ulp of vmax"""
    return vmax * (4.0 * dpos + 8.0 * U32)


# =====================================================================================================================================
# Fused window attention (pp_attn_kernels.hip): softmax(Q K^T / sqrt(128)) V, reference sparse_transformer.py:238-262
# =====================================================================================================================================
D, ROW = 128, 3 * 512
ATTN_SCALE = float(np.float32(np.float32(1.0 / math.sqrt(128.0)) * np.float32(1.4426950408889634)))   # as flow_engine.hip sets it
M_SET = (1, 31, 32, 33, 45, 127, 128, 129, 300)
NK_SET = (1, 31, 32, 33, 45 * 6, 65, 3000)


@pytest.fixture(scope="module")
def strip_shapes(built_lib):
    """(M, nk) of the window attention problems of a real 1920x360 plan (11 local + 4 reference frames), built on the host"""
    import _replay_pp as rp
    from oracle.make_golden import propainter_inputs
    from vsr_amd.engine import PpEngine
    from vsr_amd.synth import make_propainter_state_dict

    e = PpEngine(device=-1, state_dict=make_propainter_state_dict(0))
    t, lt, H, W = 15, 11, 360, 1920
    _, masks, _, _ = propainter_inputs(91, t, lt, H, W)
    view = rp.gen_plan_view(built_lib, e, t, lt, H, W, e.window_flags(masks[:lt, 0].astype(np.uint8)))
    shapes = set()
    for info, items in view.ops:
        if info.tag.decode() == "attn.qk":
            shapes |= {(int(it.M), int(it.N)) for it in items}
    view.close()
    e.close()
    assert shapes and max(n for _, n in shapes) > 1000
    return sorted(shapes)


def _attn_inputs(rng, shapes, regime):
    """fused QKV rows [R][1536] and one problem per (M, nk) in the engine's order (largest nk first); Q / K / V of problem j are the
    head j % 4 columns (offsets 0 / 128 / 256 / 384 of each third); key rows are shared between problems except the `special` keys of
    the last-tile / last-key regimes, whose rows belong to one problem"""
    shapes = sorted(shapes, key=lambda s: -s[1])
    pool = max(4096, max(n for _, n in shapes))
    nspecial = sum(min(32, nk) if regime == "lasttile" else 1 for _, nk in shapes) if regime in ("lasttile", "lastkey") else 0
    R = pool + nspecial
    X = rng.standard_normal((R, ROW)).astype(np.float32)
    u = rng.standard_normal(D)
    u = (u / np.linalg.norm(u)).astype(np.float32)
    if regime == "onehot":
        X[:, :512] *= 8.0
    elif regime in ("lasttile", "lastkey"):
        X[:, :1024] *= 0.3
        X[:, :512] += np.tile(6.0 * u, 4)
        X[pool:, 512:1024] += np.tile(6.0 * u, 4)
    elif regime == "equal":
        X[:, 512:1024] = X[0, 512:1024]
    probs, nxt, orow0 = [], pool, 0
    for j, (M, nk) in enumerate(shapes):
        qrow = rng.choice(pool, M, replace=False)
        krow = rng.choice(pool, nk, replace=False)
        if regime == "lasttile":
            s0 = ((nk - 1) // 32) * 32
            krow[s0:] = np.arange(nxt, nxt + nk - s0)
            nxt += nk - s0
        elif regime == "lastkey":
            krow[nk - 1] = nxt
            nxt += 1
        probs.append(dict(M=M, nk=nk, head=j % 4, qrow=qrow, krow=krow, orow=np.arange(orow0, orow0 + M)))
        orow0 += M
    perm = rng.permutation(orow0)          # output rows: a permutation, each written by one problem in one head's columns
    for p in probs:
        p["orow"] = perm[p["orow"]]
    return X, probs, orow0


def _attn_launch(K, X, probs, nout, f16, Xd=None):
    Xd = dev(X) if Xd is None else Xd
    O = sent(nout * 512)
    tabs, offs = [], []
    for p in probs:
        for key, ld in (("qrow", ROW), ("krow", ROW), ("orow", 512)):
            offs.append(sum(len(t) for t in tabs))
            tabs.append((p[key] * ld).astype(np.int32))
    T = dev(np.concatenate(tabs))
    arr, tile = (PpAttnProblem * len(probs))(), 0
    for j, p in enumerate(probs):
        h = 128 * p["head"]
        q = arr[j]
        q.Q, q.K, q.V, q.O = ptr(Xd, h).value, ptr(Xd, 512 + h).value, ptr(Xd, 1024 + h).value, ptr(O, h).value
        q.qrow, q.krow, q.orow = ptr(T, offs[3 * j]).value, ptr(T, offs[3 * j + 1]).value, ptr(T, offs[3 * j + 2]).value
        q.M, q.nk, q.tileStart, q.scale = p["M"], p["nk"], tile, ATTN_SCALE
        tile += (p["M"] + 127) // 128
    raw = dev(np.frombuffer(bytes(arr), dtype=np.uint8))
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    launch(K.vsr_pp_launch_flash_attn, ptr(raw), len(probs), tile, int(f16), ptr(flag))
    return O.cpu().numpy().reshape(nout, 512), int(flag.item())


def _attn_check(X, probs, O, f16, what):
    """float64 softmax(s) V with s = scale * Q K^T in log2 units (exp2), Q / K / V rounded to fp16 first in the f16 mode.
    Bound per query row (derivation):
      * a score is a 128-term fp32 dot product (exact products in the f16 mode): |ds| <= scale (D + 2) u32 sum_d |q_d k_d|; the
        exponent s - m carries the error of s and of the running maximum, and fp32 rounding u32 |s - m| (capped at 40: weights
        below 2^-40 are covered by the last term);
      * exp2 and the alpha rescales (one per key tile) add 2 + 2 ntiles ulp: relative weight error
        delta = ln2 (2 |ds| + u32 min(|s - m|, 40)) + (2 + 2 ntiles) u32;
      * normalised weights move by <= 2 delta / (1 - delta); the fp32 sums over nk keys (output and row sum) add 2 (nk + 2) u32;
      * f16: the probabilities enter P.V as fp16 (u16 relative, 2^-25 absolute below the normal range), the row sum stays fp32.
    All of it times max |V| of the row's keys."""
    Xr = X.astype(np.float16).astype(np.float64) if f16 else X.astype(np.float64)
    written = np.zeros(O.shape, dtype=bool)
    worst = (0.0, 1.0, None)
    for p in probs:
        h = 128 * p["head"]
        Q = Xr[p["qrow"], h:h + D]
        Kk = Xr[p["krow"], 512 + h:512 + h + D]
        V = Xr[p["krow"], 1024 + h:1024 + h + D]
        s = ATTN_SCALE * (Q @ Kk.T)
        gap = s.max(1, keepdims=True) - s
        w = np.exp2(-gap)
        ref = (w @ V) / w.sum(1, keepdims=True)
        nk = p["nk"]
        ds = ATTN_SCALE * (D + 2) * U32 * (np.abs(Q) @ np.abs(Kk).T).max(1)
        delta = LN2 * (2 * ds + U32 * np.minimum(gap.max(1), 40.0)) + (2 + 2 * ((nk + 31) // 32)) * U32
        vmax = np.abs(V).max()
        bound = vmax * (2 * delta / (1 - delta) + 2 * (nk + 2) * U32 + nk * 2.0 ** -38)
        if f16:
            bound = bound + vmax * (U16 + nk * 2.0 ** -25)
        got = O[p["orow"], h:h + D]
        err = np.abs(got - ref).max(1)
        assert np.isfinite(got).all(), f"{what}: non-finite output in problem {p['M']}x{nk}"
        bad = err > bound
        assert not bad.any(), f"{what}: problem M={p['M']} nk={nk}: err {err[bad].max():.3e} > bound {bound[bad].min():.3e}"
        r = float((err / bound).max())
        if r > worst[0] / worst[1]:
            worst = (float(err.max()), float(bound[np.argmax(err / bound)]), (p["M"], nk))
        written[np.ix_(p["orow"], np.arange(h, h + D))] = True
    print(f"{what}: worst err/bound {worst[0]:.3e} / {worst[1]:.3e} at (M, nk) = {worst[2]}")
    untouched(O, ~written, f"{what} (other heads' columns, unwritten rows)")


@pytest.mark.gpu
@pytest.mark.parametrize("regime", ["benign", "onehot", "lasttile", "lastkey", "equal"])
@pytest.mark.parametrize("f16", [0, 1])
def test_flash_attention_vs_float64(K, strip_shapes, regime, f16):
    """Every (M, nk) of the edge sets and of the 1080p strip plan as the problems of ONE launch (prefix-sum tileStart, largest nk
    first), Q / K / V column slices of fused QKV rows through permuted row tables.  Regimes: benign scores, near one-hot (Q x 8), the
    row maximum only in the last key tile (the alpha rescale decides), the maximum on key nk - 1 (a clamped row that escaped the
    `key < nk` mask would count it twice), all scores equal.  The range flag stays 0."""
    rng = np.random.default_rng(1000 + 10 * f16 + ["benign", "onehot", "lasttile", "lastkey", "equal"].index(regime))
    shapes = [(m, n) for m in M_SET for n in NK_SET] + list(strip_shapes)
    X, probs, nout = _attn_inputs(rng, shapes, regime)
    O, flag = _attn_launch(K, X, probs, nout, f16)
    _attn_check(X, probs, O, f16, f"flash attn [{'f16' if f16 else 'f32'}] {regime}")
    assert flag == 0, "range flag raised on inputs within the fp16 range"


@pytest.mark.gpu
@pytest.mark.parametrize("f16", [0, 1])
def test_flash_attention_is_deterministic(K, f16):
    rng = np.random.default_rng(77)
    X, probs, nout = _attn_inputs(rng, [(129, 3000), (45, 270), (33, 33), (1, 1)], "benign")
    Xd = dev(X)
    a, _ = _attn_launch(K, X, probs, nout, f16, Xd)
    b, _ = _attn_launch(K, X, probs, nout, f16, Xd)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "two launches on the same inputs differ"


@pytest.mark.gpu
def test_flash_attention_range_flag(K):
    """A query row of 7e4 (beyond fp16's 65504): the f16 kernel turns it into inf, the row's output is not finite and the flag is
    raised; the f32 kernel keeps it finite and exact -- the keys' first components are 0.05 apart, so the largest score leads the next
    by > 40 in log2 units and the row is V of that key up to 2^-40 nk + fp32 rounding of the normalisation (4 ulp)."""
    rng = np.random.default_rng(5)
    X, probs, nout = _attn_inputs(rng, [(33, 45), (129, 65)], "benign")
    p = probs[1]                                    # head 1 problem (nk = 45 sorts second)
    h = 128 * p["head"]
    big = p["qrow"][7]
    X[big, h:h + D] = 0.0
    X[big, h] = 7.0e4
    X[p["krow"], 512 + h] = rng.permutation(np.arange(p["nk"]) * 0.05 - 1.0).astype(np.float32)
    s = ATTN_SCALE * 7.0e4 * np.sort(X[p["krow"], 512 + h].astype(np.float64))
    assert s[-1] - s[-2] > 40
    for f16 in (0, 1):
        O, flag = _attn_launch(K, X, probs, nout, f16)
        if f16:
            assert flag == 1, "fp16 overflow of a Q row did not raise the range flag"
            assert not np.isfinite(O[p["orow"][7], h:h + D]).all()
            continue
        assert flag == 0
        top = p["krow"][np.argmax(X[p["krow"], 512 + h])]
        want = X[top, 1024 + h:1024 + h + D].astype(np.float64)
        err = np.abs(O[p["orow"][7], h:h + D] - want).max()
        check("flash attn f32, Q row of 7e4", err, np.abs(want).max() * (p["nk"] * 2.0 ** -40 + 4 * U32))
        others = [q for q in probs if q is not p] + [dict(p, qrow=np.delete(p["qrow"], 7), orow=np.delete(p["orow"], 7), M=p["M"] - 1)]
        Oc = O.copy()
        Oc[p["orow"][7], :] = SENT
        _attn_check(X, others, Oc, 0, "flash attn f32, the other rows beside the 7e4 row")


# =====================================================================================================================================
# RAFT
# =====================================================================================================================================
def _lookup_coords(rng, M, h0, w0):
    """x, y per row: integers, exactly w-1 / h-1, negative, 1..5 px outside, hundreds of px away, halfway, random"""
    kinds = [lambda: (float(rng.integers(0, w0)), float(rng.integers(0, h0))),
             lambda: (float(w0 - 1), float(h0 - 1)),
             lambda: (-rng.uniform(0.1, 3.0), -rng.uniform(0.1, 3.0)),
             lambda: (w0 - 1 + rng.integers(1, 6), -float(rng.integers(1, 6))),
             lambda: (rng.uniform(-600, -200), rng.uniform(300, 900)),
             lambda: (rng.integers(0, w0) + 0.5, rng.integers(0, h0) + 0.5),
             lambda: (rng.uniform(-8, w0 + 8), rng.uniform(-8, h0 + 8))]
    return np.array([kinds[m % len(kinds)]() for m in range(M)], dtype=np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("sizes", [[(45, 240), (22, 120), (11, 60), (5, 30)], [(9, 13), (6, 7), (4, 3), (3, 2)]])
def test_corr_lookup(K, sizes):
    """CorrBlock.__call__ against RaftOracle.lookup in float64 (grid_sample, align_corners=True, zero padding); ld = 340 > 324: the
    K-padding columns are zero"""
    from oracle.raft import RaftOracle

    rng = np.random.default_rng(len(sizes[0]) + sizes[0][0])
    M, ld = 70, 340
    vols = [rng.standard_normal((M, hh, ww)).astype(np.float32) for hh, ww in sizes]
    coords = _lookup_coords(rng, M, *sizes[0])
    dv = [dev(v) for v in vols]
    out = sent(M * ld)
    lv = (C.c_void_p * 4)(*[t.data_ptr() for t in dv])
    launch(K.vsr_raft_launch_corr_lookup, lv, (C.c_int * 4)(*[s[0] for s in sizes]), (C.c_int * 4)(*[s[1] for s in sizes]),
           ptr(dev(coords)), M, ld, ptr(out))
    got = out.cpu().numpy().reshape(M, ld)
    pyr = [torch.from_numpy(v.astype(np.float64)).unsqueeze(1) for v in vols]
    c = torch.from_numpy(coords.astype(np.float64)).T.reshape(1, 2, 1, M)
    ref = RaftOracle.lookup(pyr, c).reshape(324, M).T.numpy()
    # sampling position: x / 2^l + (i - 4), the normalise / un-normalise pair: <= 8 ulp of (|x| + W) per axis
    for lvl, (hh, ww) in enumerate(sizes):
        cols = slice(81 * lvl, 81 * lvl + 81)
        ax = np.abs(coords) / 2 ** lvl + 4
        dpos = 8 * U32 * (ax.max() + max(hh, ww))
        b = bilinear_bound(np.abs(vols[lvl]).max(), dpos)
        e = np.abs(got[:, cols] - ref[:, cols]).max()
        check(f"corr lookup level {lvl} {hh}x{ww}", e, b)
    assert np.all(got[:, 324:] == 0.0), "K-padding columns of the lookup must be written as zero"


@pytest.mark.gpu
@pytest.mark.parametrize("h,w", [(1, 1), (1, 3), (2, 2), (3, 1), (3, 3)])
def test_convex_up(K, h, w):
    """RAFT.upsample_flow against RaftOracle.upsample in float64; mask logits up to +-80 (the softmax subtracts its maximum)"""
    from oracle.raft import RaftOracle

    rng = np.random.default_rng(10 * h + w)
    pairs = 2
    flow = rng.uniform(-20, 20, (pairs, h, w, 2)).astype(np.float32)
    mask = rng.uniform(-4, 4, (pairs * h * w, 576)).astype(np.float32)
    mask[::2, :32] = 80.0                                         # half of the sub-pixels of neighbour 0 ...
    mask[1::3, 64 * 4:64 * 4 + 16] = -80.0                        # ... a quarter of the centre's: the rest keeps in-frame weight
    mask[:, 64 * 8 + 3] = 80.0
    out = sent(pairs * 2 * 64 * h * w)
    launch(K.vsr_raft_launch_convex_up, ptr(dev(flow)), ptr(dev(mask)), pairs, h, w, ptr(out))
    got = out.cpu().numpy().reshape(pairs, 2, 8 * h, 8 * w)
    ref = RaftOracle.upsample(torch.from_numpy(flow.astype(np.float64)).permute(0, 3, 1, 2),
                              torch.from_numpy(mask.astype(np.float64)).reshape(pairs, h, w, 576).permute(0, 3, 1, 2)).numpy()
    # weights e^(l - max) / sum: the fp32 difference l - max rounds by u32 |l - max| (weights below e^-40 are negligible), expf and
    # the division add 4 ulp; nine fp32 products and sums add 12 ulp of max |8 flow|
    gap = np.minimum(mask.reshape(-1, 9, 64).max(1, keepdims=True) - mask.reshape(-1, 9, 64), 40.0).max()
    check(f"convex up {h}x{w}", np.abs(got - ref).max(), 8 * np.abs(flow).max() * (2 * (U32 * gap + 4 * U32) + 12 * U32))


INORM_CASES = [  # C, H, W, halo, pointer offset (floats): 0 = aligned (partial4), 1 = 4 bytes off (partial)
    (32, 63, 65, 1, 0), (64, 17, 241, 0, 1), (96, 17, 241, 1, 0), (96, 63, 65, 0, 1), (128, 63, 65, 0, 1), (256, 17, 241, 1, 0),
    (256, 63, 65, 1, 1), (32, 513, 512, 1, 0), (32, 513, 512, 0, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("Cc,H,W,halo,off", INORM_CASES)
def test_inorm_stats(K, Cc, H, W, halo, off):
    """nn.InstanceNorm2d statistics (eps 1e-5, biased variance) against float64; channel 0 is a constant plane (var 0), channel 1 a
    large mean with a small spread (1e3 +- 1e-2), the rest mixed scales.  H*W = 4095, 4097 and 262 656 (> 64 x 4096: the slice cap)"""
    rng = np.random.default_rng(Cc + H + off)
    n = 2
    x = (rng.standard_normal((n, H, W, Cc)) * rng.uniform(0.1, 4, Cc) + rng.uniform(-3, 3, Cc)).astype(np.float32)
    x[:, :, :, 0] = 2.5
    x[:, :, :, 1] = (1e3 + rng.uniform(-1e-2, 1e-2, (n, H, W))).astype(np.float32)
    xp = with_halo(x, halo, np.nan)                 # a read of a halo cell would poison the statistics
    buf = torch.empty(xp.size + 4, dtype=torch.float32, device="cuda")
    buf[off:off + xp.size] = dev(xp.reshape(-1))
    acc = torch.empty(n * Cc * 2, dtype=torch.float64, device="cuda")
    stats = sent(n * Cc * 2)
    launch(K.vsr_raft_launch_inorm_stats, ptr(buf, off), n, H, W, Cc, halo, ptr(acc), ptr(stats))
    got = stats.cpu().numpy().reshape(n, Cc, 2)
    x64 = x.astype(np.float64)
    mean = x64.mean((1, 2))
    var = x64.var((1, 2))
    rstd = 1.0 / np.sqrt(var + 1e-5)
    # fp64 sums: each thread adds L = npix / (slices * lanes per channel) terms, then a tree of <= 32 and <= 64 slice atomics:
    # |d sum| <= (L + 100) u64 sum |.|; E[x^2] - mean^2 turns the error of the second moment into an absolute error of var
    npix = H * W
    slices = min(64, max(1, (npix + 4095) // 4096))
    lanes = (256 // (Cc // 4)) if off == 0 else 8
    terms = npix / (slices * lanes) + 100
    u64 = 2.0 ** -53
    ex2 = (x64 ** 2).mean((1, 2))
    dmean = terms * u64 * np.abs(x64).mean((1, 2)) + U32 * np.abs(mean)
    dvar = 2 * terms * u64 * ex2 + 2 * np.abs(mean) * terms * u64 * np.abs(x64).mean((1, 2))
    drstd = 0.5 * rstd * dvar / (var + 1e-5) + 2 * U32 * rstd
    what = f"inorm stats C={Cc} {H}x{W} halo {halo} {'partial' if off else 'partial4'}"
    check(what + " mean / bound", float((np.abs(got[..., 0] - mean) / dmean).max()), 1.0)
    check(what + " rstd / bound", float((np.abs(got[..., 1] - rstd) / drstd).max()), 1.0)


@pytest.mark.gpu
@pytest.mark.parametrize("relu,res_halo", [(0, None), (1, None), (0, 0), (1, 2)])
def test_inorm_apply(K, relu, res_halo):
    """(x - mean) * rstd [ReLU] [+ residual, ReLU] in place on the interior of a halo-1 NHWC map: the halo keeps its sentinel"""
    rng = np.random.default_rng(3 + relu)
    n, H, W, Cc, halo = 2, 13, 11, 64, 1
    x = rng.standard_normal((n, H, W, Cc)).astype(np.float32) * 3
    stats = np.stack([rng.uniform(-2, 2, (n, Cc)), rng.uniform(0.2, 5, (n, Cc))], -1).astype(np.float32)
    xd = dev(with_halo(x, halo))
    r = rng.standard_normal((n, H, W, Cc)).astype(np.float32)
    rd = dev(with_halo(r, res_halo, np.nan)) if res_halo is not None else None        # the residual's halo is never read
    launch(K.vsr_raft_launch_inorm_apply, ptr(xd), n, H, W, Cc, halo, ptr(dev(stats)), relu, ptr(rd) if rd is not None else None,
           res_halo or 0)
    got = xd.cpu().numpy()
    y = (x.astype(np.float64) - stats[:, None, None, :, 0]) * stats[:, None, None, :, 1]
    if relu:
        y = np.maximum(y, 0)
    if rd is not None:
        y = np.maximum(y + r, 0)
    # subtract, multiply (and add): 3 roundings of the largest intermediate
    bound = 3 * U32 * (np.abs(x).max() + 2) * 5 + 3 * U32 * np.abs(r).max()
    check(f"inorm apply relu={relu} res halo {res_halo}", np.abs(got[:, halo:halo + H, halo:halo + W] - y).max(), bound)
    untouched(got, halo_mask(n, H, W, Cc, halo), "inorm apply halo")


@pytest.mark.gpu
@pytest.mark.parametrize("hs,ws", [(7, 9), (45, 240), (1, 5), (6, 3)])
def test_avgpool2(K, hs, ws):
    """F.avg_pool2d(2, stride 2) with floor sizes; the destination's tail keeps its sentinel"""
    rng = np.random.default_rng(hs * ws)
    rows = 5
    src = rng.standard_normal((rows, hs, ws)).astype(np.float32)
    hd, wd = hs // 2, ws // 2
    out = sent(rows * hd * wd, extra=64)
    launch(K.vsr_raft_launch_avgpool2, ptr(dev(src)), rows, hs, ws, ptr(out))
    got = out.cpu().numpy()
    if hd and wd:
        ref = F.avg_pool2d(torch.from_numpy(src.astype(np.float64)).unsqueeze(1), 2, stride=2).squeeze(1).numpy()
        # three fp32 additions and one exact scaling by 0.25: 3 ulp of the sum of four magnitudes
        check(f"avgpool2 {hs}x{ws}", np.abs(got[:rows * hd * wd].reshape(rows, hd, wd) - ref).max(), 3 * U32 * np.abs(src).max())
    untouched(got[rows * hd * wd:], np.ones(64, bool), "avgpool2 tail")


@pytest.mark.gpu
@pytest.mark.parametrize("hw", [1, 63, 64, 65, 130])
def test_corr_transpose(K, hw):
    rng = np.random.default_rng(hw)
    n = 3
    src = rng.standard_normal((n, hw, hw)).astype(np.float32)
    out = sent(n * hw * hw, extra=64)
    launch(K.vsr_raft_launch_corr_transpose, ptr(dev(src)), ptr(out), n, hw)
    got = out.cpu().numpy()
    assert np.array_equal(got[:n * hw * hw].reshape(n, hw, hw), src.transpose(0, 2, 1)), "a transpose is a copy: bit-exact"
    untouched(got[n * hw * hw:], np.ones(64, bool), "corr transpose tail")


# =====================================================================================================================================
# Deformable convolution columns (RFC and ProPainter) against oracle.deform_conv.deform_conv2d with an identity weight
# =====================================================================================================================================
def _deform_ref(x, offset, mask):
    """cols [n, cin, 9, h, w] of deform_conv2d (3x3, stride 1, pad 1): an identity weight makes the contraction a copy"""
    from oracle.deform_conv import deform_conv2d

    n, cin, h, w = x.shape
    eye = torch.zeros(cin * 9, cin, 3, 3, dtype=torch.float64)
    idx = torch.arange(cin * 9)
    eye[idx, idx // 9, (idx % 9) // 3, idx % 3] = 1.0
    return deform_conv2d(x, offset, eye, padding=1, mask=mask).reshape(n, cin, 9, h, w)


def _kernel_cols(cols, cin):
    """kernel column order ((ci/32)*9 + k)*32 + ci%32 -> [m, cin, 9]"""
    m = cols.shape[0]
    return cols.reshape(m, cin // 32, 9, 32).transpose(0, 1, 3, 2).reshape(m, cin, 9)


def _offset_logits(rng, m):
    """offset logits: moderate, exactly 0 (integer positions), +-30 (maxMag tanh saturation), large (samples leave the frame)"""
    o = rng.standard_normal((m, 432)).astype(np.float32)
    o[0::4, :288] = 0.0
    o[1::4, 0:288:3] = 30.0
    o[1::4, 1:288:3] = -30.0
    o[2::4, :288] *= 4.0
    o[:, 288:] *= 3.0
    o[3::5, 288:300] = 100.0
    return o


@pytest.mark.gpu
@pytest.mark.parametrize("halo", [0, 1])
def test_rfc_deform_cols(K, halo):
    """SecondOrderDeformableAlignment's columns: cat[srcA, srcB] (2 x 128 channels, 16 offset groups of 16), offset 5 tanh, mask
    sigmoid; NaN in the sources' halo: the kernel must never read it"""
    rng = np.random.default_rng(40 + halo)
    n, h, w, Cc, ld, mag = 2, 5, 7, 128, 440, 5.0
    A = rng.standard_normal((n, h, w, Cc)).astype(np.float32)
    B = rng.standard_normal((n, h, w, Cc)).astype(np.float32)
    off = np.zeros((n * h * w, ld), dtype=np.float32)
    off[:, :432] = _offset_logits(rng, n * h * w)
    off[:, 432:] = np.nan
    cols = sent(n * h * w * 9 * 2 * Cc)
    launch(K.vsr_rfc_launch_deform_cols, ptr(dev(with_halo(A, halo, np.nan))), ptr(dev(with_halo(B, halo, np.nan))), ptr(dev(off)), ld,
           mag, n, h, w, halo, Cc, ptr(cols))
    got = _kernel_cols(cols.cpu().numpy().reshape(n * h * w, 9 * 2 * Cc), 2 * Cc)
    o64 = off[:, :432].astype(np.float64).reshape(n, h, w, 432).transpose(0, 3, 1, 2)
    x = torch.from_numpy(np.concatenate([A, B], -1).astype(np.float64)).permute(0, 3, 1, 2)
    ref = _deform_ref(x, torch.from_numpy(mag * np.tanh(o64[:, :288])), torch.from_numpy(1 / (1 + np.exp(-o64[:, 288:]))))
    ref = ref.permute(0, 3, 4, 1, 2).reshape(n * h * w, 2 * Cc, 9).numpy()
    # position (y - 1 + ky) + 5 tanhf(o): tanhf 4 ulp of 5, the product and the sum: 3 ulp of (5 + h + w); sigmoid 4 ulp
    dpos = U32 * (4 * mag + 3 * (mag + h + w))
    vmax = max(np.abs(A).max(), np.abs(B).max())
    check(f"rfc deform cols halo {halo}", np.abs(got - ref).max(), bilinear_bound(vmax, dpos) + 4 * U32 * vmax)


@pytest.mark.gpu
@pytest.mark.parametrize("h,w,halo", [(6, 5, 0), (4, 9, 2)])
def test_pp_deform_cols(K, h, w, halo):
    """DeformableAlignment's columns: 128 channels, 16 groups of 8, offset 3 tanh + flow.flip(1) (dy += flow_y, dx += flow_x)"""
    rng = np.random.default_rng(50 + h)
    Cc, ld, mag = 128, 436, 3.0
    x = rng.standard_normal((1, h, w, Cc)).astype(np.float32)
    off = np.full((h * w, ld), np.nan, dtype=np.float32)
    off[:, :432] = _offset_logits(rng, h * w)
    flow = rng.uniform(-6, 6, (2, h, w)).astype(np.float32)
    flow[:, 0, :] = np.round(flow[:, 0, :])                      # integer flows: with a zero offset the taps land on pixels
    cols = sent(h * w * 9 * Cc)
    launch(K.vsr_pp_launch_deform_cols, ptr(dev(with_halo(x, halo, np.nan))), ptr(dev(off)), ld, ptr(dev(flow)), mag, h, w, halo, Cc,
           ptr(cols))
    got = _kernel_cols(cols.cpu().numpy().reshape(h * w, 9 * Cc), Cc)
    o64 = off[:, :432].astype(np.float64).reshape(1, h, w, 432).transpose(0, 3, 1, 2)
    f64 = flow.astype(np.float64)
    offset = mag * np.tanh(o64[:, :288])
    offset[:, 0::2] += f64[1]
    offset[:, 1::2] += f64[0]
    ref = _deform_ref(torch.from_numpy(x.astype(np.float64)).permute(0, 3, 1, 2), torch.from_numpy(offset),
                      torch.from_numpy(1 / (1 + np.exp(-o64[:, 288:]))))
    ref = ref.permute(0, 3, 4, 1, 2).reshape(h * w, Cc, 9).numpy()
    dpos = U32 * (4 * mag + 4 * (mag + 6 + h + w))
    vmax = np.abs(x).max()
    check(f"pp deform cols {h}x{w} halo {halo}", np.abs(got - ref).max(), bilinear_bound(vmax, dpos) + 4 * U32 * vmax)


# =====================================================================================================================================
# ProPainter generator
# =====================================================================================================================================
@pytest.mark.gpu
@pytest.mark.parametrize("h,w,halo", [(7, 9, 1), (2, 6, 1), (5, 2, 0)])
def test_featprop_prep(K, h, w, halo):
    """flow_warp (grid_sample, align_corners=True, zeros; grid normalised by max(size-1, 1)) of the propagated feature and of the
    check flow, and misc = (flow_x, flow_y, valid, mask_in, mask_updated).  Flows point out of the frame and onto its last row and
    column.  `valid` is compared where its float64 margin exceeds the fp32 error of both sides of the threshold."""
    from oracle.propainter import flow_warp

    rng = np.random.default_rng(60 + h + w)
    Cc = 16
    prop = rng.standard_normal((1, h, w, Cc)).astype(np.float32)
    fprop = rng.uniform(-2, 2, (2, h, w)).astype(np.float32)
    fprop[:, 0, :] = rng.uniform(-9, 9, (2, w))                   # out of the frame
    xs, ys = np.meshgrid(np.arange(w), np.arange(h))
    fprop[0, -1, :] = (w - 1) - xs[-1]                            # onto the last column
    fprop[1, :, -1] = (h - 1) - ys[:, -1]                         # onto the last row
    fcheck = (-fprop + rng.normal(0, 0.4, (2, h, w))).astype(np.float32)
    fcheck[:, :, 0] = rng.uniform(-3, 3, (2, h))
    fprop[:, 0, 0] = 0.0                                          # one consistent pixel in every case: |0 + 0|^2 < 0.5
    fcheck[:, 0, 0] = 0.0
    mslot = with_halo(rng.integers(0, 2, (1, h, w, Cc)).astype(np.float32), halo, np.nan)
    warped, misc = sent((h + 2 * halo) * (w + 2 * halo) * Cc), sent((h + 2 * halo) * (w + 2 * halo) * Cc)
    launch(K.vsr_pp_launch_featprop_prep, ptr(dev(with_halo(prop, halo, np.nan))), ptr(dev(fprop)), ptr(dev(fcheck)), ptr(dev(mslot)),
           h, w, halo, Cc, ptr(warped), ptr(misc))
    gw = warped.cpu().numpy().reshape(1, h + 2 * halo, w + 2 * halo, Cc)
    gm = misc.cpu().numpy().reshape(1, h + 2 * halo, w + 2 * halo, Cc)
    fl = torch.from_numpy(fprop.astype(np.float64)).permute(1, 2, 0).unsqueeze(0)
    ref = flow_warp(torch.from_numpy(prop.astype(np.float64)).permute(0, 3, 1, 2), fl).permute(0, 2, 3, 1).numpy()
    back = flow_warp(torch.from_numpy(fcheck.astype(np.float64)).unsqueeze(0), fl)[0].numpy()
    # position x + flow through normalise / un-normalise: 6 ulp of (|x + flow| + size)
    dpos = 6 * U32 * (np.abs(fprop).max() + max(h, w) + 1)
    inner = (slice(None), slice(halo, halo + h), slice(halo, halo + w))
    check(f"featprop warp {h}x{w}", np.abs(gw[inner] - ref).max(), bilinear_bound(np.abs(prop).max(), dpos))
    gi = gm[inner][0]
    assert np.array_equal(gi[..., 0], fprop[0]) and np.array_equal(gi[..., 1], fprop[1])
    assert np.array_equal(gi[..., 3:5], mslot[0, halo:halo + h, halo:halo + w, 0:2])
    f64 = fprop.astype(np.float64)
    dx, dy = f64[0] + back[0], f64[1] + back[1]
    lhs = dx * dx + dy * dy
    rhs = 0.01 * ((f64 ** 2).sum(0) + (back ** 2).sum(0)) + 0.5
    eb = bilinear_bound(np.abs(fcheck).max(), dpos)               # error of the warped check flow
    margin = 2 * (np.sqrt(lhs) + 1) * eb * 2 + 0.02 * (np.abs(back).sum(0) + 1) * eb + 8 * U32 * (lhs + rhs)
    decided = np.abs(lhs - rhs) > margin
    assert decided.mean() > 0.8 and (lhs < rhs)[decided].any() and (lhs >= rhs)[decided].any()
    assert np.array_equal(gi[..., 2][decided], (lhs < rhs)[decided].astype(np.float32)), "flow-consistency bit"
    for g, what in ((gw, "warped"), (gm, "misc")):
        untouched(g, halo_mask(1, h, w, Cc, halo), f"featprop {what} halo")
    untouched(gm[inner][..., 5:], np.ones_like(gm[inner][..., 5:], bool), "featprop misc channels 5..")


@pytest.mark.gpu
@pytest.mark.parametrize("Cc,fh,fw,gh,gw", [(512, 10, 9, 12, 12), (64, 5, 7, 8, 8), (192, 3, 4, 4, 4)])
def test_layernorm_and_pool(K, Cc, fh, fw, gh, gw):
    """nn.LayerNorm (eps 1e-5) over tokens into a padded token grid (C = 512 register path, 64 / 192 plain path), large-mean tokens
    included; padded cells keep the sentinel.  The test then zeroes them, as the plan's clean workspace is, and the depthwise 4x4 /
    stride 4 pool runs over the grid (fh, fw not multiples of 4) against F.conv2d(groups=C) in float64."""
    rng = np.random.default_rng(Cc + fh)
    t = 2
    x = rng.standard_normal((t, fh, fw, Cc)).astype(np.float32) * rng.uniform(0.5, 3, (t, fh, fw, 1)).astype(np.float32)
    x[0, 0, :] += 1e3
    x[1, -1, -1] = (1e3 + rng.uniform(-1, 1, Cc)).astype(np.float32)
    gamma = rng.uniform(0.5, 2, Cc).astype(np.float32)
    beta = rng.standard_normal(Cc).astype(np.float32)
    y = sent(t * gh * gw * Cc)
    launch(K.vsr_pp_launch_layernorm, ptr(dev(x)), ptr(dev(gamma)), ptr(dev(beta)), t, fh, fw, Cc, gh, gw, ptr(y))
    gy = y.cpu().numpy().reshape(t, gh, gw, Cc)
    x64 = x.astype(np.float64)
    ref = F.layer_norm(torch.from_numpy(x64), (Cc,), torch.from_numpy(gamma.astype(np.float64)), torch.from_numpy(beta.astype(np.float64)),
                       eps=1e-5).numpy()
    # fp32 mean: C/64 + 6 sequential / tree additions and a division -> dmean <= (C/64 + 7) u32 sum|x| / C; the two-pass variance
    # (C/64 + 8 roundings of sum d^2, the shifted mean adds only dmean^2) and 1/sqrtf: drstd / rstd <= (C/64 + 12) u32; the output
    # (x - mean) rstd g + b: 4 roundings
    L = Cc // 64 + 7
    mean = x64.mean(-1, keepdims=True)
    sd = np.sqrt(x64.var(-1, keepdims=True) + 1e-5)
    dmean = L * U32 * np.abs(x64).mean(-1, keepdims=True)
    d = np.abs(x64 - mean)
    bound = np.abs(gamma) * ((dmean + U32 * d) / sd + d / sd * ((L + 5) * U32 + (dmean / sd) ** 2)) + 4 * U32 * np.abs(ref)
    check(f"layernorm C={Cc} err / bound", float((np.abs(gy[:, :fh, :fw] - ref) / bound).max()), 1.0)
    pad = np.ones(gy.shape, bool)
    pad[:, :fh, :fw] = False
    untouched(gy, pad, "layernorm padded grid cells")
    gy[pad] = 0.0
    ph, pw = gh // 4, gw // 4
    wgt = rng.standard_normal((Cc, 16)).astype(np.float32)
    bias = rng.standard_normal(Cc).astype(np.float32)
    out = sent(t * ph * pw * Cc, extra=64)
    launch(K.vsr_pp_launch_pool, ptr(dev(gy)), ptr(dev(wgt)), ptr(dev(bias)), t, gh, gw, Cc, ph, pw, ptr(out))
    go = out.cpu().numpy()
    inp = torch.from_numpy(gy.astype(np.float64)).permute(0, 3, 1, 2)
    pref = F.conv2d(inp, torch.from_numpy(wgt.astype(np.float64)).reshape(Cc, 1, 4, 4), torch.from_numpy(bias.astype(np.float64)),
                    stride=4, groups=Cc).permute(0, 2, 3, 1).numpy()
    # 16 fp32 products and 16 additions onto the bias (no contraction): 33 ulp of sum |terms|
    terms = F.conv2d(inp.abs(), torch.from_numpy(np.abs(wgt).astype(np.float64)).reshape(Cc, 1, 4, 4), torch.from_numpy(np.abs(bias).astype(np.float64)),
                     stride=4, groups=Cc).permute(0, 2, 3, 1).numpy()
    check(f"pool C={Cc} {gh}x{gw}", float((np.abs(go[:pref.size].reshape(pref.shape) - pref) / (33 * U32 * terms)).max()), 1.0)
    untouched(go[pref.size:], np.ones(64, bool), "pool tail")


def _fold_ref(vec, t, fh, fw, h, w, Cc, normalize):
    """F.fold(kernel 7, stride 3, padding 3) of tap-major token rows [t*fh*fw][ld] -> [t, h, w, C]"""
    v = torch.from_numpy(vec[:, :49 * Cc].astype(np.float64)).reshape(t, fh * fw, 49, Cc).permute(0, 3, 2, 1).reshape(t, Cc * 49, fh * fw)
    out = F.fold(v, (h, w), 7, padding=3, stride=3)
    if normalize:
        out = out / F.fold(torch.ones_like(v), (h, w), 7, padding=3, stride=3)
    return out.permute(0, 2, 3, 1).numpy()


def _unfold_ref(m, Cc, gelu):
    """F.unfold(kernel 7, stride 3, padding 3) of [t, h, w, C] -> tap-major rows [t*fh*fw][49 C]"""
    t = m.shape[0]
    u = F.unfold(torch.from_numpy(m.astype(np.float64)).permute(0, 3, 1, 2), 7, padding=3, stride=3)     # [t, C*49, L]
    if gelu:
        u = 0.5 * u * (1 + torch.erf(u / math.sqrt(2.0)))
    return u.reshape(t, Cc, 49, -1).permute(0, 3, 2, 1).reshape(-1, 49 * Cc).numpy()


FOLD_CASES = [  # C, ld, h, w, halo, pointer offset: C, ld % 4 == 0 and aligned -> fold4; C = 6 or an offset -> plain fold
    (8, 400, 9, 7, 0, 0), (8, 400, 10, 12, 2, 0), (8, 400, 11, 8, 2, 1), (6, 296, 10, 11, 0, 0), (6, 296, 11, 9, 2, 0), (12, 592, 9, 13, 0, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("Cc,ld,h,w,halo,off", FOLD_CASES)
@pytest.mark.parametrize("normalize", [0, 1])
def test_fold(K, Cc, ld, h, w, halo, off, normalize):
    """SoftComp / FusionFeedForward fold of tap-major token rows into an NHWC map with a halo that keeps its sentinel"""
    rng = np.random.default_rng(Cc * 100 + h * 10 + w + normalize)
    t = 2
    fh, fw = (h - 1) // 3 + 1, (w - 1) // 3 + 1
    vec = rng.standard_normal((t * fh * fw, ld)).astype(np.float32)
    vec[:, 49 * Cc:] = np.nan                                     # columns beyond 49 C are not the fold's
    vbuf = torch.empty(vec.size + 4, dtype=torch.float32, device="cuda")
    vbuf[off:off + vec.size] = dev(vec.reshape(-1))
    out = sent(t * (h + 2 * halo) * (w + 2 * halo) * Cc)
    launch(K.vsr_pp_launch_fold, ptr(vbuf, off), ld, t, fh, fw, h, w, Cc, halo, normalize, ptr(out))
    got = out.cpu().numpy().reshape(t, h + 2 * halo, w + 2 * halo, Cc)
    ref = _fold_ref(vec, t, fh, fw, h, w, Cc, normalize)
    # at most 9 patches per pixel: 8 additions (+ 1 division): 9 ulp of the sum of magnitudes
    mag = _fold_ref(np.abs(vec), t, fh, fw, h, w, Cc, normalize)
    check(f"fold{'4' if Cc % 4 == 0 and off == 0 else ''} C={Cc} {h}x{w} halo {halo} norm {normalize}",
          float((np.abs(got[:, halo:halo + h, halo:halo + w] - ref) / (9 * U32 * mag + 1e-300)).max()), 1.0)
    untouched(got, halo_mask(t, h, w, Cc, halo), "fold halo")


@pytest.mark.gpu
@pytest.mark.parametrize("Cc,h,w", [(8, 9, 7), (12, 10, 11), (4, 11, 5)])
def test_unfold_and_fused_pair(K, Cc, h, w):
    """unfold + GELU (exact erf) and the plain unfold against F.unfold; K-padding columns (49 C .. ld) written as zero; and the
    fused pair fold_gelu -> unfold_plain gives fold -> unfold_gelu bit for bit"""
    rng = np.random.default_rng(Cc + h + w)
    t = 2
    fh, fw = (h - 1) // 3 + 1, (w - 1) // 3 + 1
    ld = 49 * Cc + 8
    m = (rng.standard_normal((t, h, w, Cc)) * 2).astype(np.float32)
    md = dev(m)
    for fn, gelu in ((K.vsr_pp_launch_unfold_gelu, True), (K.vsr_pp_launch_unfold_plain, False)):
        out = sent(t * fh * fw * ld)
        launch(fn, ptr(md), t, fh, fw, h, w, Cc, ld, ptr(out))
        got = out.cpu().numpy().reshape(t * fh * fw, ld)
        ref = _unfold_ref(m, Cc, gelu)
        # GELU: erff and three roundings, 6 ulp of |x|; the plain unfold is a copy
        check(f"unfold{' gelu' if gelu else ''} C={Cc} {h}x{w}", np.abs(got[:, :49 * Cc] - ref).max(), 6 * U32 * np.abs(m).max() if gelu else 0.0)
        assert np.all(got[:, 49 * Cc:] == 0.0), "K-padding columns must be written as zero"
    vec = rng.standard_normal((t * fh * fw, ld)).astype(np.float32)
    vd = dev(vec)
    a_map, b_map = sent(t * h * w * Cc), sent(t * h * w * Cc)
    a_tok, b_tok = sent(t * fh * fw * ld), sent(t * fh * fw * ld)
    launch(K.vsr_pp_launch_fold_gelu, ptr(vd), ld, t, fh, fw, h, w, Cc, 0, 1, ptr(a_map))
    launch(K.vsr_pp_launch_unfold_plain, ptr(a_map), t, fh, fw, h, w, Cc, ld, ptr(a_tok))
    launch(K.vsr_pp_launch_fold, ptr(vd), ld, t, fh, fw, h, w, Cc, 0, 1, ptr(b_map))
    launch(K.vsr_pp_launch_unfold_gelu, ptr(b_map), t, fh, fw, h, w, Cc, ld, ptr(b_tok))
    assert torch.equal(a_tok, b_tok), "fold_gelu -> unfold_plain must equal fold -> unfold_gelu bit for bit"


# =====================================================================================================================================
# LaMa
# =====================================================================================================================================
LAMA_SIZES = [(H, W, halo) for H in (2, 3, 5, 45) for W in (2, 3, 5, 45) for halo in (1, 3) if halo < min(H, W)]


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,halo", LAMA_SIZES)
def test_lama_halo(K, H, W, halo):
    """reflect halo (ReflectionPad2d: defined for halo < H, W) in place: every halo cell, corners included, equals
    np.pad(mode="reflect") of the interior; the interior is not touched"""
    rng = np.random.default_rng(H * 100 + W * 10 + halo)
    n, Cc = 2, 8
    x = rng.standard_normal((n, H, W, Cc)).astype(np.float32)
    xd = dev(with_halo(x, halo))
    launch(K.vsr_lama_launch_halo, ptr(xd), n, H, W, Cc, halo)
    want = np.pad(x, ((0, 0), (halo, halo), (halo, halo), (0, 0)), mode="reflect")
    assert np.array_equal(xd.cpu().numpy(), want)


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,halo", [(2, 3, 1), (5, 45, 3), (45, 5, 1), (3, 3, 1)])
@pytest.mark.parametrize("reflect", [0, 1])
def test_lama_add_halo(K, H, W, halo, reflect):
    """dst = a + b over the padded frame: the halo takes the reflected interior sum (reflect = 1) or keeps its sentinel (0)"""
    rng = np.random.default_rng(H + W + halo + reflect)
    n, Cc = 2, 8
    a = rng.standard_normal((n, H, W, Cc)).astype(np.float32)
    b = rng.standard_normal((n, H, W, Cc)).astype(np.float32)
    dst = sent(n * (H + 2 * halo) * (W + 2 * halo) * Cc)
    launch(K.vsr_lama_launch_add_halo, ptr(dev(with_halo(a, halo, np.nan))), ptr(dev(with_halo(b, halo, np.nan))), ptr(dst), n, H, W, Cc,
           halo, reflect)
    got = dst.cpu().numpy().reshape(n, H + 2 * halo, W + 2 * halo, Cc)
    s = (a.astype(np.float64) + b).astype(np.float32)             # one correctly rounded fp32 addition
    if reflect:
        assert np.array_equal(got, np.pad(s, ((0, 0), (halo, halo), (halo, halo), (0, 0)), mode="reflect"))
    else:
        assert np.array_equal(got[:, halo:halo + H, halo:halo + W], s)
        untouched(got, halo_mask(n, H, W, Cc, halo), "add_halo without reflect")


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,W,Hp,Wp", [(2, 5, 7, 8, 8), (1, 45, 13, 48, 16), (1, 4, 8, 8, 8), (2, 13, 6, 16, 8)])
def test_lama_im2col7(K, B, H, W, Hp, Wp):
    """pad_img_to_modulo (np.pad symmetric to Hp x Wp), then the 7x7 conv's reflect padding of the padded frame: columns of
    (image / 255 * (1 - mask), mask), tap-major, 196 -> 224 with zero K padding"""
    rng = np.random.default_rng(H * W + Hp)
    img = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    mask = (rng.random((B, H, W)) < 0.3).astype(np.uint8) * rng.integers(1, 256, (B, H, W), dtype=np.uint8)
    cols = sent(B * Hp * Wp * 224)
    launch(K.vsr_lama_launch_im2col7, ptr(dev(img)), ptr(dev(mask)), B, H, W, Hp, Wp, ptr(cols))
    got = cols.cpu().numpy().reshape(B, Hp, Wp, 56, 4)
    m = (mask > 0).astype(np.float32)
    x = np.concatenate([(img.astype(np.float32) / np.float32(255)) * (1 - m)[..., None], m[..., None]], -1)
    x = np.pad(x, ((0, 0), (0, Hp - H), (0, Wp - W), (0, 0)), mode="symmetric")
    x = np.pad(x, ((0, 0), (3, 3), (3, 3), (0, 0)), mode="reflect")
    ref = np.stack([x[:, ky:ky + Hp, kx:kx + Wp] for ky in range(7) for kx in range(7)], 3).astype(np.float32)
    assert np.array_equal(got[:, :, :, :49], ref), "x.astype(float32) / 255 is one correctly rounded division; the mask factor is exact"
    assert np.all(got[:, :, :, 49:] == 0.0)


@pytest.mark.gpu
def test_lama_out(K):
    """sigmoid, mask * pred + (1 - mask) * image, clip(x * 255, 0, 255) truncated to uint8 and cropped; logits of +-100 saturate.
    One level of difference is allowed only where the float64 value lies within 1e-4 of an integer (truncation can fall either
    side there); everywhere else the bytes are equal"""
    rng = np.random.default_rng(9)
    B, H, W, Hp, Wp = 2, 13, 22, 16, 24
    logits = (rng.standard_normal((B, Hp // 4, Wp // 4, 64)) * 3).astype(np.float32)
    logits[0, 0, 0, :] = 100.0
    logits[1, 1, 1, :] = -100.0
    img = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    mask = (rng.random((B, H, W)) < 0.5).astype(np.uint8) * 255
    out = torch.full((B * H * W * 3,), 77, dtype=torch.uint8, device="cuda")
    launch(K.vsr_lama_launch_out, ptr(dev(logits)), ptr(dev(img)), ptr(dev(mask)), B, H, W, Hp, Wp, ptr(out))
    got = out.cpu().numpy().reshape(B, H, W, 3).astype(np.int64)
    lg = logits[:, :, :, :48].reshape(B, Hp // 4, Wp // 4, 4, 4, 3).transpose(0, 1, 3, 2, 4, 5).reshape(B, Hp, Wp, 3)[:, :H, :W].astype(np.float64)
    p = 1 / (1 + np.exp(-lg))
    m = (mask > 0).astype(np.float64)[..., None]
    v = np.clip((m * p + (1 - m) * img / 255.0) * 255, 0, 255)
    ref = np.floor(v).astype(np.int64)
    near = np.abs(v - np.round(v)) <= 1e-4
    d = np.abs(got - ref)
    assert np.all(d[~near] == 0) and np.all(d[near] <= 1), f"{int((d[~near] != 0).sum())} bytes differ away from an integer"


# =====================================================================================================================================
# The small elementwise kernels: odd sizes, saturating inputs
# =====================================================================================================================================
def _state(rng, pairs, h, w, halo, Chx):
    return rng.standard_normal((pairs, h + 2 * halo, w + 2 * halo, Chx)).astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("h,w,halo", [(3, 5, 1), (1, 7, 0)])
def test_gru_gates(K, h, w, halo):
    """SepConvGRU: r * h into channels chRH.. and h = (1 - z) h + z tanh(q) in channels chH..; z, r, q up to +-100.  Nothing else
    of the state changes."""
    rng = np.random.default_rng(h * w + halo)
    pairs, Chx, chH, chRH = 2, 392, 4, 260
    M = pairs * h * w
    zr = (rng.standard_normal((M, 256)) * 4).astype(np.float32)
    zr[::3, :] = 100.0
    zr[1::3, ::2] = -100.0
    q = (rng.standard_normal((M, 128)) * 4).astype(np.float32)
    q[::4] = -100.0
    s0 = _state(rng, pairs, h, w, halo, Chx)
    sd = dev(s0)
    launch(K.vsr_raft_launch_gru_rh, ptr(dev(zr)), ptr(sd), pairs, h, w, halo, Chx, chH, chRH)
    s1 = sd.cpu().numpy()
    inner = (slice(None), slice(halo, halo + h), slice(halo, halo + w))
    hv = s0[inner][..., chH:chH + 128].astype(np.float64).reshape(M, 128)
    ref = hv / (1 + np.exp(-zr[:, 128:].astype(np.float64)))
    # sigmoid: expf, an addition and a division (4 ulp), the product (1 ulp)
    check(f"gru r*h {h}x{w}", np.abs(s1[inner][..., chRH:chRH + 128].reshape(M, 128) - ref).max(), 5 * U32 * np.abs(hv).max())
    keep = np.ones(s0.shape, bool)
    keep[inner + (slice(chRH, chRH + 128),)] = False
    assert np.array_equal(s1[keep], s0[keep]), "gru_rh wrote outside channels chRH..chRH+127 of the interior"
    launch(K.vsr_raft_launch_gru_update, ptr(dev(zr)), ptr(dev(q)), ptr(sd), pairs, h, w, halo, Chx, chH)
    s2 = sd.cpu().numpy()
    z = 1 / (1 + np.exp(-zr[:, :128].astype(np.float64)))
    ref = (1 - z) * hv + z * np.tanh(q.astype(np.float64))
    # z 4 ulp (absolute, z <= 1), 1 - z 1 ulp, tanhf 4 ulp, two products and a sum: 10 ulp of (|h| + 1)
    check(f"gru update {h}x{w}", np.abs(s2[inner][..., chH:chH + 128].reshape(M, 128) - ref).max(), 10 * U32 * (np.abs(hv).max() + 1))
    keep = np.ones(s0.shape, bool)
    keep[inner + (slice(chH, chH + 128),)] = False
    assert np.array_equal(s2[keep], s1[keep]), "gru_update wrote outside channels chH..chH+127 of the interior"


@pytest.mark.gpu
def test_ctx_split(K):
    """net = tanh, inp = relu of the context map of frameOf[p], into channels 0..255 of the state; other channels and the halo keep
    the sentinel"""
    rng = np.random.default_rng(11)
    frames, pairs, h, w, halo, Chx = 3, 4, 5, 3, 1, 264
    frame_of = np.array([2, 0, 2, 1], dtype=np.int32)
    cmap = (rng.standard_normal((frames, h, w, 256)) * 3).astype(np.float32)
    cmap[1, 0, 0, :] = 100.0
    cmap[2, 1, 1, :] = -100.0
    hxr = sent(pairs * (h + 2 * halo) * (w + 2 * halo) * Chx)
    launch(K.vsr_raft_launch_ctx_split, ptr(dev(cmap)), ptr(dev(frame_of)), pairs, h, w, halo, Chx, ptr(hxr))
    got = hxr.cpu().numpy().reshape(pairs, h + 2 * halo, w + 2 * halo, Chx)
    src = cmap[frame_of].astype(np.float64)
    inner = got[:, halo:halo + h, halo:halo + w]
    check("ctx split tanh", np.abs(inner[..., :128] - np.tanh(src[..., :128])).max(), 4 * U32)
    assert np.array_equal(inner[..., 128:256], np.maximum(cmap[frame_of][..., 128:256], 0))
    other = halo_mask(pairs, h, w, Chx, halo)
    other[:, halo:halo + h, halo:halo + w, 256:] = True
    untouched(got, other, "ctx split")


@pytest.mark.gpu
@pytest.mark.parametrize("init", [0, 1])
def test_flow_update(K, init):
    """coords1 = coords0 (init) or coords1 + delta; flow = coords1 - coords0 into the flow buffer and channels chFlow, chFlow + 1 of
    the state (whose other cells keep the sentinel)"""
    rng = np.random.default_rng(21 + init)
    pairs, h, w, halo, Chx, chFlow, ldd = 2, 3, 7, 1, 136, 130, 6
    M = pairs * h * w
    delta = (rng.standard_normal((M, ldd)) * 5).astype(np.float32)
    coords = (rng.standard_normal((M, 2)) * 30 + 10).astype(np.float32)
    cd, fl, hxr = dev(coords), sent(2 * M), sent(pairs * (h + 2 * halo) * (w + 2 * halo) * Chx)
    launch(K.vsr_raft_launch_flow_update, ptr(dev(delta)), ldd, ptr(cd), ptr(fl), ptr(hxr), pairs, h, w, init, halo, Chx, chFlow)
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    c0 = np.stack([np.tile(xs.reshape(-1), pairs), np.tile(ys.reshape(-1), pairs)], 1).astype(np.float64)
    c1 = c0 if init else coords.astype(np.float64) + delta[:, :2]
    gc, gf = cd.cpu().numpy(), fl.cpu().numpy().reshape(M, 2)
    # one fp32 addition and one subtraction
    check(f"flow update coords init={init}", np.abs(gc - c1).max(), U32 * np.abs(c1).max())
    check(f"flow update flow init={init}", np.abs(gf - (c1 - c0)).max(), 2 * U32 * (np.abs(c1).max() + w))
    st = hxr.cpu().numpy().reshape(pairs, h + 2 * halo, w + 2 * halo, Chx)
    assert np.array_equal(st[:, halo:halo + h, halo:halo + w, chFlow:chFlow + 2].reshape(M, 2), gf)
    other = np.ones(st.shape, bool)
    other[:, halo:halo + h, halo:halo + w, chFlow:chFlow + 2] = False
    untouched(st, other, "flow update state")


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,bgr", [(9, 13, 0), (7, 5, 1), (16, 10, 1)])
def test_im2col7_u8(K, H, W, bgr):
    """to_tensors() * 2 - 1 and the stem conv's im2col (7x7, stride 2, pad 3; zero padding after the transform): rows of the
    kernel's H/2 x W/2 outputs, 147 -> 160 columns with zero K padding"""
    rng = np.random.default_rng(H * W + bgr)
    n = 2
    img = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    oh, ow = H // 2, W // 2
    out = sent(n * oh * ow * 160)
    launch(K.vsr_raft_launch_im2col7_u8, ptr(dev(img)), n, H, W, bgr, ptr(out))
    got = out.cpu().numpy().reshape(n, oh, ow, 160)
    x = img[..., ::-1] if bgr else img
    x = torch.from_numpy(np.ascontiguousarray(x).astype(np.float64) / 255 * 2 - 1).permute(0, 3, 1, 2)
    u = F.unfold(x, 7, padding=3, stride=2).reshape(n, 3, 49, (H + 1) // 2, (W + 1) // 2)[:, :, :, :oh, :ow]
    ref = u.permute(0, 3, 4, 2, 1).reshape(n, oh, ow, 147).numpy()
    # u / 255 (1 ulp of <= 1), * 2 (exact), - 1 (1 ulp of <= 1)
    check(f"im2col7 u8 {H}x{W} bgr {bgr}", np.abs(got[..., :147] - ref).max(), 3 * U32)
    assert np.all(got[..., 147:] == 0.0)


@pytest.mark.gpu
def test_im2col7_flow(K):
    rng = np.random.default_rng(31)
    pairs, h, w = 2, 5, 9
    flow = rng.standard_normal((pairs, h, w, 2)).astype(np.float32)
    out = sent(pairs * h * w * 128)
    launch(K.vsr_raft_launch_im2col7_flow, ptr(dev(flow)), pairs, h, w, ptr(out))
    got = out.cpu().numpy().reshape(pairs * h * w, 128)
    u = F.unfold(torch.from_numpy(flow).permute(0, 3, 1, 2), 7, padding=3).reshape(pairs, 2, 49, h * w)
    ref = u.permute(0, 3, 2, 1).reshape(pairs * h * w, 98).numpy()
    assert np.array_equal(got[:, :98], ref) and np.all(got[:, 98:] == 0.0)


@pytest.mark.gpu
def test_rfc_im2col5_and_combine(K):
    """forward_bidirect_flow's masking + the stem Conv3d (1,5,5) / stride 2 im2col with replicate padding; then combine_flow with
    the backward sequence un-flipped"""
    rng = np.random.default_rng(41)
    t, H, W = 4, 10, 14
    T = t - 1
    ff = rng.standard_normal((T, 2, H, W)).astype(np.float32) * 4
    fb = rng.standard_normal((T, 2, H, W)).astype(np.float32) * 4
    mask = (rng.random((t, H, W)) < 0.4).astype(np.uint8) * rng.integers(1, 256, (t, H, W), dtype=np.uint8)
    oh, ow = H // 2, W // 2
    out = sent(2 * T * oh * ow * 96)
    dff, dfb, dm = dev(ff), dev(fb), dev(mask)
    launch(K.vsr_rfc_launch_im2col5, ptr(dff), ptr(dfb), ptr(dm), t, H, W, ptr(out))
    got = out.cpu().numpy().reshape(T, 2, oh, ow, 96)
    m = (mask != 0).astype(np.float32)
    for s, flows, masks in ((0, ff, m[:-1]), (1, fb[::-1], m[1:][::-1])):
        x = np.concatenate([flows * (1 - masks[:, None]), masks[:, None]], 1)
        xp = F.pad(torch.from_numpy(np.ascontiguousarray(x)), (2, 2, 2, 2), mode="replicate")
        u = F.unfold(xp, 5, stride=2).reshape(T, 3, 25, oh, ow).permute(0, 3, 4, 2, 1).reshape(T, oh, ow, 75).numpy()
        assert np.array_equal(got[:, s, :, :, :75], u), f"im2col5 sequence {s}"
    assert np.all(got[..., 75:] == 0.0)
    ld = 6
    pred = rng.standard_normal((2 * T * H * W, ld)).astype(np.float32)
    oF, oB = sent(T * 2 * H * W), sent(T * 2 * H * W)
    launch(K.vsr_rfc_launch_combine, ptr(dev(pred)), ld, ptr(dff), ptr(dfb), ptr(dm), t, H, W, ptr(oF), ptr(oB))
    pr = pred.reshape(T, 2, H, W, ld)[..., :2].transpose(0, 1, 4, 2, 3)       # [step][s][c][H][W]
    predF, predB = pr[:, 0], pr[::-1, 1]                                       # the backward sequence ran flipped
    wantF = predF * m[:-1, None] + (ff * (1 - m[:-1, None])) * (1 - m[:-1, None])
    wantB = predB * m[1:, None] + (fb * (1 - m[1:, None])) * (1 - m[1:, None])
    assert np.array_equal(oF.cpu().numpy().reshape(T, 2, H, W), wantF)
    assert np.array_equal(oB.cpu().numpy().reshape(T, 2, H, W), wantB)


@pytest.mark.gpu
def test_pp_small_kernels(K):
    """ds_flow (bilinear 1/4, align_corners=False, / 4), ds_mask (nearest 1/4 into channels 0, 1 of a halo'd slot), im2col3
    (cat[frames, masks] and the 3x3 / stride 2 / pad 1 im2col, 45 -> 64) and tanh_out (+-100 saturate)"""
    rng = np.random.default_rng(51)
    n, H, W = 3, 20, 28
    src = rng.standard_normal((2 * n, H, W)).astype(np.float32) * 8
    out = sent(2 * n * (H // 4) * (W // 4))
    launch(K.vsr_pp_launch_ds_flow, ptr(dev(src)), 2 * n, H, W, ptr(out))
    ref = F.interpolate(torch.from_numpy(src.astype(np.float64)).unsqueeze(1), scale_factor=0.25, mode="bilinear",
                        align_corners=False).squeeze(1).numpy() / 4.0
    check("ds_flow", np.abs(out.cpu().numpy().reshape(ref.shape) - ref).max(), 4 * U32 * np.abs(src).max() / 4)
    m1 = rng.integers(0, 2, (n, H, W), dtype=np.uint8) * 200
    m2 = rng.integers(0, 2, (n, H, W), dtype=np.uint8)
    halo, Cc = 1, 8
    h, w = H // 4, W // 4
    slots = sent(n * (h + 2) * (w + 2) * Cc)
    launch(K.vsr_pp_launch_ds_mask, ptr(dev(m1)), ptr(dev(m2)), n, H, W, ptr(slots), halo, Cc)
    gs = slots.cpu().numpy().reshape(n, h + 2, w + 2, Cc)
    for c, mk in ((0, m1), (1, m2)):
        near = F.interpolate(torch.from_numpy((mk != 0).astype(np.float64)).unsqueeze(1), scale_factor=0.25, mode="nearest").squeeze(1).numpy()
        assert np.array_equal(gs[:, 1:1 + h, 1:1 + w, c], near)
    other = halo_mask(n, h, w, Cc, halo)
    other[:, 1:1 + h, 1:1 + w, 2:] = True
    untouched(gs, other, "ds_mask slot")
    frames = rng.standard_normal((n, 3, H, W)).astype(np.float32)
    cols = sent(n * (H // 2) * (W // 2) * 64)
    launch(K.vsr_pp_launch_im2col3, ptr(dev(frames)), ptr(dev(m1)), ptr(dev(m2)), n, H, W, ptr(cols))
    x = torch.from_numpy(np.concatenate([frames, (m1 != 0)[:, None].astype(np.float32), (m2 != 0)[:, None].astype(np.float32)], 1))
    u = F.unfold(x, 3, padding=1, stride=2).reshape(n, 5, 9, -1).permute(0, 3, 2, 1).reshape(-1, 45).numpy()
    gc = cols.cpu().numpy().reshape(-1, 64)
    assert np.array_equal(gc[:, :45], u) and np.all(gc[:, 45:] == 0.0)
    ld = 8
    y = (rng.standard_normal((n * H * W, ld)) * 3).astype(np.float32)
    y[::7, :3] = 100.0
    y[1::7, :3] = -100.0
    to = sent(n * 3 * H * W)
    launch(K.vsr_pp_launch_tanh_out, ptr(dev(y)), ld, n, H, W, ptr(to))
    ref = np.tanh(y[:, :3].astype(np.float64)).reshape(n, H, W, 3).transpose(0, 3, 1, 2)
    check("tanh_out", np.abs(to.cpu().numpy().reshape(n, 3, H, W) - ref).max(), 4 * U32)


# =====================================================================================================================================
# ProPainter image propagation (pp_kernels.hip: k_pp_imgprop, k_pp_mask_f32, k_pp_mask_u8) against tests/_pp_glue_ref.py, the numpy
# restatement of propagate() that tests/test_pp_glue_reference.py holds against the torch oracle bit for bit
# =====================================================================================================================================
def _imgprop_launch(K, inp, first):
    """one launch into sentinel-filled outputs with 64 floats behind each, which must keep the sentinel"""
    Cc, h, w = inp["cur"].shape
    prop, mprop = sent(Cc * h * w, extra=64), sent(h * w, extra=64)
    launch(K.vsr_pp_launch_imgprop, ptr(dev(inp["prev_prop"])), ptr(dev(inp["prev_mask"])), ptr(dev(inp["cur"])), ptr(dev(inp["mcur"])),
           ptr(dev(inp["fprop"])), ptr(dev(inp["fcheck"])), Cc, h, w, first, ptr(prop), ptr(mprop))
    gp, gm = prop.cpu().numpy(), mprop.cpu().numpy()
    untouched(gp[Cc * h * w:], np.ones(64, bool), "imgprop prop tail")
    untouched(gm[h * w:], np.ones(64, bool), "imgprop mprop tail")
    return gp[:Cc * h * w].reshape(Cc, h, w), gm[:h * w].reshape(h, w)


@pytest.mark.gpu
@pytest.mark.parametrize("Cc", [3, 1])
@pytest.mark.parametrize("h,w", [(9, 17), (17, 33), (2, 9)])
def test_imgprop_dyadic_grid_exact(K, h, w, Cc):
    """h - 1 and w - 1 are powers of two and the flows multiples of 1/4: x + f, 2 pos / (size - 1), the un-normalisation and the
    bilinear weights (multiples of 1/4, products multiples of 1/16, on check flows that are multiples of 1/4) are exact in fp32, so
    every sampling position, tie included, is the float64 one and there is no margin: prop and mprop equal the restatement bit for
    bit.  step_conditions asserts the shares of ties (>= 20 %, on even and odd lower neighbours), of nearest targets and bilinear
    footprints outside the picture (>= 5 %, every side), of the eight (mcur, valid, mvalid) combinations and of the union branch
    (some of it on targets outside the picture: the zero padding of the nearest warp), and that no forward-backward or mask decision is within fp32 rounding of its threshold (2x9: what 18 pixels can hold)."""
    import _pp_glue_ref as R

    inp = R.imgprop_inputs(R.step_seed(h, w), h, w, Cc, 0.0)
    prop, mprop, info, _ = R.step_conditions(inp, True)
    gp, gm = _imgprop_launch(K, inp, 0)
    dp, dm = int((gp != prop).any(0).sum()), int((gm != mprop).sum())
    print(f"imgprop dyadic {h}x{w} C={Cc}: {dp} pixels and {dm} mask cells differ (bound 0)")
    assert dp == 0 and dm == 0


def _imgprop_general_check(inp, gp, gm, prop, mprop, info, und, what):
    """bit equality on decided pixels; an undecided pixel holds one of its candidates: cur or the propagated picture at one of the
    four integer positions around the sampling position (zero outside), mask 0 or 1"""
    import _pp_glue_ref as R

    dec = ~und
    dp, dm = int(((gp != prop).any(0) & dec).sum()), int(((gm != mprop) & dec).sum())
    print(f"{what}: {dp} decided pixels and {dm} decided mask cells differ (bound 0); undecided {und.mean():.5f} (cap 0.005)")
    assert dp == 0 and dm == 0
    y0, x0 = np.floor(info["iy"]).astype(np.int64), np.floor(info["ix"]).astype(np.int64)
    cands = [inp["cur"]] + [R.gather(inp["prev_prop"], y0 + dy, x0 + dx) for dy in (0, 1) for dx in (0, 1)]
    anyc = np.any([gp == c for c in cands], axis=0).all(0)
    assert anyc[und].all() and np.isin(gm[und], (0.0, 1.0)).all(), "an undecided pixel holds none of its candidates"


@pytest.mark.gpu
@pytest.mark.parametrize("Cc", [3, 1])
@pytest.mark.parametrize("h,w", [(13, 22), (45, 75), (2, 3)])
def test_imgprop_general_grid(K, h, w, Cc):
    """Sizes whose positions round in fp32 (2x3: size - 1 = 1, the normalisation's max(size - 1, 1)), flows with N(0, 0.2) on top of
    the blocks.  A pixel is undecided where a float64 margin (forward-backward test, warped mask against 0.1, nearest position
    against a .5 tie) is below what fp32 can move it by -- R.imgprop_bounds derives it from u = 2^-24 and the magnitudes involved;
    step_conditions caps their share at 0.5 % (these inputs: 0 to 6e-4) and asserts the branch shares as on the dyadic grid."""
    import _pp_glue_ref as R

    inp = R.imgprop_inputs(R.step_seed(h, w), h, w, Cc, 0.2)
    prop, mprop, info, und = R.step_conditions(inp, False)
    gp, gm = _imgprop_launch(K, inp, 0)
    _imgprop_general_check(inp, gp, gm, prop, mprop, info, und, f"imgprop general {h}x{w} C={Cc}")


@pytest.mark.gpu
def test_imgprop_second_turn_of_the_stride_loop(K):
    """h w = 1449 x 1448 = 2 097 152 + 1000 pixels: the grid is capped at 8192 blocks of 256 threads, so 1000 threads take a
    second pixel (1080p stays below the cap).  fp32 positions are 1e-4 wide at x = 1448, so this case keeps the check flow free of
    per-pixel noise and sends no block a picture's width away: 0.42 % of its pixels are undecided (cap 0.5 %)"""
    import _pp_glue_ref as R

    h, w = R.LARGE_SIZE
    assert h * w == 8192 * 256 + 1000
    inp = R.imgprop_inputs(R.step_seed(h, w), h, w, 3, 0.2, far=False, bad=0.1, check_noise=False)
    prop, mprop, info, und = R.step_conditions(inp, False, oob=False)
    gp, gm = _imgprop_launch(K, inp, 0)
    _imgprop_general_check(inp, gp, gm, prop, mprop, info, und, f"imgprop {h}x{w}")
    sel = ~und[-1, -1000:]                              # the pixels of the second turn: the union branch is taken among them too
    assert sel.sum() > 900 and (info["union"][-1, -1000:][sel] == 1).any()
    assert np.array_equal(gp[:, -1, -1000:][:, sel], prop[:, -1, -1000:][:, sel]) and np.array_equal(gm[-1, -1000:][sel], mprop[-1, -1000:][sel])


@pytest.mark.gpu
@pytest.mark.parametrize("h,w,Cc", [(9, 17, 3), (45, 75, 1)])
def test_imgprop_first_step_copies(K, h, w, Cc):
    """first = 1: prop and mprop are copies of cur and mcur; the propagated picture, its mask and both flows are NaN and none of it
    reaches the output"""
    import _pp_glue_ref as R

    inp = R.imgprop_inputs(R.step_seed(h, w), h, w, Cc, 0.0)
    inp = {k: (v if k in ("cur", "mcur") else np.full_like(v, np.nan)) for k, v in inp.items()}
    gp, gm = _imgprop_launch(K, inp, 1)
    assert np.array_equal(gp.view(np.uint32), inp["cur"].view(np.uint32)) and np.array_equal(gm.view(np.uint32), inp["mcur"].view(np.uint32))


MASK_N = (1, 255, 257, 8192 * 256 + 77)               # below / above one block, and the second turn of the capped grid


@pytest.mark.gpu
@pytest.mark.parametrize("n", MASK_N)
def test_pp_mask_f32(K, n):
    """u8 -> fp32 {0, 1}: any non-zero byte is a hole; from n = 257 on all 256 byte values occur"""
    src = ((np.arange(n, dtype=np.int64) * 37 + 255) % 256).astype(np.uint8)
    assert n < 256 or len(np.unique(src)) == 256
    out = sent(n, extra=64)
    launch(K.vsr_pp_launch_mask_f32, ptr(dev(src)), n, ptr(out))
    got = out.cpu().numpy()
    assert np.array_equal(got[:n], (src != 0).astype(np.float32)) and set(np.unique(got[:n])) <= {0.0, 1.0}
    untouched(got[n:], np.ones(64, bool), "mask_f32 tail")


@pytest.mark.gpu
@pytest.mark.parametrize("n", MASK_N)
def test_pp_mask_u8(K, n):
    """fp32 -> u8: 1 where the value exceeds 0.5 -- 0.5 itself, its lower neighbour, 0, -0.0, 0.1 and NaN give 0; the upper
    neighbour of 0.5 and 1 give 1"""
    half = np.float32(0.5)
    special = np.array([half, np.nextafter(half, np.float32(1)), np.nextafter(half, np.float32(0)), 0.0, 1.0, -0.0, 0.1, np.nan], dtype=np.float32)
    want8 = np.array([0, 1, 0, 0, 1, 0, 0, 0], dtype=np.uint8)
    idx = (np.arange(n) * 3 + 1) % 8                   # n = 1: the upper neighbour of 0.5
    out = torch.full((n + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    launch(K.vsr_pp_launch_mask_u8, ptr(dev(special[idx])), n, ptr(out))
    got = out.cpu().numpy()
    assert np.array_equal(got[:n], want8[idx])
    assert np.all(got[n:] == 0xA5), "mask_u8 wrote behind its n bytes"


@pytest.mark.gpu
def test_pp_mask_empty(K):
    """n = 0: both launchers return 0 and write nothing"""
    f, b = sent(64), torch.full((64,), 0xA5, dtype=torch.uint8, device="cuda")
    launch(K.vsr_pp_launch_mask_f32, ptr(b), 0, ptr(f))
    launch(K.vsr_pp_launch_mask_u8, ptr(f), 0, ptr(b))
    assert np.all(f.cpu().numpy() == SENT) and np.all(b.cpu().numpy() == 0xA5)
