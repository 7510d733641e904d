"""Child process of tests/test_pad_taps.py: the library reads VSR_SKIP_PAD_TAPS once, so each setting gets a process of its own.
Replays the three-window sttn-auto plan of L = 12 frames on the CPU (tests/_replay.py) -- once without a promise about the mask
rows, once with mask rows that reach the bottom border of the strip -- checks both against the oracle as tests/_replay_check.py
does, and prints one JSON line: digests of the composites, the FLOP counts of both plans, the state of the switch.
With --structure it checks the tables of the band problems instead (check_structure) and prints what it saw.

The replay's own GEMM is one torch matmul per problem, and a CPU matmul blocks its K loop by the problem's shape: a problem with K = 6 * cin
and the same problem with three more zero taps per channel chunk round differently there, which says nothing about the plan.  The kernels
accumulate chunk after chunk in the order of the chunk tables, so the problems that read the packed weights are replayed that way here
(gemm_chunk_order: one 32-deep product per chunk, every call of the same shape); everything else stays with tests/_replay.py."""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

L, ROWS = 12, (84, 120)
BLOCK = 1024

# input / output activation of every conv that goes through Plan::addConv with stride 1: (halo, channels) of the input, halo and channels
# of the output, dilation, scale of the map against the feature map (Plan::buildWindow, Plan::Plan)
CONVS = {
    "attn.out": dict(hin=1, cin=256, hout=2, cout=256, dil=1, scale=1),
    "ffn.1": dict(hin=2, cin=256, hout=1, cout=256, dil=2, scale=1),
    "ffn.2": dict(hin=1, cin=256, hout=2, cout=256, dil=1, scale=1),
    "dec.1": dict(hin=1, cin=256, hout=1, cout=128, dil=1, scale=2),
    "dec.2": dict(hin=1, cin=128, hout=0, cout=64, dil=1, scale=2),
    "dec.3": dict(hin=1, cin=64, hout=1, cout=64, dil=1, scale=4),
}


def _pixels(rows, H, W, C, halo):
    """element offsets of pixels of an NHWC activation with a physical halo -> (frame, y, x)"""
    Hp, Wp = H + 2 * halo, W + 2 * halo
    assert (rows % C == 0).all()
    p = rows // C
    f, r = p // (Hp * Wp), p % (Hp * Wp)
    return f, r // Wp - halo, r % Wp - halo


def check_structure(view, fh, fw):
    seen = {}
    for info, items in view.ops:
        tag = info.tag.decode()
        if info.kind != 1 or tag not in CONVS or len(items) < 2:
            continue
        g = CONVS[tag]
        H, W, cin, dil = fh * g["scale"], fw * g["scale"], g["cin"], g["dil"]
        ncb, Wp = cin // 32, W + 2 * g["hin"]
        full_order = [(cb, tap) for cb in range(ncb) for tap in range(9)]         # channel-major K order of the one-problem conv
        # the op's output pixels: whole rows [ylo, yhi) of nF frames (a ranged last block / decoder computes a row range; no column range here)
        outs = [_pixels(view.tables[it.tRowC][:it.M], H, W, g["cout"], g["hout"]) for it in items]
        nF = max(int(f.max()) for f, _, _ in outs) + 1
        ylo, yhi = min(int(y.min()) for _, y, _ in outs), max(int(y.max()) for _, y, _ in outs) + 1
        assert sum(it.M for it in items) == nF * (yhi - ylo) * W, (tag, nF, ylo, yhi)
        counts = np.zeros(nF * H * W * 9 * ncb, dtype=np.int64)
        for it in items:
            assert it.K % 32 == 0 and it.splitK == 1 and it.chunksPerSplit == it.K // 32
            nch = it.K // 32
            # ---- the chunks of A: (channel block, tap) from the offset ((ky-1) * dil * Wp + (kx-1) * dil) * cin + c0
            colA = view.tables[it.tColA][:nch]
            c0 = colA % cin
            q = (colA - c0) // cin
            dy = np.rint(q / Wp).astype(np.int64)
            dx = q - dy * Wp
            assert (c0 % 32 == 0).all() and (dy % dil == 0).all() and (dx % dil == 0).all() and (np.abs(dy) <= dil).all() and (np.abs(dx) <= dil).all()
            tapA = (dy // dil + 1) * 3 + dx // dil + 1
            chunksA = list(zip((c0 // 32).tolist(), tapA.tolist()))
            # ---- the chunks of B: chunk (cb * 9 + tap) of the packed weights [cout][9 * cin]
            colB = view.tables[it.tColB][:nch]
            assert (colB % 32 == 0).all()
            chunksB = list(zip((colB // 32 // 9).tolist(), (colB // 32 % 9).tolist()))
            assert chunksA == chunksB, (tag, "A and B name different chunks")
            kept = set(tapA.tolist())
            assert chunksA == [c for c in full_order if c[1] in kept], (tag, "chunk order is not the full problem's, restricted")
            assert len(view.tables[it.tRowB]) >= it.N and (np.diff(view.tables[it.tRowB][:it.N]) == 9 * cin).all()   # rows of the unrepacked weights
            # ---- rows: the input pixel under the centre tap and the output pixel are the same (y, x)
            fa, ya, xa = _pixels(view.tables[it.tRowA][:it.M], H, W, cin, g["hin"])
            fc, yc, xc = _pixels(view.tables[it.tRowC][:it.M], H, W, g["cout"], g["hout"])
            assert np.array_equal(ya, yc) and np.array_equal(xa, xc) and np.array_equal(fa, fc)     # (idQ in, iota out: the same frames here)
            assert fc.min() >= 0 and fc.max() < nF and yc.min() >= 0 and yc.max() < H and xc.min() >= 0 and xc.max() < W
            if it.bufR >= 0:
                hr = {"attn.out": 2, "ffn.2": 2}[tag]
                fr, yr, xr = _pixels(view.tables[it.tRowR][:it.M], H, W, g["cout"], hr)
                assert np.array_equal(yr, yc) and np.array_equal(xr, xc)
            pix = (fc * H + yc) * W + xc
            ch = tapA * ncb + c0 // 32
            counts += np.bincount((pix[:, None] * (9 * ncb) + ch[None, :]).reshape(-1), minlength=counts.size)
            seen.setdefault(tag, set()).add(len(kept))
        # ---- every (output pixel, tap, channel block) whose source row is inside the map exactly once, nothing else: the items
        # partition the pixels (a gap would leave the centre tap at 0, an overlap at 2), no band keeps a halo row, no interior tap is lost
        ys = np.arange(H)[:, None] + (np.arange(9) // 3 - 1)[None, :] * dil                       # source row of (y, tap)
        want = ((ys >= 0) & (ys < H)).astype(np.int64)                                            # [H][9]
        want[:ylo] = 0
        want[yhi:] = 0
        want = np.broadcast_to(want[None, :, None, :, None], (nF, H, W, 9, ncb)).reshape(-1)
        assert np.array_equal(counts, want), tag
        assert [it.M * it.K for it in items] == sorted((it.M * it.K for it in items), reverse=True), (tag, "largest problem first")
    return seen


def structure(what):
    """--structure auto | det: the L = 7 plan (two windows, full rows); ranged: one-window sttn-auto plans with a decoder row range"""
    import vsr_amd  # noqa: F401
    from vsr_amd import _lib
    from vsr_amd.engine import SttnEngine
    from vsr_amd.synth import make_state_dict
    from _replay import PlanView

    assert _lib.lib.vsr_switch_state(b"VSR_SKIP_PAD_TAPS") == 1
    variant = "det" if what == "det" else "auto"
    fh, fw = (60, 108) if variant == "det" else (30, 160)
    eng = SttnEngine(make_state_dict(1 if variant == "det" else 0, variant), variant, device=None)
    if what == "ranged":
        out = {}
        for rows in ((50, 70), (84, 120), (0, 20)):
            view = PlanView(_lib, eng, 2, rows=rows)
            check_structure(view, fh, fw)
            last = {}
            for info, items in view.ops:
                if info.kind == 1 and info.tag.decode() in CONVS:
                    last[info.tag.decode()] = [it.K // CONVS[info.tag.decode()]["cin"] for it in items]     # the last block's overwrite the others'
            assert set(last) == set(CONVS)
            out["%d-%d" % rows] = sorted({tuple(v) for v in last.values()})
            view.close()
    else:
        view = PlanView(_lib, eng, 7)
        seen = check_structure(view, fh, fw)
        out = {"seen": {k: sorted(v) for k, v in seen.items()},
               "taps": [[it.K // CONVS[info.tag.decode()]["cin"] for it in items] for info, items in view.ops if info.kind == 1 and info.tag.decode() in CONVS],
               "flops": view.flops, "executed": float(_lib.lib.vsr_plan_flops_executed(view.p))}
        view.close()
    eng.close()
    print(json.dumps(out))


def gemm_chunk_order(it, bmode, bufs, tables, tile_m=128):
    """tests/_replay.py gemm_reference for the NK problems on the packed weights (convs, q/k/v), with the contraction done as the kernels
    do it: acc += A[:, chunk] . B[chunk, :] for the chunks in table order.  A chunk of zeros adds +0; a fixed block of rows per call keeps
    the shape of every product -- hence its rounding -- independent of the problem's M and K."""
    import torch
    import _replay

    if bmode != 0 or it.bufB != _replay.BUF_WEIGHTS or it.splitK != 1 or it.act & 0xc00 or it.K % 32:
        return _replay.GEMM_REFERENCE(it, bmode, bufs, tables, tile_m)
    M, N, K = it.M, it.N, it.K
    nch = K // 32
    Am = torch.from_numpy(_replay._gather(bufs[it.bufA], it.offA, tables[it.tRowA][:M], tables[it.tColA], K))
    Bm = torch.from_numpy(_replay._gather(bufs[it.bufB], it.offB, tables[it.tRowB][:N], tables[it.tColB], K))
    b3 = Bm.view(N, nch, 32).permute(1, 2, 0).contiguous()                 # [chunk][32][N]
    acc = torch.empty(M, N)
    for r0 in range(0, M, BLOCK):
        rows = min(BLOCK, M - r0)
        a3 = torch.zeros(nch, BLOCK, 32)
        a3[:, :rows] = Am[r0:r0 + rows].view(rows, nch, 32).permute(1, 0, 2)
        c = torch.zeros(BLOCK, N)
        for kc in range(nch):
            c = c + a3[kc] @ b3[kc]
        acc[r0:r0 + rows] = c[:rows]
    acc = acc * it.alpha
    if it.offBias >= 0:
        acc = acc + torch.from_numpy(bufs[_replay.BUF_WEIGHTS][it.offBias:it.offBias + N])[None, :]
    if it.act & 0xff == 1:
        acc = torch.nn.functional.leaky_relu(acc, 0.2)
    else:
        assert it.act & 0xff == 0, it.act
    tColC = tables[it.tColC]
    if it.bufR >= 0:
        assert not it.act & 0x200
        acc = acc + torch.from_numpy(_replay._gather(bufs[it.bufR], it.offR, tables[it.tRowR][:M], tColC, N))
    _replay._scatter(bufs[it.bufC], it.offC, tables[it.tRowC][:M], tColC, N, acc.numpy())


def main():
    import vsr_amd  # noqa: F401
    from vsr_amd import _lib
    from vsr_amd.engine import SttnEngine
    from vsr_amd.synth import make_state_dict
    from oracle.sttn_auto import STTNInpaintOracle, calculate_psnr
    import _replay
    from _replay import PlanView, replay

    _replay.GEMM_REFERENCE = _replay.gemm_reference
    _replay.gemm_reference = gemm_chunk_order            # (replay() looks the name up at every call)
    sd = make_state_dict(0, "auto")
    eng = SttnEngine(sd, "auto", device=None)            # stride 5, references every 10: windows of 7 / 11 / 8 frames
    frames = np.random.default_rng(31).integers(0, 256, size=(L, 120, 640, 3), dtype=np.uint8)
    ref = STTNInpaintOracle(sd, "auto").inpaint(list(frames))
    refa = np.stack([r.astype(np.float32) for r in ref])
    out = {"switch": int(_lib.lib.vsr_switch_state(b"VSR_SKIP_PAD_TAPS"))}
    for name, rows in (("full", None), ("bottom", ROWS)):
        view = PlanView(_lib, eng, L, rows=rows)
        comp, counts, _ = replay(view, eng.packed_weights(), frames)
        lo, hi = (0, 120) if rows is None else rows
        d = np.abs(comp[:, lo:hi] - refa[:, lo:hi])
        # same fp32 arithmetic up to summation order: only truncation-boundary flips (+-1 before averaging)
        assert d.max() <= 1.0, (name, d.max())
        assert (d > 0).mean() < 2e-3, (name, (d > 0).mean())
        assert calculate_psnr(comp[:, lo:hi], refa[:, lo:hi]) > 70.0, name
        for i, r in enumerate(ref):
            assert (r.dtype == np.uint8) == (counts[i] == 1)
        convs = (b"attn.out", b"ffn.1", b"ffn.2", b"dec.1", b"dec.2", b"dec.3", b"enc.2", b"enc.4")
        nitems = sorted({(info.tag.decode(), info.nitems) for info, _ in view.ops if info.kind == 1 and info.tag in convs})
        out[name] = {"sha": hashlib.sha256(np.ascontiguousarray(comp).tobytes()).hexdigest(), "counts": counts.tolist(),
                     "flops": view.flops, "executed": float(_lib.lib.vsr_plan_flops_executed(view.p)), "items": nitems,
                     "max_abs": float(d.max()), "flips": float((d > 0).mean())}
        view.close()
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    if "--structure" in sys.argv:
        structure(sys.argv[sys.argv.index("--structure") + 1])
    else:
        main()
