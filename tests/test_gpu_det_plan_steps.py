"""A compiled detector plan on the MI355X, launch by launch, against tests/_det_replay.py in float64.

tests/_det_replay.py is the project's statement of what every launcher of a plan does; tests/test_ocr_det_plan.py holds it to the
program interpreter on the CPU, tests/test_gpu_ocr_det.py holds the GPU's final map to the interpreter.  Here the GPU is held to the
replay step by step: after every launch the buffers it writes are downloaded and compared with the float64 value of that ONE step on
the same float32 inputs under the step's rounding bound (tests/_det_bounds.py: (K + e) * 2^-24 * S, bit-equal for data movement), the
cells no step has written yet must still hold what the buffer was created with (a sentinel, or the zeros of a halo), and the GPU's
values replace the replay's before the next step, so nothing drifts and a failure names the launch: index, kind and parameters."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle.ppocr_det import synthetic_weights
from vsr_amd.backend.tools.paddle_graph import load_graph

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _det_replay  # noqa: E402
from _det_bounds import SENT, U32, act_ref_bound, hswish_exact_input, sigmoid_ref_bar  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SHAPE = (2, 3, 32, 64)
BIT_EQUAL = ("to_view", "from_view", "nearest_view", "im2col_view", "maxpool", "nearest_nchw", "copy", "binary")


class _AbsConsts:
    """the plan's constants by absolute value in float64 (offset tables stay what they are)"""

    def __init__(self, consts):
        self.c = consts

    def __getitem__(self, k):
        a = self.c[k]
        return a if np.issubdtype(a.dtype, np.integer) else np.abs(a.astype(np.float64))


def _buffers_of(plan, kind, p):
    names = [v for v in p.values() if isinstance(v, str) and v in plan.buffers]
    if kind == "binary" and p["b"][0] != "const":
        names.append(p["b"][1])
    return sorted(set(names))


def step_reference(plan, kind, p, bufs):
    """(buffer, cells, float64 reference, per-cell bound or None for bit-equal, float32 replay value) of one step on the CURRENT content
    of bufs, which the float32 replay of the step then updates"""
    names = _buffers_of(plan, kind, p)
    b64 = {n: bufs[n].astype(np.float64) for n in names}
    if kind in BIT_EQUAL or (kind == "unary" and p["kind"] == 0):
        # data movement, a selection, or ONE correctly rounded fp32 operation (binary): the float32 replay is the answer bit for bit
        (name, idx), = _det_replay.run_step(kind, p, bufs, plan.consts)
        return name, idx, None, None, bufs[name][idx].copy()
    if kind == "unary" and p["kind"] in (1, 3):
        v = bufs[p["x"]][:p["total"]].copy()
        (name, idx), = _det_replay.run_step(kind, p, bufs, plan.consts)
        ref, bound = hswish_exact_input(v) if p["kind"] == 1 else sigmoid_ref_bar(v)
        return name, idx, ref, np.broadcast_to(bound, ref.shape), bufs[name][idx].copy()
    babs = {n: np.abs(b64[n]) for n in names}
    q = dict(p)
    act = 0
    if kind == "gemm":
        act = 1 if p["act"] == 2 else 0                # GGProblem's act 2 is relu
    elif "act" in p:
        act = p["act"]
    if "act" in q:
        q["act"] = 0
    qa = dict(q)
    if kind == "unary":                                # kinds 2 and 4: v * p0 + p1 (and a clip of slope 1)
        qa.update(kind=4, p0=abs(float(np.float32(p["p0"]))), p1=abs(float(np.float32(p["p1"]))))
        q["kind"] = 4
    (name, idx), = _det_replay.run_step(kind, q, b64, plan.consts, np.float64)
    _det_replay.run_step(kind, qa, babs, _AbsConsts(plan.consts), np.float64)
    pre, S = b64[name][idx], babs[name][idx]
    # roundings per output, K products summed in some order + e epilogue operations -> (K + e) * u * S (tests/_det_bounds.py)
    if kind == "gemm":
        ke = p["K"] + 2                                # K-term dot product, bias add, residual add
    elif kind == "dwconv_view":
        ke = p["kh"] * p["kw"] + (2 if p["scale"] is not None else 0)
    elif kind == "dots_view":
        ke = p["C"] + 1
    elif kind == "conv_nchw":
        ke = (1 if p["dw"] else p["cin"]) * p["kh"] * p["kw"]
    elif kind == "deconv_nchw":
        ke = 1 if p["dw"] else p["cin"]
    elif kind in ("affine", "unary"):
        ke = 2                                         # one multiply, one add
    elif kind == "gap":
        ke = p["HW"]                                   # HW - 1 adds and the divide
    else:
        raise NotImplementedError(kind)
    pre_err = ke * U32 * S
    if kind == "gemm" and p["R"] is not None and act:
        # the GEMM's epilogue is relu(sum + bias) + residual: the relu sits BEFORE the residual add.  The same step without the residual
        # gives the relu's argument; the residual is the difference of the two float64 results (exact to 1e-16 of S: the slack below)
        b0 = {n: bufs[n].astype(np.float64) for n in names}
        _det_replay.run_step(kind, dict(q, R=None), b0, plan.consts, np.float64)
        inner = b0[name][idx]
        pre = np.maximum(inner, 0.0) + (pre - inner)
        pre_err, act = pre_err + 1e-12 * S, 0
    if kind == "unary" and p["kind"] == 2:
        ref, bound = np.clip(pre, 0.0, 1.0), pre_err
    elif act == 3:                                     # sigmoid: slope <= 1/4 on the pre-activation's error + the calibrated bar of its evaluation
        _, bar = sigmoid_ref_bar(pre.astype(np.float32))
        ref, bound = 1.0 / (1.0 + np.exp(-pre)), 0.25 * pre_err + bar
    else:
        ref, bound = act_ref_bound(pre, pre_err, S, act)
    (name32, idx32), = _det_replay.run_step(kind, p, bufs, plan.consts)
    assert name32 == name and np.array_equal(idx32, idx)
    return name, idx, ref, bound, bufs[name][idx].copy()


def walk(plan, launches, x, issue, fetch):
    """drive the replay and the device through the plan; issue(t) runs tape entry t to completion, fetch(name) downloads a buffer.
    Returns a per-kind summary {kind: [steps, worst err / bound, worst err]}."""
    bufs = {k: (np.zeros(sz, np.float32) if zero else np.full(sz, np.nan, np.float32)) for k, (sz, zero) in plan.buffers.items()}
    fill = {k: np.float32(0.0 if zero else SENT) for k, (sz, zero) in plan.buffers.items()}
    written = {k: np.zeros(sz, bool) for k, (sz, zero) in plan.buffers.items()}
    xin = np.asarray(x, np.float32).reshape(-1)
    bufs[plan.input][:xin.size] = xin
    written[plan.input][:xin.size] = True
    summary, nstep = {}, 0

    def untouched(name, g, where):
        stray = np.flatnonzero(~written[name] & (g.view(np.uint32) != fill[name].view(np.uint32)))
        assert stray.size == 0, (f"{where}: {stray.size} cells of {name} that no step has written no longer hold {fill[name]!r}, first at {stray[0]}: "
                                 f"{g[stray[0]]!r}")
        if fill[name] != 0:
            assert np.array_equal(np.isnan(bufs[name]), ~written[name]), f"{where}: the replay's own store set of {name} is inconsistent"

    for t, (kind, pp) in enumerate(launches):
        members = pp if kind == "gemm" else [pp]
        refs = []
        for p in members:
            assert plan.steps[nstep][0] == kind and plan.steps[nstep][1] is p, f"tape entry {t} is not plan step {nstep}"
            refs.append((nstep, p) + step_reference(plan, kind, p, bufs))
            nstep += 1
        issue(t)
        for i, p, name, idx, ref, bound, rep32 in refs:
            where = f"step {i} (tape entry {t}) {kind} {({k: v for k, v in p.items() if k != 'tables'})}"
            g = fetch(name)
            got = g[idx]
            if ref is None:
                bad = np.flatnonzero(got.view(np.uint32) != rep32.view(np.uint32))
                assert bad.size == 0, f"{where}: {bad.size} of {idx.size} cells differ from the replay (bit-equal required), first at {name}[{idx[bad[0]]}]: " \
                                      f"got {got[bad[0]]!r} want {rep32[bad[0]]!r}"
                err, ratio = 0.0, 0.0
            else:
                assert np.isfinite(got).all(), f"{where}: non-finite output"
                e = np.abs(got.astype(np.float64) - ref)
                k = int(np.argmax(e - bound))
                assert e[k] <= bound[k], f"{where}: {name}[{idx[k]}]: got {got[k]!r} ref {ref[k]!r} err {e[k]:.3e} > bound {bound[k]:.3e}"
                err = float(e.max())
                ratio = float((e / np.maximum(bound, 1e-300)).max()) if err > 0 else 0.0
            written[name][idx] = True
            untouched(name, g, where)
            bufs[name][idx] = got                      # the next step starts from the device's values
            s = summary.setdefault(kind, [0, 0.0, 0.0])
            s[0], s[1], s[2] = s[0] + 1, max(s[1], ratio), max(s[2], err)
    assert nstep == len(plan.steps), f"the walk covered {nstep} of {len(plan.steps)} steps"
    for name in plan.buffers:                          # one more sweep: a late stray store into a buffer that was checked early
        untouched(name, fetch(name), "after the last step")
    return summary


@pytest.mark.parametrize("fixture", ["ppocr_det_graph.json", "ppocr_det_fast_graph.json"])
def test_plan_steps_match_replay(built_lib, gpu_device, fixture):
    from vsr_amd.backend.tools import ocr_det

    g = load_graph(os.path.join(GOLD, fixture))
    r = ocr_det.PaddleGraphRunner(g, synthetic_weights(g), device=0)
    r.nhwc = "1"
    st = r.plan_for(SHAPE)
    assert st is not None
    plan, tape, launches = st["plan"], st["tape"], st["launches"]
    assert len(tape) == len(launches)
    for name, (sz, zero) in plan.buffers.items():
        if not zero:
            st["bufs"][name].fill_(SENT)
    x = np.random.default_rng(7).standard_normal(SHAPE).astype(np.float32)
    xd = torch.from_numpy(x).to(gpu_device)
    st["xin"].copy_(xd.reshape(-1))
    r._sa.value = torch.cuda.current_stream().cuda_stream
    issued = []

    def issue(t):
        fn, args = tape[t]
        rc = fn(*args)
        torch.cuda.synchronize()
        assert rc == 0, f"tape entry {t} returned {rc}"
        issued.append(t)

    def fetch(name):
        return st["bufs"][name][:plan.buffers[name][0]].cpu().numpy()

    summary = walk(plan, launches, x, issue, fetch)
    assert issued == list(range(len(tape))), "the walk did not cover every tape entry"
    for kind, (n, ratio, err) in sorted(summary.items()):
        print(f"{fixture} {kind}: {n} steps, worst err {err:.3e}, worst err / bound {ratio:.3f}" + (" (bit-equal)" if kind in BIT_EQUAL else ""))
    walked = st["out"].clone()
    again = r.run_planned(xd, st).clone()
    torch.cuda.synchronize()
    assert torch.equal(walked, again), "the launch-by-launch walk and run_planned disagree"
    r.close()
