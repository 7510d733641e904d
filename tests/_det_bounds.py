"""Rounding-error bounds of the detector kernels' arithmetic, shared by tests/test_gpu_det_kernels.py (each launcher alone) and
tests/test_gpu_det_plan_steps.py (a compiled plan, launch by launch).  Nothing here is fitted: every bound is derived from the
operations the kernels perform (csrc/det_kernels.hip is compiled with fp contract off: a multiply and an add are two roundings)."""
import numpy as np

U32 = 2.0 ** -24        # fp32 unit roundoff
SENT = -7.0             # sentinel of every output buffer


def hswish(v):
    return v * np.clip(v + 3.0, 0.0, 6.0) / 6.0


def f32_exact(a):
    """True where the float64 value is a float32 number"""
    with np.errstate(over="ignore"):
        return a.astype(np.float32).astype(np.float64) == a


def hswish_exact_input(v32):
    """hardswish of float32 inputs that reach the activation exactly (unary kind 1, an epilogue without affine): reference and bound.
    The kernel evaluates t = clip(v + 3, 0, 6), m = v * t, r = m / 6 with one rounding each.  A rounding whose exact result is a float32
    number is no rounding: e counts, per element, the operations from the first inexact one on (v + 3 and v * t are exact in float64;
    the quotient is compared with its float32 rounding), and the result is within e * 2^-24 * |hardswish(v)| (each rounding is a
    relative 2^-24 of a factor of the result) -- bit-equal where e = 0, e.g. v >= 3 with 6 v a float32 number, where the result is v."""
    v = v32.astype(np.float64)
    s = v + 3.0
    e1 = ~f32_exact(s)
    t = np.clip(s, 0.0, 6.0)
    e1 &= (t == s)                                    # a clipped value is the exact constant
    m = v * t
    e2 = e1 | ~f32_exact(m)
    q = m / 6.0
    e3 = e2 | ~f32_exact(q)
    e = e1.astype(np.float64) + e2 + e3
    return q, e * U32 * np.abs(q) * (1 + 4 * U32)


def act_ref_bound(pre, pre_err, S, act):
    """activation after an inexact pre-activation: pre = float64 value, pre_err its bound, S >= |pre|.  relu has slope 1 and no
    rounding; hardswish has slope at most 1.5 and three roundings (add, multiply, divide), each a relative 2^-24 of a quantity
    bounded by the |v| the kernel holds, |v| <= S + pre_err"""
    if act == 0:
        return pre, pre_err
    if act == 1:
        return np.maximum(pre, 0.0), pre_err
    assert act == 2
    return hswish(pre), 1.5 * pre_err + 3 * U32 * (S + pre_err)


def sigmoid_ref_bar(v32):
    """sigmoid on float32 inputs: float64 reference and THE BAR, 4 x the worst error of the float32 numpy statement 1/(1+exp(-v)) of the
    same inputs (expf's error is the runtime's, not derivable from the source; 4 covers one more ulp in expf and the divide), with a
    floor of 2 * 2^-24.  The reference calibrates the bar, never the kernel."""
    v32 = np.asarray(v32, np.float32)
    with np.errstate(over="ignore", under="ignore"):
        ref = 1.0 / (1.0 + np.exp(-v32.astype(np.float64)))
        np32 = np.float32(1.0) / (np.float32(1.0) + np.exp(-v32))
    cal = float(np.abs(np32.astype(np.float64) - ref).max())
    bar = max(4.0 * cal, 2.0 * U32)
    print(f"sigmoid: float32 numpy statement max err {cal:.3e} -> bar {bar:.3e}")
    return ref, bar
