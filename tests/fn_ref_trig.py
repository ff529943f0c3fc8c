"""sin, cos and log of the flow graphs restated in numpy, operation for operation with the constants zignal_amd/csrc/fz_codegen.cpp
prints (include/flowz_hip.h, FZ_OP_SIN ..).  numpy float32 / float64 arrays round every operation as the kernels do (no FMA, no libm),
so the restatement gives the kernels' bits for every non-NaN result.

Importing this module registers the three functions in fn_ref.FN and fn_ref._UN: fn_ref.run_ir then evaluates the IR kinds
"sin", "cos" and "log" unchanged.
"""
import numpy as np

import fn_ref as R

F32, F64 = np.float32, np.float64
h = float.fromhex

SINCOS_C = dict(
    two_over_pi=h("0x1.45f306dc9c883p-1"), h1=h("0x1.921fb54400000p+0"), h2=h("0x1.0b4611a600000p-34"), h3=h("0x1.3198a2e037073p-69"),
    ps=[h("0x1.952c77030ad4ap-49"), -h("0x1.ae7f3e733b81fp-41"), h("0x1.6124613a86d09p-33"), -h("0x1.ae64567f544e4p-26"),
        h("0x1.71de3a556c734p-19"), -h("0x1.a01a01a01a01ap-13"), h("0x1.1111111111111p-7"), -h("0x1.5555555555555p-3")],
    pc=[-h("0x1.6827863b97d97p-53"), h("0x1.ae7f3e733b81fp-45"), -h("0x1.93974a8c07c9dp-37"), h("0x1.1eed8eff8d898p-29"),
        -h("0x1.27e4fb7789f5cp-22"), h("0x1.a01a01a01a01ap-16"), -h("0x1.6c16c16c16c17p-10"), h("0x1.5555555555555p-5"),
        -h("0x1.0000000000000p-1")])
LOG_C = {
    F32: dict(minn=0x00800000, scale=h("0x1p25"), sbits=25, off=0x004afb0d, mant=0x007fffff, rh=0x3f3504f3,
              lg=[h("0x1.555556p-1"), h("0x1.9999ecp-2"), h("0x1.245c0ap-2"), h("0x1.dddadep-3")]),
    F64: dict(minn=0x0010000000000000, scale=h("0x1p54"), sbits=54, off=0x00095f619980c433, mant=0x000fffffffffffff, rh=0x3fe6a09e667f3bcd,
              lg=[h("0x1.5555555555558p-1"), h("0x1.9999999995204p-2"), h("0x1.2492492e09d1ap-2"), h("0x1.c71c62c63e016p-3"),
                  h("0x1.7462bd8e53c17p-3"), h("0x1.39fd39474ad34p-3"), h("0x1.2b6686d1072f3p-3")]),
}


def _sincos_core(a):
    """fz_sincos_core: s = sin r, c = cos r in double, the quadrant k & 3, and ok = |a| < 2^20 (the core runs on 0 elsewhere)"""
    a = np.asarray(a, F32)
    c = SINCOS_C
    ok = (a.view(np.int32) & np.int32(0x7fffffff)) < np.int32(0x49800000)
    x = np.where(ok, a, F32(0)).astype(F64)
    t = x * F64(c["two_over_pi"])
    th = t + np.where(t < F64(0), F64(-0.5), F64(0.5))
    k = th.astype(np.int32)                                  # truncates
    kd = k.astype(F64)
    r = x - kd * F64(c["h1"])
    r = r - kd * F64(c["h2"])
    r = r - kd * F64(c["h3"])
    z = r * r
    ps = np.full_like(z, F64(c["ps"][0]))
    for v in c["ps"][1:]:
        ps = F64(v) + z * ps
    s = r + r * (z * ps)
    pc = np.full_like(z, F64(c["pc"][0]))
    for v in c["pc"][1:]:
        pc = F64(v) + z * pc
    co = F64(1) + z * pc
    return s, co, k.astype(np.int64) & np.int64(3), ok


def sin(a):
    """fz_sin: quadrant 0..3 -> s, c, -s, -c; rounded to float once; |a| >= 2^20, inf, NaN -> NaN"""
    with np.errstate(all="ignore"):
        s, c, q, ok = _sincos_core(a)
        m = np.where((q & 1) != 0, c, s)
        y = np.where((q & 2) != 0, -m, m).astype(F32)
        y = np.where(np.asarray(a, F32) == F32(0), np.asarray(a, F32), y)   # sin(+-0) = +-0
        return np.where(ok, y, F32(np.nan)).astype(F32)


def cos(a):
    """fz_cos: quadrant 0..3 -> c, -s, -c, s"""
    with np.errstate(all="ignore"):
        s, c, q, ok = _sincos_core(a)
        m = np.where((q & 1) != 0, s, c)
        y = np.where(((q + 1) & 2) != 0, -m, m)
        return np.where(ok, y.astype(F32), F32(np.nan)).astype(F32)


def log(a):
    """fz_log, float32 or float64: a = m 2^e with m in [sqrt(1/2), sqrt 2) through the exponent bits, f = m - 1, s = f / (2 + f),
    log = e ln2_hi + (f - (h - (s (h + R) + e ln2_lo)))"""
    a = np.asarray(a)
    T = a.dtype.type
    I, sh, bias = R._T[T]
    c, ec = LOG_C[T], R.EXP_C[T]
    with np.errstate(all="ignore"):
        sub = a.view(I) < I(c["minn"])
        x = np.where(sub, a * T(c["scale"]), a).astype(T)
        ix = x.view(I) + I(c["off"])
        e = ((ix >> I(sh)) - I(bias)) - np.where(sub, I(c["sbits"]), I(0))
        m = ((ix & I(c["mant"])) + I(c["rh"])).astype(I).view(T)
        f = m - T(1)
        s = f / (T(2) + f)
        z = s * s
        w = z * z
        lg = c["lg"]
        ts = []
        for par in (0, 1):                                   # t2: L1, L3, ..; t1: L2, L4, ..
            cs = lg[par::2]
            t = np.full_like(w, T(cs[-1]))
            for v in cs[-2::-1]:
                t = T(v) + w * t
            ts.append(t)
        Rp = z * ts[0] + w * ts[1]
        hh = (T(0.5) * f) * f
        ef = e.astype(T)
        u = s * (hh + Rp) + ef * T(ec["ln2lo"])
        y = ef * T(ec["ln2hi"]) + (f - (hh - u))
        y = np.where(a == T(np.inf), a, y)
        y = np.where(a < T(0), T(np.nan), y)
        y = np.where(a == T(0), T(-np.inf), y)
        return np.where(a != a, a, y).astype(T)


R.FN.update({"sin": sin, "cos": cos, "log": log})
R._UN.update({"sin": sin, "cos": cos, "log": log})
