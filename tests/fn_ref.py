"""The graph functions (abs, sqrt, exp, tanh, min, max) restated in numpy, and a per-sample evaluator of Program.ir() that knows them.

exp and tanh follow the kernels' algorithm operation for operation (include/flowz_hip.h, "Graph functions"): IEEE basic operations in
the operand's type, no FMA, no libm.  numpy float32 / float64 arrays round every operation the same way, so the restatement gives
the kernels' bits for every non-NaN result.  The constants below are the ones zignal_amd/csrc/fz_codegen.cpp prints.

The evaluator follows tests/ir_interp.py (which it does not change): one delay line per delayed wire, row (row0 + j) of a float line
holds the wire's value j + 1 samples ago; a double line (typed programs) takes two float rows per slot, slot j being ONE row of
n_streams doubles over float rows (row0 + 2j, row0 + 2j + 1).  Double input wires are (low word, high word) frame slots, double
outputs of typed programs leave as such slot pairs; sample-rate modulators are rows of a [n_mod, T] array.  The hand-written recurrences at the
end restate the workloads of zignal_amd/workloads.py from their equations, not from the IR, so they check the lowering too.
"""
import numpy as np

from zignal_amd import flowz as F

F32, F64 = np.float32, np.float64
h = float.fromhex

# float type -> (the signed integer type of its bits, position of the exponent field, exponent bias)
_T = {F32: (np.int32, 23, 127), F64: (np.int64, 52, 1023)}

EXP_C = {
    F32: dict(log2e=h("0x1.715476p+0"), ln2hi=h("0x1.62ep-1"), ln2lo=h("0x1.0bfbe8p-15"), magic=h("0x1.8p+23"),
              lo=-104.0, hi=89.0, xmax=h("0x1.62e42ep+6"),
              q=[h("0x1.a127fcp-13"), h("0x1.6d469p-10"), h("0x1.1110ep-7"), h("0x1.5554e6p-5"), h("0x1.555556p-3"), h("0x1p-1")]),
    F64: dict(log2e=h("0x1.71547652b82fep+0"), ln2hi=h("0x1.62e42fee00000p-1"), ln2lo=h("0x1.a39ef35793c76p-33"), magic=h("0x1.8p+52"),
              lo=-746.0, hi=710.0, xmax=h("0x1.62e42fefa39efp+9"),
              q=[h("0x1.1f74882ae4b27p-29"), h("0x1.af509232e2477p-26"), h("0x1.27e4daa87b888p-22"), h("0x1.71de00e89dd34p-19"),
                 h("0x1.a01a01a714245p-16"), h("0x1.a01a01ac50533p-13"), h("0x1.6c16c16c16266p-10"), h("0x1.111111111001cp-7"),
                 h("0x1.5555555555556p-5"), h("0x1.5555555555557p-3"), h("0x1p-1")]),
}
TANH_C = {
    F32: dict(sw=h("0x1.19999ap-1"), sat=10.0,
              p=[h("0x1.4b0ed2p-9"), -h("0x1.176084p-7"), h("0x1.6578cap-6"), -h("0x1.ba1428p-5"), h("0x1.111104p-3"), -h("0x1.555556p-2")]),
    F64: dict(sw=h("0x1.19999ap-1"), sat=20.0,
              p=[h("0x1.081656de10f02p-17"), -h("0x1.1ad1adfc0e63cp-15"), h("0x1.8c8f32860a20fp-14"), -h("0x1.f41c32178e2b0p-13"),
                 h("0x1.3547b24884a3fp-11"), -h("0x1.7da25c9e6e474p-10"), h("0x1.d6d3c5f32768dp-9"), -h("0x1.226e353986e33p-7"),
                 h("0x1.664f48822db68p-6"), -h("0x1.ba1ba1ba1a711p-5"), h("0x1.1111111111109p-3"), -h("0x1.5555555555555p-2")]),
}


def _pow2(k, T):
    I, sh, bias = _T[T]
    return ((k + I(bias)).astype(I) << I(sh)).view(T)


def exp(x):
    """fz_exp: Cody-Waite reduction by ln 2, a polynomial by Horner's rule, scaling by 2^k in two exact-then-rounding steps."""
    x = np.asarray(x)
    T = x.dtype.type
    I = _T[T][0]
    c = EXP_C[T]
    with np.errstate(all="ignore"):
        xc = np.where(x < T(c["lo"]), T(c["lo"]), x)
        xc = np.where(xc > T(c["hi"]), T(c["hi"]), xc)
        xc = np.where(xc == xc, xc, T(0))
        tm = xc * T(c["log2e"]) + T(c["magic"])
        kf = tm - T(c["magic"])
        r = (xc - kf * T(c["ln2hi"])) - kf * T(c["ln2lo"])
        q = np.full_like(r, T(c["q"][0]))
        for a in c["q"][1:]:
            q = T(a) + r * q
        p = T(1) + (r + (r * r) * q)
        k = tm.view(I) - np.asarray(T(c["magic"])).view(I)
        k1 = k >> I(1)
        k2 = k - k1
        y = (p * _pow2(k1, T)) * _pow2(k2, T)
        y = np.where(x > T(c["xmax"]), T(np.inf), y)
        return np.where(x != x, x, y).astype(T)


def tanh(x):
    """fz_tanh: odd, |x| below the switch point: |x| + |x| * (z * P(z)), z = x^2; above: 1 - 2 / (exp(2|x|) + 1); past saturation 1;
    the sign bit of x put back last."""
    x = np.asarray(x)
    T = x.dtype.type
    I = _T[T][0]
    c = TANH_C[T]
    sign = I(np.iinfo(I).min)
    with np.errstate(all="ignore"):
        ax = (x.view(I) & ~sign).view(T)
        z = ax * ax
        p = np.full_like(z, T(c["p"][0]))
        for a in c["p"][1:]:
            p = T(a) + z * p
        ys = ax + ax * (z * p)
        ac = np.where(ax > T(c["sat"]), T(c["sat"]), ax)
        yb = T(1) - T(2) / (exp(ac + ac) + T(1))
        y = np.where(ax < T(c["sw"]), ys, yb)
        y = np.where(ax > T(c["sat"]), T(1), y)
        y = (y.view(I) | (x.view(I) & sign)).view(T)
        return np.where(x != x, x, y).astype(T)


def fabs(x):
    x = np.asarray(x)
    I = _T[x.dtype.type][0]
    return (x.view(I) & I(np.iinfo(I).max)).view(x.dtype)


def sqrt(x):
    with np.errstate(all="ignore"):
        return np.sqrt(np.asarray(x))


def fmin(a, b):
    """std::min: (b < a) ? b : a"""
    a, b = np.broadcast_arrays(np.asarray(a), np.asarray(b))
    return np.where(b < a, b, a)


def fmax(a, b):
    """std::max: (a < b) ? b : a"""
    a, b = np.broadcast_arrays(np.asarray(a), np.asarray(b))
    return np.where(a < b, b, a)


FN = {"abs": fabs, "sqrt": sqrt, "exp": exp, "tanh": tanh, "min": fmin, "max": fmax}


# ---- the IR evaluator ---------------------------------------------------------------------------------------------------------
_BIN = {"add": np.add, "sub": np.subtract, "mul": np.multiply, "div": np.divide, "min": fmin, "max": fmax}
_UN = {"neg": np.negative, "abs": fabs, "sqrt": sqrt, "exp": exp, "tanh": tanh}
_CMP = {"lt": np.less, "le": np.less_equal, "gt": np.greater, "ge": np.greater_equal, "eq": np.equal, "ne": np.not_equal}


def run_ir(prog, x, params=None, state=None, mod=None, out_f64=False):
    """Evaluate a program on frames x [T, n_streams, n_in slots] from `state` (None: zeros, else [n_state, n_streams] float32 rows).
    mod: [n_mod, >= T], sample t reads mod[k][t] (as Program.set_modulation rows from the block's first sample).  out_f64: float64
    output frames (FZ_VF_OUT_F64: double results unrounded).  Returns (y [T, n_streams, n_out], the state after the block)."""
    x = np.asarray(x, F32)
    if x.ndim == 2:
        x = x[:, :, None]
    Tn, ns, _ = x.shape
    ir, dts, outs, codes = prog.ir(), prog.ir_dtypes(), prog.outputs(), prog.output_slot_codes()
    row0, r = {}, 0
    for (src, depth), ldt in zip(prog.lines(), prog.line_dtypes()):
        f64 = ldt == "f64"
        assert ldt in ("f32", "f64"), ldt
        row0[src] = (r, depth, f64)
        r += depth * (2 if f64 else 1)
    st = np.zeros((max(r, 1), ns), F32) if state is None else np.array(state, F32, copy=True)
    flat = st.reshape(-1)

    def drow(rr):                                          # the row of ns doubles that starts at float row rr
        return flat[rr * ns:(rr + 2) * ns].view(F64)

    y = np.empty((Tn, ns, len(outs)), F64 if out_f64 else F32)
    with np.errstate(all="ignore"):
        for t in range(Tn):
            v = [None] * len(ir)
            for i, (kind, a, b, val) in enumerate(ir):
                T = F64 if dts[i] == "f64" else F32
                if kind == "input":
                    r_ = np.stack([x[t, :, a], x[t, :, a + 1]], -1).view(F64)[:, 0] if T == F64 else x[t, :, a]
                elif kind == "const": r_ = np.full(ns, T(val), T)
                elif kind == "param": r_ = np.asarray(params[a], F32)
                elif kind == "mod": r_ = np.full(ns, F32(mod[a][t]), F32)
                elif kind == "delay":
                    r0, depth, f64 = row0[a]
                    assert 1 <= b <= depth and f64 == (T == F64)
                    r_ = drow(r0 + 2 * (b - 1)).copy() if f64 else st[r0 + b - 1].copy()
                elif kind in _BIN: r_ = _BIN[kind](v[a].astype(T), v[b].astype(T))
                elif kind in _UN: r_ = _UN[kind](v[a].astype(T))
                elif kind in _CMP:
                    dd = F64 if F64 in (v[a].dtype.type, v[b].dtype.type) else F32
                    r_ = np.where(_CMP[kind](v[a].astype(dd), v[b].astype(dd)), F32(1), F32(0))
                else:
                    raise NotImplementedError(kind)
                v[i] = np.asarray(r_).astype(T)
            for j, o in enumerate(outs):
                if codes[j] in (4, 5):                     # a double wire of a typed program: its low / high word
                    y[t, :, j] = np.ascontiguousarray(v[o], F64)[:, None].view(F32)[:, codes[j] - 4]
                else:
                    y[t, :, j] = v[o].astype(y.dtype)
            for src, (r0, depth, f64) in row0.items():    # pushes last: every read above saw the previous samples
                if f64:
                    for k in range(depth - 1, 0, -1):
                        drow(r0 + 2 * k)[:] = drow(r0 + 2 * (k - 1))
                    drow(r0)[:] = v[src]
                else:
                    st[r0 + 1:r0 + depth] = st[r0:r0 + depth - 1].copy()
                    st[r0] = v[src].astype(F32)
    return y, st


# ---- the workloads from their equations ----------------------------------------------------------------------------------------
def moog_ladder_ref(x, g, k):
    """zignal_amd.workloads.moog_ladder: x [T, ns] float32, g [ns] per-stream cutoff, k the resonance.
        u = tanh(x - k*y4[n-1]);  y1 = y1' + g*(u - tanh(y1'));  y_i = y_i' + g*(tanh(y_{i-1}) - tanh(y_i'))  (i = 2..4)
    where y' is the stage's value one sample ago; the output is y4."""
    x = np.asarray(x, F32)
    g = np.asarray(g, F32)
    k = F32(k)
    ns = x.shape[1]
    y = [np.zeros(ns, F32) for _ in range(4)]
    out = np.empty_like(x)
    with np.errstate(all="ignore"):
        for t in range(x.shape[0]):
            u = tanh(x[t] - k * y[3])
            n1 = y[0] + g * (u - tanh(y[0]))
            n2 = y[1] + g * (tanh(n1) - tanh(y[1]))
            n3 = y[2] + g * (tanh(n2) - tanh(y[2]))
            n4 = y[3] + g * (tanh(n3) - tanh(y[3]))
            y = [n1, n2, n3, n4]
            out[t] = n4
    return out


def soft_clip_cascade_ref(x, coeffs):
    """zignal_amd.workloads.soft_clip_cascade: per stage (b0, b1, b2, a1, a2): w = b0 x + b1 x[-1] + b2 x[-2] (left to right), then
    y = tanh(w + a1 y[-1] + a2 y[-2]) -- written as ((w + a1*y1) + a2*y2)."""
    s = np.asarray(x, F32)
    with np.errstate(all="ignore"):
        for b0, b1, b2, a1, a2 in coeffs:
            b0, b1, b2, a1, a2 = (F32(c) for c in (b0, b1, b2, a1, a2))
            x1 = np.zeros(s.shape[1], F32); x2 = np.zeros_like(x1); y1 = np.zeros_like(x1); y2 = np.zeros_like(x1)
            out = np.empty_like(s)
            for t in range(s.shape[0]):
                w = (b0 * s[t] + b1 * x1) + b2 * x2
                yt = tanh((w + a1 * y1) + a2 * y2)
                x2, x1 = x1, s[t]
                y2, y1 = y1, yt
                out[t] = yt
            s = out
    return s


def envelope_follower_ref(x, attack, release):
    """zignal_amd.workloads.envelope_follower: r = |x|;  e = max(r, e[-1] + release*(r - e[-1]))  with the attack as a one-pole
    toward a rising input:  e = max(e[-1] + attack*(r - e[-1]), e[-1] + release*(r - e[-1]))"""
    x = np.asarray(x, F32)
    a, rl = F32(attack), F32(release)
    e = np.zeros(x.shape[1], F32)
    out = np.empty_like(x)
    with np.errstate(all="ignore"):
        for t in range(x.shape[0]):
            r = fabs(x[t])
            d = r - e
            e = fmax(e + a * d, e + rl * d)
            out[t] = e
    return out
