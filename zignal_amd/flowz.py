"""Python mirror of the Flowz EDSL (reference: flowz/flowz.hpp) over the C ABI of libflowz_hip.

Same surface as the C++ front end in include/flowz/flowz.hpp, spelled with what Python's
grammar allows:

    reference (C++)            here
    _1 .. _6                   _1 .. _6, placeholder(i)            flowz.hpp:1252-1257, :78-82
    _1[_2]                     _1[_2]  (or _1[-2], _1[2])          :84-85
    a , b                      chan(a, b, ...)  or a tuple (a, b)  :90
    a | b                      a | b                               :91
    a |= b                     a >> b  (`|=` is a statement in Python; `>>` is the sequence
                               operator of the reference's first prototype,
                               experimental_steps/wires_mono_only.cpp:37), seq(a, b, ...) for
                               C++'s right-associative chaining
    ~a                         ~a                                  :93
    + - * / unary -            same; Python numbers become float32 literal terminals   :68-72, :769-772
    std::ref(x)                param(k): per-stream, block-constant coefficient k (flowz/README.md:42-61)
    compile(expr)              compile(expr) -> Program            :1233-1249

A Program evaluates blocks on the GPU only (Program.run_block / Bank); there is no CPU path.
"""
from __future__ import annotations

import builtins as _bi   # (the module's own abs / min / max are graph functions)
import ctypes
from typing import Iterable, Optional, Sequence

from . import _capi as C
from ._capi import FlowzError, NoDeviceError, Variant  # noqa: F401  (re-exported)


class Expr:
    """Immutable handle of a Flowz expression tree (value semantics, flowz.hpp:46-61)."""

    __slots__ = ("_h",)

    def __init__(self, handle):
        self._h = C.check_ptr(handle)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and C is not None:
            try:
                C.lib.fz_expr_release(h)
            except Exception:
                pass

    # -- analysis (flowz.hpp:162-246, :443-506) ------------------------------------------
    @property
    def ins(self) -> int:
        return C.check(C.lib.fz_input_arity(self._h))

    @property
    def outs(self) -> int:
        return C.check(C.lib.fz_output_arity(self._h))

    def max_input_delays(self):
        n = C.check(C.lib.fz_max_input_delays(self._h, None, 0))
        buf = (ctypes.c_uint32 * _bi.max(n, 1))()
        C.check(C.lib.fz_max_input_delays(self._h, buf, n))
        return tuple(buf[i] for i in range(n))

    # -- arithmetic ------------------------------------------------------------------------
    def _ar(self, op, other, swap=False):
        o = as_expr(other)
        a, b = (o, self) if swap else (self, o)
        return Expr(C.lib.fz_arith(op, a._h, b._h))

    def __add__(self, o): return self._ar(C.FZ_OP_ADD, o)
    def __radd__(self, o): return self._ar(C.FZ_OP_ADD, o, True)
    def __sub__(self, o): return self._ar(C.FZ_OP_SUB, o)
    def __rsub__(self, o): return self._ar(C.FZ_OP_SUB, o, True)
    def __mul__(self, o): return self._ar(C.FZ_OP_MUL, o)
    def __rmul__(self, o): return self._ar(C.FZ_OP_MUL, o, True)
    def __truediv__(self, o): return self._ar(C.FZ_OP_DIV, o)
    def __rtruediv__(self, o): return self._ar(C.FZ_OP_DIV, o, True)
    def __neg__(self): return Expr(C.lib.fz_arith(C.FZ_OP_NEG, self._h, None))

    # -- comparison and logical operators (proto::_default applies whatever C++ operator a node is, flowz.hpp:769-772): 1.0 / 0.0 -----------
    # (== and != are the methods eq / ne: Python needs __eq__ for its own purposes; `and` / `or` / `not` cannot be overloaded at all)
    def __lt__(self, o): return self._ar(C.FZ_OP_LT, o)
    def __le__(self, o): return self._ar(C.FZ_OP_LE, o)
    def __gt__(self, o): return self._ar(C.FZ_OP_GT, o)
    def __ge__(self, o): return self._ar(C.FZ_OP_GE, o)
    def eq(self, o): return self._ar(C.FZ_OP_EQ, o)
    def ne(self, o): return self._ar(C.FZ_OP_NE, o)
    def logical_and(self, o): return self._ar(C.FZ_OP_AND, o)
    def logical_or(self, o): return self._ar(C.FZ_OP_OR, o)
    def logical_not(self): return Expr(C.lib.fz_arith(C.FZ_OP_NOT, self._h, None))
    def __abs__(self): return Expr(C.lib.fz_arith(C.FZ_OP_ABS, self._h, None))     # std::fabs (graph function)

    def __bool__(self):
        # (`_1 < _2` is an expression, not a Python truth value: `if a < b`, builtin `max(a, b)`, `a and b` would silently take the wrong branch)
        raise TypeError("a Flowz expression has no truth value: comparisons build graph nodes (use .logical_and / .logical_or / .logical_not to combine them)")

    # -- combinators -----------------------------------------------------------------------
    def __or__(self, o): return Expr(C.lib.fz_parallel(self._h, as_expr(o)._h))
    def __ror__(self, o): return Expr(C.lib.fz_parallel(as_expr(o)._h, self._h))
    def __rshift__(self, o): return Expr(C.lib.fz_sequence(self._h, as_expr(o)._h))
    def __rrshift__(self, o): return Expr(C.lib.fz_sequence(as_expr(o)._h, self._h))
    def __invert__(self): return Expr(C.lib.fz_feedback(self._h))


class Placeholder(Expr):
    __slots__ = ("index",)

    def __init__(self, i: int):
        super().__init__(C.lib.fz_placeholder(int(i)))
        self.index = int(i)

    def __getitem__(self, d):
        """_i[_n] (reference syntax), _i[-n] (delay_expression.cpp:99-100 spelling) or _i[n]."""
        n = d.index if isinstance(d, Placeholder) else _bi.abs(int(d))
        return Expr(C.lib.fz_delayed(self.index, n))


def placeholder(i: int) -> Placeholder:
    return Placeholder(i)


_1, _2, _3, _4, _5, _6 = (Placeholder(i) for i in range(1, 7))


def lit(v: float) -> Expr:
    return Expr(C.lib.fz_literal(float(v)))


def lit64(v: float) -> Expr:
    """A C++ `double` literal terminal: the operators above it evaluate in float64 (usual arithmetic
    conversions); delay lines and frames stay float32.  Plain Python numbers are float32 literals."""
    return Expr(C.lib.fz_literal_f64(float(v)))


def litc(re: float, im: float = 0.0) -> Expr:
    """A std::complex<float> terminal (test/tests.cpp:206-207): the wire above it is complex and takes
    two float32 slots (re, im) of the output frame.  Python complex numbers become these."""
    return Expr(C.lib.fz_literal_c32(float(re), float(im)))


def litc64(re: float, im: float = 0.0) -> Expr:
    """A std::complex<double> terminal: as litc with double parts (z / w is libgcc's __divdc3, Smith's method).  In a
    typed program the wire takes four float32 slots: the double of the real part, then that of the imaginary part."""
    return Expr(C.lib.fz_literal_c64(float(re), float(im)))


def uniform(k: int, initial: float = 0.0) -> Expr:
    """Uniform run-time coefficient k (the std::ref(x) terminal): Program.set_uniform(k, v)."""
    return Expr(C.lib.fz_uniform(int(k), float(initial)))


def param(k: int) -> Expr:
    return Expr(C.lib.fz_stream_param(int(k)))


def modulator(k: int) -> Expr:
    """Sample-rate modulator k: the std::ref(x) terminal whose variable changes between calls (flowz/README.md:42-61), for
    block evaluation -- one value per sample, the same for all streams: Program.set_modulation(tensor [n_mod, rows])."""
    return Expr(C.lib.fz_modulator(int(k)))


def as_expr(x) -> Expr:
    if isinstance(x, Expr):
        return x
    if isinstance(x, tuple):
        return chan(*x)
    if isinstance(x, complex):
        return litc(x.real, x.imag)
    if isinstance(x, (int, float)) or hasattr(x, "__float__"):
        return lit(float(x))
    raise TypeError(f"cannot use {type(x).__name__} in a Flowz expression")


def chan(*xs) -> Expr:
    """(a, b, c): C++ comma is left-associative."""
    r = as_expr(xs[0])
    for x in xs[1:]:
        r = Expr(C.lib.fz_channel(r._h, as_expr(x)._h))
    return r


def par(*xs) -> Expr:
    r = as_expr(xs[0])
    for x in xs[1:]:
        r = r | as_expr(x)
    return r


def seq(*xs) -> Expr:
    """a |= b |= c: C++ `|=` is right-associative, a |= (b |= c)."""
    r = as_expr(xs[-1])
    for x in reversed(xs[:-1]):
        r = as_expr(x) >> r
    return r


# ---- graph functions (include/flowz_hip.h, FZ_OP_ABS ..): std::fabs, std::sqrt, std::exp, std::tanh, std::min, std::max, std::sin, std::cos, std::log
def _fn1(op, a) -> Expr:
    a = as_expr(a)                      # (held: a temporary's handle would be released before fz_arith retains it)
    return Expr(C.lib.fz_arith(op, a._h, None))


def _fn2(op, a, b) -> Expr:
    a, b = as_expr(a), as_expr(b)
    return Expr(C.lib.fz_arith(op, a._h, b._h))


def abs(a) -> Expr:  # noqa: A001  (mirrors flowz::abs)
    """std::fabs: the sign bit cleared"""
    return _fn1(C.FZ_OP_ABS, a)


def sqrt(a) -> Expr:
    """std::sqrt, correctly rounded"""
    return _fn1(C.FZ_OP_SQRT, a)


def exp(a) -> Expr:
    """std::exp: the library's algorithm, within 2 ulp"""
    return _fn1(C.FZ_OP_EXP, a)


def tanh(a) -> Expr:
    """std::tanh: the library's algorithm, within 2 ulp, odd, |tanh| <= 1"""
    return _fn1(C.FZ_OP_TANH, a)


def sin(a) -> Expr:
    """std::sin of a float32 wire: correctly rounded but for arguments next to a rounding boundary, odd; |a| >= 2^20 gives NaN"""
    return _fn1(C.FZ_OP_SIN, a)


def cos(a) -> Expr:
    """std::cos of a float32 wire: correctly rounded but for arguments next to a rounding boundary, even; |a| >= 2^20 gives NaN"""
    return _fn1(C.FZ_OP_COS, a)


def log(a) -> Expr:
    """std::log: the library's algorithm, within 2 ulp; log(+-0) = -inf, a negative operand gives NaN"""
    return _fn1(C.FZ_OP_LOG, a)


def min(a, b) -> Expr:  # noqa: A001  (mirrors flowz::min)
    """std::min: (b < a) ? b : a, in the operands' common type; either side may be a scalar (a float literal)"""
    return _fn2(C.FZ_OP_MIN, a, b)


def max(a, b) -> Expr:  # noqa: A001  (mirrors flowz::max)
    """std::max: (a < b) ? b : a, in the operands' common type; either side may be a scalar (a float literal)"""
    return _fn2(C.FZ_OP_MAX, a, b)


_FN1 = {"abs": C.FZ_OP_ABS, "sqrt": C.FZ_OP_SQRT, "exp": C.FZ_OP_EXP, "tanh": C.FZ_OP_TANH,
        "sin": C.FZ_OP_SIN, "cos": C.FZ_OP_COS, "log": C.FZ_OP_LOG}
_FN2 = {"min": C.FZ_OP_MIN, "max": C.FZ_OP_MAX}


_CMP_OPS = {"lt": C.FZ_OP_LT, "le": C.FZ_OP_LE, "gt": C.FZ_OP_GT, "ge": C.FZ_OP_GE, "eq": C.FZ_OP_EQ, "ne": C.FZ_OP_NE, "and": C.FZ_OP_AND, "or": C.FZ_OP_OR}


def from_sexpr(e) -> Expr:
    """Build from the neutral s-expression notation shared with the test-suite."""
    k = e[0]
    if k == "in": return Placeholder(e[1])
    if k == "del": return Placeholder(e[1])[int(e[2])]
    if k == "lit": return lit(e[1])
    if k == "lit64": return lit64(e[1])
    if k == "litc": return litc(e[1], e[2])
    if k == "litc64": return litc64(e[1], e[2])
    if k == "param": return param(e[1])
    if k == "mod": return modulator(e[1])
    if k == "uniform": return uniform(e[1], e[2])
    if k == "neg": return -from_sexpr(e[1])
    if k == "not": return from_sexpr(e[1]).logical_not()
    if k == "fb": return ~from_sexpr(e[1])
    if k in _FN1: return _fn1(_FN1[k], from_sexpr(e[1]))
    a, b = from_sexpr(e[1]), from_sexpr(e[2])
    if k == "add": return a + b
    if k == "sub": return a - b
    if k == "mul": return a * b
    if k == "div": return a / b
    if k in _CMP_OPS: return a._ar(_CMP_OPS[k], b)
    if k in _FN2: return _fn2(_FN2[k], a, b)
    if k == "chan": return chan(a, b)
    if k == "par": return a | b
    if k == "seq": return a >> b
    raise ValueError(f"unknown s-expression node {k!r}")


def make_variant(streams_per_lane=0, unroll=0, block_threads=0, flags=0) -> Variant:
    return Variant(int(streams_per_lane), int(unroll), int(block_threads), int(flags))


def _require(ok, what):
    """Argument check that survives `python -O` (the C ABI takes raw pointers: a wrong shape is an out-of-bounds access)."""
    if not ok:
        raise FlowzError(C.FZ_E_INVALID, str(what))


def _check_dev(t, shape, what, dtype=None):
    """A caller-supplied device buffer handed to the C ABI as a raw pointer: float32 (or `dtype`), CUDA, contiguous and of
    exactly the shape the kernel will address -- anything else would be a silent out-of-bounds device access."""
    import torch

    dtype = dtype or torch.float32
    if not (t.is_cuda and t.dtype == dtype and t.is_contiguous() and tuple(t.shape) == tuple(shape)):
        raise FlowzError(C.FZ_E_INVALID, f"{what}: expected a contiguous CUDA {dtype} tensor of shape {tuple(shape)}, got "
                                         f"{t.dtype} {tuple(t.shape)} on {t.device}" + ("" if t.is_contiguous() else " (not contiguous)"))
    return t


def _check_frames(x, last, what="x"):
    """Input frames handed over as a raw pointer: contiguous float32 CUDA tensor whose last axis is the wire count."""
    import torch

    if not x.is_cuda:
        raise NoDeviceError(C.FZ_E_NO_DEVICE, f"{what}: needs CUDA (ROCm) tensors: zignal_amd has no CPU path")
    if not (x.dtype == torch.float32 and x.is_contiguous() and x.shape[-1] == last):
        raise FlowzError(C.FZ_E_INVALID, f"{what}: expected contiguous float32 frames with {last} wire(s) on the last axis, got "
                                         f"{x.dtype} {tuple(x.shape)}" + ("" if x.is_contiguous() else " (not contiguous)"))
    return x


# ---- marshalling: each takes the C function and its leading arguments, and appends the out-parameter(s) the idiom ends in ----------
def _resources(fn, *args) -> dict:
    """fz_kernel_resources out-parameter -> dict of its fields"""
    r = C.KernelResources()
    C.check(fn(*args, ctypes.byref(r)))
    return {n: getattr(r, n) for n, _ in C.KernelResources._fields_}


def _name(fn, *args, size: int = 160) -> str:
    """(char* buf, size) of a fixed-size name"""
    buf = ctypes.create_string_buffer(size)
    C.check(fn(*args, buf, size))
    return buf.value.decode()


def _text(fn, *args) -> str:
    """(char* buf, size) of a text of any length: asked for the length first, then for the text"""
    n = C.check(fn(*args, None, 0))
    buf = ctypes.create_string_buffer(n + 1)
    C.check(fn(*args, buf, n + 1))
    return buf.value.decode()


def _out(ctype, fn, *args) -> int:
    """an integer out-parameter of type ctype (ctypes.c_uint32 / ctypes.c_uint64)"""
    v = ctype()
    C.check(fn(*args, ctypes.byref(v)))
    return int(v.value)


def _window(x, row0, n_samples, in_grad):
    """the window of a stream-major front door as Program._run_grad takes it: (row0, rows of the block, in_grad); n_samples None: to the
    last row of x"""
    return int(row0), (x.shape[1] - int(row0)) if n_samples is None else int(n_samples), in_grad


# the C entry point of Program._run_grad by (ring, loss, stream-major window, recording)
_GRAD_ENTRY = {
    (False, False, False, False): "fz_run_block_grad",
    (False, True, False, False): "fz_run_block_loss_grad",
    (False, False, True, False): "fz_run_block_grad_stream_major",
    (False, True, True, False): "fz_run_block_loss_grad_stream_major",
    (True, False, False, False): "fz_run_block_ring_grad",
    (True, True, False, False): "fz_run_block_ring_loss_grad",
    (True, False, True, False): "fz_run_block_ring_grad_stream_major",
    (True, True, True, False): "fz_run_block_ring_loss_grad_stream_major",
    (False, False, False, True): "fz_run_recording_grad",
    (False, True, False, True): "fz_run_recording_loss_grad",
    (False, False, True, True): "fz_run_recording_grad",
    (False, True, True, True): "fz_run_recording_loss_grad",
    (True, False, False, True): "fz_run_recording_ring_grad",
    (True, True, False, True): "fz_run_recording_ring_loss_grad",
    (True, False, True, True): "fz_run_recording_ring_grad_stream_major",
    (True, True, True, True): "fz_run_recording_ring_loss_grad_stream_major",
}
# the far family (delay lines deeper than 256 samples), time-major frames: by (loss, recording)
_FAR_GRAD_ENTRY = {(False, False): "fz_run_block_far_grad", (True, False): "fz_run_block_far_loss_grad",
                   (False, True): "fz_run_recording_far_grad", (True, True): "fz_run_recording_far_loss_grad"}
# the far family on stream-major buffers, by (loss, recording): the recording calls take the layout as an argument
_FAR_GRAD_SM_ENTRY = {(False, False): "fz_run_block_far_grad_stream_major", (True, False): "fz_run_block_far_loss_grad_stream_major",
                      (False, True): "fz_run_recording_far_grad_for", (True, True): "fz_run_recording_far_loss_grad_for"}


class Program:
    """compile() result: lowered graph + its fused gfx950 kernels (flowz.hpp:1233-1249)."""

    def __init__(self, expr, typed: bool = False, in_dtypes: Optional[Sequence[str]] = None):
        self.expr = as_expr(expr)
        h = ctypes.c_void_p()
        if typed or in_dtypes is not None:
            # ResultType semantics (flowz.hpp:585-644): wire types carried through inputs, state and outputs
            n = self.expr.ins
            dts = list(in_dtypes) if in_dtypes is not None else ["f32"] * n
            arr = (ctypes.c_uint32 * _bi.max(len(dts), 1))(*[C.DTYPES[d] for d in dts])
            C.check(C.lib.fz_compile_typed(self.expr._h, arr, len(dts), ctypes.byref(h)))
        else:
            C.check(C.lib.fz_compile(self.expr._h, ctypes.byref(h)))
        self._adopt(h)
        # a graph the shipped reference evaluates against its own arity table (fz_info.differs_from_reference): the library's note about it
        self.note = C.lib.fz_last_error().decode() if self.differs_from_reference else ""

    def _adopt(self, h):
        self._h = h
        info = C.Info()
        C.check(C.lib.fz_program_info(self._h, ctypes.byref(info)))
        self.info = info
        for f, _ in C.Info._fields_:
            setattr(self, f, getattr(info, f))

    def wave_part(self, n_parts: int, k: int) -> "Program":
        """Part k of the wave split into n_parts (FZ_VF_WAVES) as a program of its own, for inspection: its input is the cut
        wire before the part, its output the cut wire behind it."""
        h = ctypes.c_void_p()
        C.check(C.lib.fz_program_wave_part(self._h, int(n_parts), int(k), ctypes.byref(h)))
        q = Program.__new__(Program)
        q.expr = None
        q._adopt(h)
        return q

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and C is not None:
            try:
                C.lib.fz_program_destroy(h)
            except Exception:
                pass

    # -- inspection ------------------------------------------------------------------------
    def ir(self):
        n = C.check(C.lib.fz_program_ir(self._h, None, 0))
        buf = (C.IrNode * _bi.max(n, 1))()
        C.check(C.lib.fz_program_ir(self._h, buf, n))
        # 4th field: the literal of a 'const' node; the third operand of a 'select' node (a != 0 ? b : c)
        return [(C.IR_KINDS[buf[i].kind], buf[i].a, buf[i].b,
                 buf[i].c if buf[i].kind == 14 else (buf[i].value64 if buf[i].dtype else buf[i].value))
                for i in range(n)]

    def ir_dtypes(self):
        """per IR node: 'f32' or 'f64' (the node's C++ arithmetic type)"""
        n = C.check(C.lib.fz_program_ir(self._h, None, 0))
        buf = (C.IrNode * _bi.max(n, 1))()
        C.check(C.lib.fz_program_ir(self._h, buf, n))
        return ["f64" if buf[i].dtype else "f32" for i in range(n)]

    def outputs(self):
        buf = (ctypes.c_uint32 * _bi.max(self.n_out, 1))()
        C.check(C.lib.fz_program_outputs(self._h, buf, self.n_out))
        return [buf[i] for i in range(self.n_out)]

    def output_dtypes(self):
        """'f32' / 'f64' / 'cf32' per output WIRE: its C++ type before narrowing to the float32 frame
        (a 'cf32' wire, std::complex<float>, takes two frame slots: re, im)."""
        buf = (ctypes.c_uint32 * _bi.max(self.n_out, 1))()
        C.check(C.lib.fz_program_output_dtypes(self._h, buf, self.n_out))
        names = {0: "f32", 1: "f64", 2: "cf32", 4: "f64", 6: "cf64", 10: "cf64"}   # the first slot of a wire names it
        return [names[buf[i]] for i in range(self.n_out) if buf[i] in names]

    def output_slot_codes(self):
        """raw per-slot codes of fz_program_output_dtypes: 0 float, 1 double (narrowed to the float frame), 2 / 3 re / im
        of a complex wire, 4 / 5 low / high word of a double wire (typed programs), 6 / 7 / 8 / 9 low / high word of the
        real, low / high word of the imaginary part of a std::complex<double> wire (typed programs), 10 / 11 re / im of a
        std::complex<double> wire narrowed to the float frame (compile())"""
        buf = (ctypes.c_uint32 * _bi.max(self.n_out, 1))()
        C.check(C.lib.fz_program_output_dtypes(self._h, buf, self.n_out))
        return [buf[i] for i in range(self.n_out)]

    def input_dtypes(self):
        """'f32' / 'f64' / 'cf32' per input WIRE (typed programs; all 'f32' otherwise)"""
        n = _bi.max(self.n_in_wires, 1)
        buf = (ctypes.c_uint32 * n)()
        k = C.check(C.lib.fz_program_input_dtypes(self._h, buf, n))
        return [("f32", "f64", "cf32", "cf64")[buf[i]] for i in range(k)]

    def line_dtypes(self):
        """storage type per delay line (in lines() order): 'f32', 'f64' (two state rows per slot), 're' / 'im' (the
        float lines of a std::complex<float> wire)"""
        n = _bi.max(self.n_lines, 1)
        buf = (ctypes.c_uint32 * n)()
        k = C.check(C.lib.fz_program_line_dtypes(self._h, buf, n))
        return [("f32", "f64", "re", "im", "re64", "im64")[buf[i]] for i in range(k)]

    def lines(self):
        n = self.n_lines
        s, d = (ctypes.c_uint32 * _bi.max(n, 1))(), (ctypes.c_uint32 * _bi.max(n, 1))()
        C.check(C.lib.fz_program_lines(self._h, s, d, n))
        return [(s[i], d[i]) for i in range(n)]

    def consts(self):
        out = []
        for k in range(self.n_const):
            v = ctypes.c_float()
            C.check(C.lib.fz_program_get_const(self._h, k, ctypes.byref(v)))
            out.append(v.value)
        return out

    def set_const(self, slot: int, value: float):
        C.check(C.lib.fz_program_set_const(self._h, int(slot), float(value)))

    def set_uniform(self, k: int, value: float):
        C.check(C.lib.fz_program_set_uniform(self._h, int(k), float(value)))

    def set_modulation(self, mod):
        """mod: CUDA float32 [n_mod, rows] (rows >= the samples the frame buffers of the next launches hold): sample t of a block
        reads modulator k at mod[k, row0 + t].  The tensor must stay alive until those launches have run."""
        import torch

        if not (hasattr(mod, "is_cuda") and mod.is_cuda and mod.dtype == torch.float32 and mod.is_contiguous() and mod.dim() == 2
                and mod.shape[0] >= self.n_mod):
            raise FlowzError(C.FZ_E_INVALID, f"set_modulation: need a contiguous CUDA float32 tensor [>= {self.n_mod}, rows]")
        self._mod_keepalive = mod
        C.check(C.lib.fz_program_set_modulation(self._h, mod.data_ptr(), int(mod.shape[1])))

    def recommended_tile_streams(self) -> int:
        """Streams per frame tile that gives ~32 KiB row segments (see fz_run_block_tiled)."""
        return int(C.lib.fz_recommended_tile_streams(self._h))

    def kernel_name(self, variant: Optional[Variant] = None, n_streams: int = 0, n_samples: int = 0, tile_streams: int = 0) -> str:
        """Name of the kernel variant that a launch of this shape runs (kernel_symbol: the symbol profilers show).  tile_streams: the frame layout (0 = plain
        time-major rows, as for run_block on a 3-D tensor); stream-major frames: FZ_VF_STREAM_MAJOR in the variant's flags."""
        vp = ctypes.byref(variant) if variant is not None else None
        return _name(C.lib.fz_program_kernel_name, self._h, vp, int(n_streams), int(n_samples), int(tile_streams), size=128)

    def kernel_symbol(self, variant: Optional[Variant] = None, n_streams: int = 0, n_samples: int = 0, tile_streams: int = 0) -> str:
        """kernel_name + "_g<graph tag>": the symbol in the code object, what rocprofv3 --kernel-trace --stats lists."""
        vp = ctypes.byref(variant) if variant is not None else None
        return _name(C.lib.fz_program_kernel_symbol, self._h, vp, int(n_streams), int(n_samples), int(tile_streams))

    def kernel_code_id(self, variant: Optional[Variant] = None, n_streams: int = 0, n_samples: int = 0, tile_streams: int = 0) -> str:
        """16 hex digits naming the CODE of that kernel (hash of generated source + build options + compiler): the code object's file name
        in the kernel cache.  Needs no GPU and builds nothing."""
        vp = ctypes.byref(variant) if variant is not None else None
        return _name(C.lib.fz_program_kernel_code_id, self._h, vp, int(n_streams), int(n_samples), int(tile_streams), size=32)

    def source(self, variant: Optional[Variant] = None) -> str:
        vp = ctypes.byref(variant) if variant is not None else None
        return _text(C.lib.fz_program_source, self._h, vp)

    def plan(self, n_streams: int, tile_streams: int = 0) -> Variant:
        """The variant a launch of this shape WITHOUT a variant would use on the current device: tuned in this process,
        else persisted by an earlier one (plans.txt in the kernel cache), else Variant(0,0,0,0) = the library default."""
        v = Variant(0, 0, 0, 0)
        C.check(C.lib.fz_program_plan(self._h, int(n_streams), int(tile_streams), ctypes.byref(v)))
        return v

    def tune_candidates(self, n_streams: int, n_samples: int, tile_streams: int = 0):
        """The variants Program.tune would measure for this shape (the first one is the library default)."""
        n = C.check(C.lib.fz_program_tune_candidates(self._h, int(n_streams), int(n_samples), int(tile_streams), None, 0))
        buf = (Variant * _bi.max(n, 1))()
        C.check(C.lib.fz_program_tune_candidates(self._h, int(n_streams), int(n_samples), int(tile_streams), buf, n))
        return [Variant(buf[i].streams_per_lane, buf[i].unroll, buf[i].block_threads, buf[i].flags) for i in range(n)]

    def build(self, variant: Optional[Variant] = None, n_streams: int = 0, n_samples: int = 0, tile_streams: int = 0):
        """JIT-compile (or fetch from the on-disk cache) the kernel of `variant`; needs no GPU.  With a block shape the
        variant's automatic fields resolve as a launch of that shape would (else as for a large stream count)."""
        vp = ctypes.byref(variant) if variant is not None else None
        if n_streams:
            C.check(C.lib.fz_program_build_for(self._h, vp, int(n_streams), int(n_samples or 4096), int(tile_streams)))
        else:
            C.check(C.lib.fz_program_build(self._h, vp))
        return self

    def kernel_resources(self, variant: Optional[Variant] = None, n_streams: int = 1 << 20, n_samples: int = 4096,
                         as_launched: bool = True, tile_streams: int = 0) -> dict:
        """registers / LDS / scratch bytes per lane of a variant's kernel (JITs it; needs no GPU).  as_launched: with the
        unroll lowered until nothing spills, as run_block does ('unroll' = what runs); False: the variant exactly as given."""
        vp = ctypes.byref(variant) if variant is not None else None
        return _resources(C.lib.fz_program_kernel_resources, self._h, vp, int(n_streams), int(n_samples), int(tile_streams), int(as_launched))

    # -- the hot path ----------------------------------------------------------------------
    def run_block_ptr(self, in_ptr, out_ptr, state_ptr, params_ptr, n_streams, n_samples,
                      variant: Optional[Variant] = None, stream=None, tile_streams: int = 0):
        vp = ctypes.byref(variant) if variant is not None else None
        if tile_streams:
            C.check(C.lib.fz_run_block_tiled(self._h, in_ptr, out_ptr, state_ptr, params_ptr, int(n_streams),
                                             int(n_samples), int(tile_streams), vp, stream))
        else:
            C.check(C.lib.fz_run_block(self._h, in_ptr, out_ptr, state_ptr, params_ptr, int(n_streams),
                                       int(n_samples), vp, stream))

    def run_window(self, x, out, state, row0: int, n_samples: int, params=None, variant: Optional[Variant] = None):
        """Samples [row0, row0 + n_samples) of the frame buffers x / out (laid out as for run_block, holding
        more samples than the block): fz_run_block_window.  state advances; params as for run_block."""
        import torch

        _check_frames(x, _bi.max(self.n_in, 1))
        if x.dim() == 4:
            n_tiles, rows, tile, _ = x.shape
            ns = n_tiles * tile
            oshape = (n_tiles, rows, tile, self.n_out)
        else:
            rows, ns, _ = x.shape
            tile = 0
            oshape = (rows, ns, self.n_out)
        _check_dev(out, oshape, "out")
        if self.n_state:
            _check_dev(state, (self.n_state, ns), "state")
        pp = _check_dev(params, (self.n_param, ns), "params").data_ptr() if self.n_param else None
        vp = ctypes.byref(variant) if variant is not None else None
        C.check(C.lib.fz_run_block_window(self._h, x.data_ptr() if self.n_in else None, out.data_ptr(),
                                          state.data_ptr() if self.n_state else None, pp, ns, rows, int(row0), int(n_samples),
                                          tile, vp, torch.cuda.current_stream().cuda_stream))
        return out, state

    def run_block_stream_major(self, x, state=None, params=None, out=None, variant: Optional[Variant] = None, row0: int = 0,
                               n_samples: Optional[int] = None):
        """x: CUDA float32 [n_streams, rows, n_in] -- one contiguous buffer per stream (the reference's calling
        convention); out [n_streams, rows, n_out].  No layout pass (fz_run_block_stream_major); the block is
        rows [row0, row0 + n_samples).  Returns (out, state)."""
        import torch

        if x.dim() == 2:
            x = x.unsqueeze(-1)
        _check_frames(x, _bi.max(self.n_in, 1))
        ns, rows, _ = x.shape
        n = rows - row0 if n_samples is None else int(n_samples)
        if out is None:
            out = torch.empty((ns, rows, self.n_out), dtype=torch.float32, device=x.device)
        if state is None:
            state = torch.zeros((_bi.max(self.n_state, 1), ns), dtype=torch.float32, device=x.device)
        _check_dev(out, (ns, rows, self.n_out), "out")
        _check_dev(state, (_bi.max(self.n_state, 1), ns), "state")
        pp = _check_dev(params, (self.n_param, ns), "params").data_ptr() if self.n_param else None
        vp = ctypes.byref(variant) if variant is not None else None
        C.check(C.lib.fz_run_block_stream_major(self._h, x.data_ptr() if self.n_in else None, out.data_ptr(),
                                                state.data_ptr() if self.n_state else None, pp, ns, rows, int(row0), n, vp,
                                                torch.cuda.current_stream().cuda_stream))
        return out, state

    def run_block(self, x, state=None, params=None, out=None, variant: Optional[Variant] = None, out_f64: bool = False):
        """x: CUDA float32 frames, either time-major [T, n_streams, n_in] or stream-tiled
        [n_tiles, T, tile_streams, n_in] (the HBM-friendly layout, see fz_run_block_tiled).
        state: [n_state, n_streams] in/out (allocated zeroed when None), params: [n_param, n_streams].
        out_f64: float64 output frames (results of double sub-expressions leave un-narrowed).
        Launches on torch's current stream; returns (out, state), out laid out like x."""
        import torch

        if not x.is_cuda:
            raise NoDeviceError(C.FZ_E_NO_DEVICE, "run_block needs CUDA (ROCm) tensors: zignal_amd has no CPU path")
        if x.dim() == 2:
            x = x.unsqueeze(-1)
        _check_frames(x, self.n_in)
        if x.dim() == 4:
            n_tiles, T, tile, _ = x.shape
            ns = n_tiles * tile
            oshape = (n_tiles, T, tile, self.n_out)
        else:
            T, ns, _ = x.shape
            tile = 0
            oshape = (T, ns, self.n_out)
        odt = torch.float64 if out_f64 else torch.float32
        if out_f64:
            v0 = variant if variant is not None else Variant(0, 0, 0, 0)
            variant = Variant(v0.streams_per_lane, v0.unroll, v0.block_threads, v0.flags | C.FZ_VF_OUT_F64)
        if out is None:
            out = torch.empty(oshape, dtype=odt, device=x.device)
        _check_dev(out, oshape, "out", odt)
        if state is None:
            state = torch.zeros((_bi.max(self.n_state, 1), ns), dtype=torch.float32, device=x.device)
        if self.n_state:
            _check_dev(state, (self.n_state, ns), "state")
        pp = None
        if self.n_param:
            if params is None:
                raise FlowzError(C.FZ_E_INVALID, f"params: the graph has {self.n_param} per-stream coefficient(s), none given")
            pp = _check_dev(params, (self.n_param, ns), "params").data_ptr()
        self.run_block_ptr(x.data_ptr() if self.n_in else None, out.data_ptr(),
                           state.data_ptr() if self.n_state else None, pp, ns, T, variant,
                           torch.cuda.current_stream().cuda_stream, tile)
        return out, state

    # -- 16-bit PCM frames (fz_run_block_pcm16) ------------------------------------------------------
    def pcm16_supported(self) -> bool:
        """True when fz_run_block_pcm16 takes this program (pcm16_unsupported_reason() says why not)."""
        return C.lib.fz_program_pcm16_check(self._h) == C.FZ_OK

    def pcm16_unsupported_reason(self) -> str:
        return "" if self.pcm16_supported() else C.last_error()

    @staticmethod
    def _frame_type(dtype, what):
        """FZ_FRAMES_* of a torch / numpy dtype or of the strings "int16" / "float32" """
        name = str(dtype).replace("torch.", "").replace("<class 'numpy.", "").replace("'>", "")
        _require(name in ("int16", "float32"), f"{what}: frames are int16 or float32, not {dtype}")
        return C.FZ_FRAMES_I16 if name == "int16" else C.FZ_FRAMES_F32

    def pcm16_resources(self, in_dtype="int16", out_dtype="int16", n_streams: int = 0) -> dict:
        """registers / scratch bytes of the PCM kernel a block of these frame types and this stream count (0: 2^20) runs (JITs it; needs
        no GPU); 'unroll' = rows per chunk"""
        return _resources(C.lib.fz_program_pcm16_resources, self._h, self._frame_type(in_dtype, "in_dtype"), self._frame_type(out_dtype, "out_dtype"), int(n_streams))

    def pcm16_kernel_symbol(self, in_dtype="int16", out_dtype="int16", n_streams: int = 0) -> str:
        return _name(C.lib.fz_program_pcm16_kernel_symbol, self._h, self._frame_type(in_dtype, "in_dtype"), self._frame_type(out_dtype, "out_dtype"), int(n_streams))

    def pcm16_source(self, in_dtype="int16", out_dtype="int16", n_streams: int = 0) -> str:
        """the PCM kernel's whole source: generated configuration and body, the common head, the PCM frame walk"""
        return _text(C.lib.fz_program_pcm16_source, self._h, self._frame_type(in_dtype, "in_dtype"), self._frame_type(out_dtype, "out_dtype"), int(n_streams))

    def run_block_pcm16(self, x, state=None, params=None, out=None, out_dtype=None):
        """run_block with 16-bit PCM frames on one side or on both: x is a CUDA int16 or float32 tensor [T, n_streams, n_in] (or
        [T, n_streams] for one wire), the output int16 or float32 as out_dtype says (default: x.dtype); one side at least is int16.
        In: x = q / 32768, exact.  Out: y * 32768 rounded to nearest, ties to even, saturated to [-32768, 32767], NaN -> 0
        (include/flowz_hip.h states the rule).  out may be x itself when both sides are int16 and n_out == n_in.
        state / params as for run_block; returns (out, state)."""
        import torch

        if not x.is_cuda:
            raise NoDeviceError(C.FZ_E_NO_DEVICE, "run_block_pcm16 needs CUDA (ROCm) tensors: zignal_amd has no CPU path")
        if x.dim() == 2:
            x = x.unsqueeze(-1)
        it = self._frame_type(x.dtype, "x")
        _require(x.dim() == 3 and x.is_contiguous() and x.shape[-1] == _bi.max(self.n_in, 1),
                 f"x: expected contiguous frames [T, n_streams, {self.n_in}], got {tuple(x.shape)}")
        T, ns, _ = x.shape
        odt = x.dtype if out_dtype is None else out_dtype
        ot = self._frame_type(odt, "out_dtype")
        odt = torch.int16 if ot == C.FZ_FRAMES_I16 else torch.float32
        if out is None:
            out = torch.empty((T, ns, self.n_out), dtype=odt, device=x.device)
        _check_dev(out, (T, ns, self.n_out), "out", odt)
        if state is None:
            state = torch.zeros((_bi.max(self.n_state, 1), ns), dtype=torch.float32, device=x.device)
        if self.n_state:
            _check_dev(state, (self.n_state, ns), "state")
        pp = None
        if self.n_param:
            if params is None:
                raise FlowzError(C.FZ_E_INVALID, f"params: the graph has {self.n_param} per-stream coefficient(s), none given")
            pp = _check_dev(params, (self.n_param, ns), "params").data_ptr()
        C.check(C.lib.fz_run_block_pcm16(self._h, x.data_ptr() if self.n_in else None, out.data_ptr(), state.data_ptr() if self.n_state else None,
                                         pp, ns, T, it, ot, torch.cuda.current_stream().cuda_stream))
        return out, state

    # -- 16-bit PCM frames on stream-major buffers (fz_run_block_pcm16_stream_major) -----------------
    def pcm16_stream_major_resources(self, in_dtype="int16", out_dtype="int16") -> dict:
        """registers / scratch / LDS bytes of the kernel a stream-major PCM block of these frame types runs (JITs it; needs no GPU);
        'unroll' = rows per chunk"""
        return _resources(C.lib.fz_program_pcm16_stream_major_resources, self._h, self._frame_type(in_dtype, "in_dtype"), self._frame_type(out_dtype, "out_dtype"))

    def pcm16_stream_major_kernel_symbol(self, in_dtype="int16", out_dtype="int16") -> str:
        return _name(C.lib.fz_program_pcm16_stream_major_kernel_symbol, self._h, self._frame_type(in_dtype, "in_dtype"), self._frame_type(out_dtype, "out_dtype"))

    def pcm16_stream_major_source(self, in_dtype="int16", out_dtype="int16") -> str:
        """that kernel's whole source: generated configuration and body, the common head, the stream-major PCM walk"""
        return _text(C.lib.fz_program_pcm16_stream_major_source, self._h, self._frame_type(in_dtype, "in_dtype"), self._frame_type(out_dtype, "out_dtype"))

    def run_block_pcm16_stream_major(self, x, state=None, params=None, out=None, out_dtype=None, row0=0, n_samples=None):
        """run_block_stream_major with 16-bit PCM frames on one side or on both: x is a CUDA int16 or float32 tensor
        [n_streams, rows, n_in] (or [n_streams, rows] for one wire: a [batch, time] tensor as it lies), the output
        [n_streams, rows, n_out] int16 or float32 as out_dtype says (default: x.dtype); one side at least is int16.  The block is
        the window of rows [row0, row0 + n_samples) (default: to the end); rows of out outside it are not written.  The
        conversion rule of run_block_pcm16.  rows * wires and row0 * wires are multiples of 8 on an int16 side, of 4 on a float32
        side.  out may be x itself when both sides are int16 and n_out == n_in.  Returns (out, state)."""
        import torch

        if not x.is_cuda:
            raise NoDeviceError(C.FZ_E_NO_DEVICE, "run_block_pcm16_stream_major needs CUDA (ROCm) tensors: zignal_amd has no CPU path")
        if x.dim() == 2:
            x = x.unsqueeze(-1)
        it = self._frame_type(x.dtype, "x")
        _require(x.dim() == 3 and x.is_contiguous() and x.shape[-1] == _bi.max(self.n_in, 1),
                 f"x: expected contiguous buffers [n_streams, rows, {self.n_in}], got {tuple(x.shape)}")
        ns, rows, _ = x.shape
        row0 = int(row0)
        T = rows - row0 if n_samples is None else int(n_samples)
        _require(row0 >= 0 and T >= 0, "row0 / n_samples: a window inside the buffers")
        odt = x.dtype if out_dtype is None else out_dtype
        ot = self._frame_type(odt, "out_dtype")
        odt = torch.int16 if ot == C.FZ_FRAMES_I16 else torch.float32
        if out is None:
            out = torch.zeros((ns, rows, self.n_out), dtype=odt, device=x.device)
        _check_dev(out, (ns, rows, self.n_out), "out", odt)
        if state is None:
            state = torch.zeros((_bi.max(self.n_state, 1), ns), dtype=torch.float32, device=x.device)
        if self.n_state:
            _check_dev(state, (self.n_state, ns), "state")
        pp = None
        if self.n_param:
            if params is None:
                raise FlowzError(C.FZ_E_INVALID, f"params: the graph has {self.n_param} per-stream coefficient(s), none given")
            pp = _check_dev(params, (self.n_param, ns), "params").data_ptr()
        C.check(C.lib.fz_run_block_pcm16_stream_major(self._h, x.data_ptr() if self.n_in else None, out.data_ptr() if self.n_out else None,
                                                      state.data_ptr() if self.n_state else None, pp, ns, rows, row0, T, it, ot,
                                                      torch.cuda.current_stream().cuda_stream))
        return out, state

    # -- delay lines deeper than 256 samples on stream-major buffers, forward (fz_run_block_far_stream_major) --------
    def far_stream_major_supported(self) -> bool:
        """True when fz_run_block_far_stream_major takes this program (far_stream_major_unsupported_reason() says why not)."""
        return C.lib.fz_program_far_stream_major_check(self._h) == C.FZ_OK

    def far_stream_major_unsupported_reason(self) -> str:
        return "" if self.far_stream_major_supported() else C.last_error()

    def far_stream_major_resources(self) -> dict:
        """registers / scratch / LDS bytes of the kernel run_block_far_stream_major runs (JITs it; needs no GPU); 'unroll' = the rows G
        of one unrolled group"""
        return _resources(C.lib.fz_program_far_stream_major_resources, self._h)

    def far_stream_major_kernel_symbol(self) -> str:
        """fz_far_sm_kernel_g<G>r<R>b<lanes>_g<graph tag>; a graph without a far line: run_block_stream_major's default kernel"""
        return _name(C.lib.fz_program_far_stream_major_kernel_symbol, self._h)

    def far_stream_major_source(self) -> str:
        """that kernel's whole source: generated configuration and body, the common head, the stream-major far walk"""
        return _text(C.lib.fz_program_far_stream_major_source, self._h)

    def run_block_far_stream_major(self, x, state=None, params=None, out=None, row0=0, n_samples=None):
        """run_block_stream_major for a graph with delay lines deeper than 256 samples (rings in HBM): x is a CUDA float32 tensor
        [n_streams, rows, n_in] (or [n_streams, rows] for one wire: a [batch, time] tensor as it lies), out [n_streams, rows, n_out].
        The block is the window of rows [row0, row0 + n_samples) (default: to the end); rows of out outside it are not written.
        out and state are bit for bit run_block's on the transposed frames; the far rings are read and written in the rows of state.
        rows * wires and row0 * wires are multiples of 4.  A graph without such a line runs run_block_stream_major's default kernel.
        Returns (out, state)."""
        import torch

        if not x.is_cuda:
            raise NoDeviceError(C.FZ_E_NO_DEVICE, "run_block_far_stream_major needs CUDA (ROCm) tensors: zignal_amd has no CPU path")
        if x.dim() == 2:
            x = x.unsqueeze(-1)
        _check_frames(x, _bi.max(self.n_in, 1))
        ns, rows, _ = x.shape
        row0 = int(row0)
        T = rows - row0 if n_samples is None else int(n_samples)
        _require(row0 >= 0 and T >= 0, "row0 / n_samples: a window inside the buffers")
        if out is None:
            out = torch.zeros((ns, rows, self.n_out), dtype=torch.float32, device=x.device)
        _check_dev(out, (ns, rows, self.n_out), "out")
        if state is None:
            state = torch.zeros((_bi.max(self.n_state, 1), ns), dtype=torch.float32, device=x.device)
        if self.n_state:
            _check_dev(state, (self.n_state, ns), "state")
        pp = None
        if self.n_param:
            if params is None:
                raise FlowzError(C.FZ_E_INVALID, f"params: the graph has {self.n_param} per-stream coefficient(s), none given")
            pp = _check_dev(params, (self.n_param, ns), "params").data_ptr()
        C.check(C.lib.fz_run_block_far_stream_major(self._h, x.data_ptr() if self.n_in else None, out.data_ptr() if self.n_out else None,
                                                    state.data_ptr() if self.n_state else None, pp, ns, rows, row0, T,
                                                    torch.cuda.current_stream().cuda_stream))
        return out, state

    # -- the backward of a block (fz_run_block_grad) ------------------------------------------------
    GRAD_WANT = ("x", "state", "params", "consts")

    def grad_supported(self) -> bool:
        """True when fz_run_block_grad takes this program (grad_unsupported_reason() says why not)."""
        return C.lib.fz_program_grad_check(self._h) == C.FZ_OK

    def grad_unsupported_reason(self) -> str:
        return "" if self.grad_supported() else C.last_error()

    def grad_workspace_bytes(self, n_streams: int, T: int, checkpoint_rows: int = 0) -> int:
        return _out(ctypes.c_uint64, C.lib.fz_program_grad_workspace, self._h, int(n_streams), int(T), int(checkpoint_rows))

    def grad_resources(self, checkpoint_rows: int = 0, stream_major: bool = False) -> dict:
        """registers / scratch / LDS bytes of the adjoint kernel (JITs it; needs no GPU); 'unroll' = the checkpoint stride it uses.
        stream_major: the kernel of run_block_grad_stream_major"""
        return _resources(C.lib.fz_program_grad_resources_for, self._h, int(checkpoint_rows), int(bool(stream_major)))

    def grad_kernel_symbol(self, checkpoint_rows: int = 0, stream_major: bool = False) -> str:
        return _name(C.lib.fz_program_grad_kernel_symbol_for, self._h, int(checkpoint_rows), int(bool(stream_major)))

    def grad_source(self, checkpoint_rows: int = 0, stream_major: bool = False) -> str:
        """the adjoint kernel's whole source: generated configuration and body, then the hand-written skeleton"""
        return _text(C.lib.fz_program_grad_source_for, self._h, int(checkpoint_rows), int(bool(stream_major)))

    def run_block_grad(self, x, out_grad, state=None, params=None, state_grad=None, want=GRAD_WANT, accum=None, checkpoint_rows: int = 0):
        """Reverse-mode gradients of the block run_block(x, state, params) computes (time-major frames; run_block_grad_stream_major takes [n_streams, rows, wire]): out_grad = dL/dy
        [T, n_streams, n_out], state_grad = dL/d(state after the block) [n_state, n_streams] (None: zero).  state = the state BEFORE
        the block (None: zeros; read only).  want: which of "x" (dL/dx, like x), "state" (dL/d(state before), [n_state, n_streams]),
        "params" ([n_param, n_streams]) and "consts" ([n_const, n_streams]: per stream, not summed) to compute.  accum: optional dict
        with "params" / "consts" tensors the gradients are ADDED to (returned as those entries); otherwise they start from zero.
        The uniform coefficients are the program's current constants.  Launches on torch's current stream; returns a dict."""
        return self._run_grad(x, out_grad, state, params, state_grad, want, accum, checkpoint_rows, None)

    def run_block_grad_stream_major(self, x, out_grad, state=None, params=None, state_grad=None, want=GRAD_WANT, accum=None,
                                    checkpoint_rows: int = 0, row0: int = 0, n_samples: Optional[int] = None, in_grad=None):
        """run_block_grad on stream-major buffers, the layout of run_block_stream_major: x [n_streams, rows, n_in] (or [n_streams, rows]
        for one input wire), out_grad [n_streams, rows, n_out]; the block is rows [row0, row0 + n_samples) (n_samples None: to the last
        row).  No layout pass (fz_run_block_grad_stream_major), and not a bit differs from run_block_grad on the transposed frames.
        Returns the same dict, "x" laid out like x: only the rows of the window are written.  in_grad: the tensor to write them to
        (returned as "x"), so that consecutive windows fill one tensor; otherwise a new one, zero outside the window."""
        return self._run_grad(x, out_grad, state, params, state_grad, want, accum, checkpoint_rows, _window(x, row0, n_samples, in_grad))

    # -- the backward of a block with delay lines deeper than 8 samples (fz_run_block_ring_grad): a call family of its own --------------
    def ring_grad_supported(self) -> bool:
        """True when fz_run_block_ring_grad takes this program: what grad_supported() takes, and graphs with float delay lines of 9 ..
        256 samples whose adjoint rings fit a workgroup's LDS (ring_grad_unsupported_reason() says why not)."""
        return C.lib.fz_program_ring_grad_check(self._h) == C.FZ_OK

    def ring_grad_unsupported_reason(self) -> str:
        return "" if self.ring_grad_supported() else C.last_error()

    def ring_grad_workspace_bytes(self, n_streams: int, T: int, checkpoint_rows: int = 0) -> int:
        return _out(ctypes.c_uint64, C.lib.fz_program_ring_grad_workspace, self._h, int(n_streams), int(T), int(checkpoint_rows))

    def ring_grad_resources(self, c: int = 0, stream_major: bool = False) -> dict:
        """grad_resources() of the kernel of run_block_ring_grad at checkpoint stride c (0: the library default); 'lds_bytes' = the
        adjoint rings of one workgroup.  stream_major: the kernel of run_block_ring_grad_stream_major ('lds_bytes': rings and patches)"""
        return _resources(C.lib.fz_program_ring_grad_resources_for, self._h, int(c), int(bool(stream_major)))

    def ring_grad_kernel_symbol(self, c: int = 0, stream_major: bool = False) -> str:
        return _name(C.lib.fz_program_ring_grad_kernel_symbol_for, self._h, int(c), int(bool(stream_major)))

    def ring_grad_source(self, c: int = 0, stream_major: bool = False) -> str:
        return _text(C.lib.fz_program_ring_grad_source_for, self._h, int(c), int(bool(stream_major)))

    def run_block_ring_grad(self, x, out_grad, state=None, params=None, state_grad=None, want=GRAD_WANT, accum=None, checkpoint_rows: int = 0):
        """run_block_grad for graphs with delay lines deeper than 8 samples (fz_run_block_ring_grad): the same arguments, the same
        result dict, the same order of every sum; time-major frames only.  For a graph run_block_grad takes it is run_block_grad."""
        return self._run_grad(x, out_grad, state, params, state_grad, want, accum, checkpoint_rows, None, ring=True)

    def run_block_ring_grad_stream_major(self, x, out_grad, state=None, params=None, state_grad=None, want=GRAD_WANT, accum=None,
                                         checkpoint_rows: int = 0, row0: int = 0, n_samples: Optional[int] = None, in_grad=None):
        """run_block_ring_grad on stream-major buffers (fz_run_block_ring_grad_stream_major): the arguments, windows and result dict of
        run_block_grad_stream_major; not a bit differs from run_block_ring_grad on the transposed frames.  For a graph
        run_block_grad_stream_major takes it is run_block_grad_stream_major."""
        return self._run_grad(x, out_grad, state, params, state_grad, want, accum, checkpoint_rows, _window(x, row0, n_samples, in_grad), ring=True)

    # -- the backward under a squared-error loss (fz_run_block_loss_grad): dL/dy formed in the kernel from a target ------------------
    LOSS_GRAD_WANT = GRAD_WANT + ("loss", "out")

    def loss_grad_resources(self, checkpoint_rows: int = 0, stream_major: bool = False) -> dict:
        """grad_resources() of the kernel of run_block_loss_grad (stream_major: of run_block_loss_grad_stream_major)"""
        return _resources(C.lib.fz_program_loss_grad_resources_for, self._h, int(checkpoint_rows), int(bool(stream_major)))

    def loss_grad_kernel_symbol(self, checkpoint_rows: int = 0, stream_major: bool = False) -> str:
        return _name(C.lib.fz_program_loss_grad_kernel_symbol_for, self._h, int(checkpoint_rows), int(bool(stream_major)))

    def loss_grad_source(self, checkpoint_rows: int = 0, stream_major: bool = False) -> str:
        return _text(C.lib.fz_program_loss_grad_source_for, self._h, int(checkpoint_rows), int(bool(stream_major)))

    def run_block_loss_grad(self, x, target, state=None, params=None, state_grad=None, grad_scale: float = 1.0, want=LOSS_GRAD_WANT, accum=None,
                            checkpoint_rows: int = 0):
        """run_block_grad with dL/dy formed in the kernel (fz_run_block_loss_grad): per row and output slot e = y - target, dL/dy = e *
        grad_scale, loss[stream] += e * e -- one launch, neither y nor dL/dy crosses HBM.  target [T, n_streams, n_out].  want: as for
        run_block_grad, plus "loss" ([n_streams], the per-stream sums of e * e) and "out" (y, like target: the bits of run_block).
        accum: "params" / "consts" / "loss" tensors that are ADDED to.  Returns a dict."""
        return self._run_grad(x, target, state, params, state_grad, want, accum, checkpoint_rows, None, (float(grad_scale), None))

    def run_block_loss_grad_stream_major(self, x, target, state=None, params=None, state_grad=None, grad_scale: float = 1.0, want=LOSS_GRAD_WANT,
                                         accum=None, checkpoint_rows: int = 0, row0: int = 0, n_samples: Optional[int] = None, in_grad=None,
                                         out=None):
        """run_block_loss_grad on stream-major buffers, windows as for run_block_grad_stream_major: x [n_streams, rows, n_in], target
        [n_streams, rows, n_out].  in_grad / out: the tensors the window's rows of "x" / "out" are written to (otherwise new ones, zero
        outside the window).  Not a bit differs from run_block_loss_grad on the transposed frames."""
        return self._run_grad(x, target, state, params, state_grad, want, accum, checkpoint_rows, _window(x, row0, n_samples, in_grad), (float(grad_scale), out))

    # -- the squared-error backward of a block with delay lines deeper than 8 samples (fz_run_block_ring_loss_grad) -------------------
    def ring_loss_grad_resources(self, c: int = 0, stream_major: bool = False) -> dict:
        """ring_grad_resources() of the kernel of run_block_ring_loss_grad at checkpoint stride c (0: the library default);
        stream_major: of run_block_ring_loss_grad_stream_major"""
        return _resources(C.lib.fz_program_ring_loss_grad_resources_for, self._h, int(c), int(bool(stream_major)))

    def ring_loss_grad_kernel_symbol(self, c: int = 0, stream_major: bool = False) -> str:
        return _name(C.lib.fz_program_ring_loss_grad_kernel_symbol_for, self._h, int(c), int(bool(stream_major)))

    def ring_loss_grad_source(self, c: int = 0, stream_major: bool = False) -> str:
        return _text(C.lib.fz_program_ring_loss_grad_source_for, self._h, int(c), int(bool(stream_major)))

    def run_block_ring_loss_grad(self, x, target, state=None, params=None, state_grad=None, grad_scale: float = 1.0, want=LOSS_GRAD_WANT, accum=None,
                                 checkpoint_rows: int = 0):
        """run_block_loss_grad for graphs with delay lines deeper than 8 samples (fz_run_block_ring_loss_grad): the same arguments, the
        same result dict, the rule of run_block_loss_grad and then the order of run_block_ring_grad; time-major frames only, the
        workspace of run_block_ring_grad.  For a graph run_block_loss_grad takes it is run_block_loss_grad."""
        return self._run_grad(x, target, state, params, state_grad, want, accum, checkpoint_rows, None, (float(grad_scale), None), ring=True)

    def run_block_ring_loss_grad_stream_major(self, x, target, state=None, params=None, state_grad=None, grad_scale: float = 1.0,
                                              want=LOSS_GRAD_WANT, accum=None, checkpoint_rows: int = 0, row0: int = 0,
                                              n_samples: Optional[int] = None, in_grad=None, out=None):
        """run_block_ring_loss_grad on stream-major buffers (fz_run_block_ring_loss_grad_stream_major): the arguments, windows and
        result dict of run_block_loss_grad_stream_major; not a bit differs from run_block_ring_loss_grad on the transposed frames.  For
        a graph run_block_loss_grad_stream_major takes it is run_block_loss_grad_stream_major."""
        return self._run_grad(x, target, state, params, state_grad, want, accum, checkpoint_rows, _window(x, row0, n_samples, in_grad), (float(grad_scale), out),
                              ring=True)

    # -- the backward of a whole recording (fz_run_recording_grad): two-level checkpointing over the calls above ---------------------
    def recording_block_rows(self, T: int, block_rows: int = 0, checkpoint_rows: int = 0) -> int:
        """the rows per block a recording of T rows is cut into (block_rows = 0: the library's choice; include/flowz_hip.h has the rule)"""
        return _out(ctypes.c_uint32, C.lib.fz_program_recording_block_rows, self._h, int(T), int(block_rows), int(checkpoint_rows))

    def recording_workspace_bytes(self, n_streams: int, T: int, block_rows: int = 0, checkpoint_rows: int = 0, stream_major: bool = False) -> int:
        """workspace bytes of run_recording_grad / run_recording_loss_grad: the block-start states, then one block's checkpoints"""
        return _out(ctypes.c_uint64, C.lib.fz_program_recording_workspace, self._h, int(n_streams), int(T), int(block_rows), int(checkpoint_rows), int(bool(stream_major)))

    def states_resources(self, stream_major: bool = False) -> dict:
        """grad_resources() of the block-start-states kernel of a recording; 'unroll' = the rows of its unrolled group"""
        return _resources(C.lib.fz_program_states_resources, self._h, int(bool(stream_major)))

    def states_kernel_symbol(self, stream_major: bool = False) -> str:
        return _name(C.lib.fz_program_states_kernel_symbol, self._h, int(bool(stream_major)))

    def states_source(self, stream_major: bool = False) -> str:
        return _text(C.lib.fz_program_states_source, self._h, int(bool(stream_major)))

    def run_recording_grad(self, x, out_grad, state=None, params=None, state_grad=None, want=GRAD_WANT, accum=None, checkpoint_rows: int = 0,
                           block_rows: int = 0, stream_major: bool = False, row0: int = 0, n_samples: Optional[int] = None, in_grad=None,
                           workspace=None):
        """run_block_grad (stream_major: run_block_grad_stream_major, with its window and in_grad) over a whole recording in bounded
        workspace (fz_run_recording_grad): the recording runs forward once keeping only the state before every block of block_rows rows
        (0: the library's choice), then the blocks are differentiated from the last to the first.  Every bit is run_block_grad's over
        the same rows.  want may also name "state_out": the state after the last row (the bits of run_block's).  workspace: a float32
        tensor of at least recording_workspace_bytes to use (otherwise one is allocated).  Returns the dict of run_block_grad."""
        window = _window(x, row0, n_samples, in_grad) if stream_major else None
        return self._run_grad(x, out_grad, state, params, state_grad, want, accum, checkpoint_rows, window, None, (int(block_rows), workspace))

    def run_recording_loss_grad(self, x, target, state=None, params=None, state_grad=None, grad_scale: float = 1.0, want=LOSS_GRAD_WANT, accum=None,
                                checkpoint_rows: int = 0, block_rows: int = 0, stream_major: bool = False, row0: int = 0,
                                n_samples: Optional[int] = None, in_grad=None, out=None, workspace=None):
        """run_block_loss_grad (stream_major: run_block_loss_grad_stream_major) over a whole recording, as run_recording_grad is to
        run_block_grad: the same arguments, results and bits as the one-launch call over the same rows, plus "state_out" in want."""
        window = _window(x, row0, n_samples, in_grad) if stream_major else None
        return self._run_grad(x, target, state, params, state_grad, want, accum, checkpoint_rows, window, (float(grad_scale), out),
                              (int(block_rows), workspace))

    # -- the backward of a block with delay lines deeper than 256 samples (fz_run_block_far_grad): the far call family ------------------
    def far_grad_supported(self) -> bool:
        """True when fz_run_block_far_grad takes this program: what ring_grad_supported() takes, and graphs with float delay lines
        deeper than 256 samples, whose rings live in HBM (far_grad_unsupported_reason() says why not)."""
        return C.lib.fz_program_far_grad_check(self._h) == C.FZ_OK

    def far_grad_unsupported_reason(self) -> str:
        return "" if self.far_grad_supported() else C.last_error()

    def far_grad_workspace_bytes(self, n_streams: int, T: int, checkpoint_rows: int = 0) -> int:
        """workspace bytes of run_block_far_grad / run_block_far_loss_grad: checkpoints, the tape (ring and far lines) and the adjoint
        ring of the far lines, one row per slot"""
        return _out(ctypes.c_uint64, C.lib.fz_program_far_grad_workspace, self._h, int(n_streams), int(T), int(checkpoint_rows))

    def far_grad_resources(self, c: int = 0, stream_major: bool = False) -> dict:
        """grad_resources() of the kernel of run_block_far_grad at checkpoint stride c (0: the library default); 'lds_bytes' = the
        adjoint rings of the LDS ring lines alone: the far lines take none.  stream_major: the kernel of
        run_block_far_grad_stream_major ('lds_bytes': those rings and the patches)"""
        return _resources(C.lib.fz_program_far_grad_resources_for, self._h, int(c), int(bool(stream_major)))

    def far_grad_kernel_symbol(self, c: int = 0, stream_major: bool = False) -> str:
        return _name(C.lib.fz_program_far_grad_kernel_symbol_for, self._h, int(c), int(bool(stream_major)))

    def far_grad_source(self, c: int = 0, stream_major: bool = False) -> str:
        return _text(C.lib.fz_program_far_grad_source_for, self._h, int(c), int(bool(stream_major)))

    def run_block_far_grad(self, x, out_grad, state=None, params=None, state_grad=None, want=GRAD_WANT, accum=None, checkpoint_rows: int = 0):
        """run_block_ring_grad for graphs with delay lines deeper than 256 samples (fz_run_block_far_grad): the same arguments, the same
        result dict; time-major frames only.  The rows of such a line in `state`, state_grad and the "state" result are ring SLOTS, and
        its phase row follows the line rows (zero in "state").  For a graph run_block_ring_grad takes it is run_block_ring_grad."""
        return self._run_grad(x, out_grad, state, params, state_grad, want, accum, checkpoint_rows, None, ring=True, far=True)

    def run_block_far_grad_stream_major(self, x, out_grad, state=None, params=None, state_grad=None, want=GRAD_WANT, accum=None,
                                        checkpoint_rows: int = 0, row0: int = 0, n_samples: Optional[int] = None, in_grad=None):
        """run_block_far_grad on stream-major buffers (fz_run_block_far_grad_stream_major): the arguments, windows and result dict of
        run_block_ring_grad_stream_major; not a bit differs from run_block_far_grad on the transposed frames.  The state rows are
        [row, n_streams] in both layouts: a far line's slot rows and phase row are run_block_far_grad's.  For a graph
        run_block_ring_grad_stream_major takes it is run_block_ring_grad_stream_major."""
        return self._run_grad(x, out_grad, state, params, state_grad, want, accum, checkpoint_rows, _window(x, row0, n_samples, in_grad), ring=True, far=True)

    def far_loss_grad_resources(self, c: int = 0, stream_major: bool = False) -> dict:
        """far_grad_resources() of the kernel of run_block_far_loss_grad at checkpoint stride c (0: the library default);
        stream_major: of run_block_far_loss_grad_stream_major"""
        return _resources(C.lib.fz_program_far_loss_grad_resources_for, self._h, int(c), int(bool(stream_major)))

    def far_loss_grad_kernel_symbol(self, c: int = 0, stream_major: bool = False) -> str:
        return _name(C.lib.fz_program_far_loss_grad_kernel_symbol_for, self._h, int(c), int(bool(stream_major)))

    def far_loss_grad_source(self, c: int = 0, stream_major: bool = False) -> str:
        return _text(C.lib.fz_program_far_loss_grad_source_for, self._h, int(c), int(bool(stream_major)))

    def run_block_far_loss_grad(self, x, target, state=None, params=None, state_grad=None, grad_scale: float = 1.0, want=LOSS_GRAD_WANT, accum=None,
                                checkpoint_rows: int = 0):
        """run_block_ring_loss_grad for graphs with delay lines deeper than 256 samples (fz_run_block_far_loss_grad): the same
        arguments, the same result dict, the rule of run_block_loss_grad and then the order of run_block_far_grad; time-major frames
        only, the workspace of run_block_far_grad.  For a graph run_block_ring_loss_grad takes it is run_block_ring_loss_grad."""
        return self._run_grad(x, target, state, params, state_grad, want, accum, checkpoint_rows, None, (float(grad_scale), None), ring=True, far=True)

    def run_block_far_loss_grad_stream_major(self, x, target, state=None, params=None, state_grad=None, grad_scale: float = 1.0,
                                             want=LOSS_GRAD_WANT, accum=None, checkpoint_rows: int = 0, row0: int = 0,
                                             n_samples: Optional[int] = None, in_grad=None, out=None):
        """run_block_far_loss_grad on stream-major buffers (fz_run_block_far_loss_grad_stream_major): the arguments, windows and
        result dict of run_block_ring_loss_grad_stream_major, in_grad and out included; not a bit differs from run_block_far_loss_grad
        on the transposed frames.  For a graph run_block_ring_loss_grad_stream_major takes it is that call."""
        return self._run_grad(x, target, state, params, state_grad, want, accum, checkpoint_rows, _window(x, row0, n_samples, in_grad), (float(grad_scale), out),
                              ring=True, far=True)

    # -- the backward of a whole recording with delay lines deeper than 256 samples (fz_run_recording_far_grad) ----------------------
    def far_recording_block_rows(self, T: int, block_rows: int = 0, checkpoint_rows: int = 0) -> int:
        """the rows per block run_recording_far_grad cuts a recording of T rows into (block_rows = 0: the library's choice, which
        counts the far lines among the tape lines; include/flowz_hip.h has the rule).  Without a far line: ring_recording_block_rows"""
        return _out(ctypes.c_uint32, C.lib.fz_program_far_recording_block_rows, self._h, int(T), int(block_rows), int(checkpoint_rows))

    def far_recording_workspace_bytes(self, n_streams: int, T: int, block_rows: int = 0, checkpoint_rows: int = 0) -> int:
        """workspace bytes of run_recording_far_grad / run_recording_far_loss_grad: the block-start states, then one block's far workspace"""
        return _out(ctypes.c_uint64, C.lib.fz_program_far_recording_workspace, self._h, int(n_streams), int(T), int(block_rows), int(checkpoint_rows))

    def far_states_resources(self, stream_major: bool = False) -> dict:
        """grad_resources() of the block-start-states kernel of a far recording; 'unroll' = the rows of its unrolled group, 'lds_bytes' =
        the value rings of the LDS ring lines of one workgroup (the far lines keep their working rings in the workspace).
        stream_major: the kernel of run_recording_far_grad(stream_major=True) ('lds_bytes': those rings and the x-only patches)"""
        return _resources(C.lib.fz_program_far_states_resources_for, self._h, int(bool(stream_major)))

    def far_states_kernel_symbol(self, stream_major: bool = False) -> str:
        return _name(C.lib.fz_program_far_states_kernel_symbol_for, self._h, int(bool(stream_major)))

    def far_states_source(self, stream_major: bool = False) -> str:
        return _text(C.lib.fz_program_far_states_source_for, self._h, int(bool(stream_major)))

    def run_recording_far_grad(self, x, out_grad, state=None, params=None, state_grad=None, want=GRAD_WANT, accum=None, checkpoint_rows: int = 0,
                               block_rows: int = 0, workspace=None, stream_major: bool = False, row0: int = 0, n_samples: Optional[int] = None,
                               in_grad=None):
        """run_block_far_grad over a whole recording in bounded workspace (fz_run_recording_far_grad), as run_recording_ring_grad is to
        run_block_ring_grad: every bit is run_block_far_grad's over the same rows, "state_out" may be named in want.  For a graph
        run_recording_ring_grad takes it is run_recording_ring_grad.
        stream_major (fz_run_recording_far_grad_for with FZ_GRAD_STREAM_MAJOR): x [n_streams, rows, n_in] (or [n_streams, rows] for
        one input wire: a [batch, time] tensor as it lies), the shapes, windows (row0, n_samples, in_grad) and result dict of
        run_recording_ring_grad_stream_major; not a bit differs from the time-major call on the transposed frames, nor from
        run_block_far_grad_stream_major over the same window.  Without it there is no window: row0 0, n_samples None or T, in_grad None."""
        if not stream_major:
            _require(int(row0) == 0 and (n_samples is None or int(n_samples) == x.shape[0]) and in_grad is None,
                     "run_recording_far_grad takes time-major frames unless stream_major: no window (row0, n_samples, in_grad)")
        return self._run_grad(x, out_grad, state, params, state_grad, want, accum, checkpoint_rows,
                              _window(x, row0, n_samples, in_grad) if stream_major else None, None, (int(block_rows), workspace), ring=True, far=True)

    def run_recording_far_loss_grad(self, x, target, state=None, params=None, state_grad=None, grad_scale: float = 1.0, want=LOSS_GRAD_WANT,
                                    accum=None, checkpoint_rows: int = 0, block_rows: int = 0, out=None, workspace=None,
                                    stream_major: bool = False, row0: int = 0, n_samples: Optional[int] = None, in_grad=None):
        """run_block_far_loss_grad over a whole recording (fz_run_recording_far_loss_grad): the arguments, results and bits of the
        one-launch call over the same rows, plus "state_out" in want.  stream_major (fz_run_recording_far_loss_grad_for with
        FZ_GRAD_STREAM_MAJOR): the arguments, windows and result dict of run_recording_ring_loss_grad_stream_major, in_grad and out
        included; not a bit differs from the time-major call on the transposed frames."""
        if not stream_major:
            _require(int(row0) == 0 and (n_samples is None or int(n_samples) == x.shape[0]) and in_grad is None,
                     "run_recording_far_loss_grad takes time-major frames unless stream_major: no window (row0, n_samples, in_grad)")
        return self._run_grad(x, target, state, params, state_grad, want, accum, checkpoint_rows,
                              _window(x, row0, n_samples, in_grad) if stream_major else None, (float(grad_scale), out),
                              (int(block_rows), workspace), ring=True, far=True)

    # -- the backward of a whole recording with delay lines deeper than 8 samples (fz_run_recording_ring_grad) -----------------------
    def ring_recording_block_rows(self, T: int, block_rows: int = 0, checkpoint_rows: int = 0) -> int:
        """the rows per block run_recording_ring_grad cuts a recording of T rows into (block_rows = 0: the library's choice, which
        counts the tape of the deep lines; include/flowz_hip.h has the rule)"""
        return _out(ctypes.c_uint32, C.lib.fz_program_ring_recording_block_rows, self._h, int(T), int(block_rows), int(checkpoint_rows))

    def ring_recording_workspace_bytes(self, n_streams: int, T: int, block_rows: int = 0, checkpoint_rows: int = 0) -> int:
        """workspace bytes of run_recording_ring_grad / run_recording_ring_loss_grad: the block-start states, then one block's ring workspace"""
        return _out(ctypes.c_uint64, C.lib.fz_program_ring_recording_workspace, self._h, int(n_streams), int(T), int(block_rows), int(checkpoint_rows))

    def ring_states_resources(self, stream_major: bool = False) -> dict:
        """grad_resources() of the block-start-states kernel of a ring recording; 'unroll' = the rows of its unrolled group, 'lds_bytes' =
        the value rings of one workgroup (the ring adjoint kernel's bytes).  stream_major: the kernel of
        run_recording_ring_grad_stream_major ('lds_bytes': rings and the x-only patches)"""
        return _resources(C.lib.fz_program_ring_states_resources_for, self._h, int(bool(stream_major)))

    def ring_states_kernel_symbol(self, stream_major: bool = False) -> str:
        return _name(C.lib.fz_program_ring_states_kernel_symbol_for, self._h, int(bool(stream_major)))

    def ring_states_source(self, stream_major: bool = False) -> str:
        return _text(C.lib.fz_program_ring_states_source_for, self._h, int(bool(stream_major)))

    def run_recording_ring_grad(self, x, out_grad, state=None, params=None, state_grad=None, want=GRAD_WANT, accum=None, checkpoint_rows: int = 0,
                                block_rows: int = 0, row0: int = 0, n_samples: Optional[int] = None, in_grad=None, workspace=None):
        """run_block_ring_grad over a whole recording in bounded workspace (fz_run_recording_ring_grad), as run_recording_grad is to
        run_block_grad: every bit is run_block_ring_grad's over the same rows, "state_out" may be named in want.  Time-major frames
        (stream-major buffers: run_recording_ring_grad_stream_major): row0 must be 0, n_samples None or T, in_grad None.  For a graph run_recording_grad takes it is run_recording_grad."""
        _require(int(row0) == 0 and (n_samples is None or int(n_samples) == x.shape[0]) and in_grad is None,
                 "run_recording_ring_grad takes time-major frames: no window (row0, n_samples, in_grad)")
        return self._run_grad(x, out_grad, state, params, state_grad, want, accum, checkpoint_rows, None, None, (int(block_rows), workspace), ring=True)

    def run_recording_ring_loss_grad(self, x, target, state=None, params=None, state_grad=None, grad_scale: float = 1.0, want=LOSS_GRAD_WANT,
                                     accum=None, checkpoint_rows: int = 0, block_rows: int = 0, row0: int = 0, n_samples: Optional[int] = None,
                                     in_grad=None, out=None, workspace=None):
        """run_block_ring_loss_grad over a whole recording (fz_run_recording_ring_loss_grad): the arguments, results and bits of the
        one-launch call over the same rows, plus "state_out" in want.  Time-major frames only, as run_recording_ring_grad."""
        _require(int(row0) == 0 and (n_samples is None or int(n_samples) == x.shape[0]) and in_grad is None,
                 "run_recording_ring_loss_grad takes time-major frames: no window (row0, n_samples, in_grad)")
        return self._run_grad(x, target, state, params, state_grad, want, accum, checkpoint_rows, None, (float(grad_scale), out),
                              (int(block_rows), workspace), ring=True)

    def run_recording_ring_grad_stream_major(self, x, out_grad, state=None, params=None, state_grad=None, want=GRAD_WANT, accum=None,
                                             checkpoint_rows: int = 0, block_rows: int = 0, row0: int = 0, n_samples: Optional[int] = None,
                                             in_grad=None, workspace=None):
        """run_recording_ring_grad on stream-major buffers (fz_run_recording_ring_grad_stream_major): x [n_streams, rows, n_in] (or
        [n_streams, rows] for one input wire: a [batch, time] tensor as it lies), the windows, in_grad and result dict of
        run_recording_grad(stream_major=True), the workspace of run_recording_ring_grad.  Not a bit differs from run_recording_ring_grad
        on the transposed frames, nor from run_block_ring_grad_stream_major over the same window.  For a graph run_recording_grad takes
        it is run_recording_grad(stream_major=True)."""
        return self._run_grad(x, out_grad, state, params, state_grad, want, accum, checkpoint_rows, _window(x, row0, n_samples, in_grad), None,
                              (int(block_rows), workspace), ring=True)

    def run_recording_ring_loss_grad_stream_major(self, x, target, state=None, params=None, state_grad=None, grad_scale: float = 1.0,
                                                  want=LOSS_GRAD_WANT, accum=None, checkpoint_rows: int = 0, block_rows: int = 0, row0: int = 0,
                                                  n_samples: Optional[int] = None, in_grad=None, out=None, workspace=None):
        """run_recording_ring_loss_grad on stream-major buffers (fz_run_recording_ring_loss_grad_stream_major): the arguments, windows
        and result dict of run_recording_loss_grad(stream_major=True); not a bit differs from run_recording_ring_loss_grad on the
        transposed frames."""
        return self._run_grad(x, target, state, params, state_grad, want, accum, checkpoint_rows, _window(x, row0, n_samples, in_grad),
                              (float(grad_scale), out), (int(block_rows), workspace), ring=True)

    def _run_grad(self, x, out_grad, state, params, state_grad, want, accum, checkpoint_rows, window, loss=None, recording=None, ring=False, far=False):
        """both frame layouts; window: None (time-major frames) or (row0, n_samples, in_grad) of stream-major buffers; loss: None, or
        (grad_scale, out tensor or None) of the squared-error backward, whose target comes as out_grad; recording: None (one block), or
        (block_rows, workspace tensor or None) of the calls over a whole recording; ring: the call is of the ring family:
        run_block_ring_grad / run_block_ring_loss_grad, or with recording run_recording_ring_grad / run_recording_ring_loss_grad, and their
        _stream_major twins; far (with ring): run_block_far_grad / run_block_far_loss_grad and their _stream_major twins, or with
        recording run_recording_far_grad / run_recording_far_loss_grad in either layout"""
        import torch

        if far:
            _require(self.far_grad_supported(), self.far_grad_unsupported_reason())
        elif ring:
            _require(self.ring_grad_supported(), self.ring_grad_unsupported_reason())
        else:
            _require(self.grad_supported(), self.grad_unsupported_reason())
        want = tuple(want)
        allowed = self.GRAD_WANT if loss is None else self.LOSS_GRAD_WANT
        if recording is not None:
            allowed = allowed + ("state_out",)
        _require(set(want) <= set(allowed), f"want: a subset of {allowed}")
        _require(loss is None or self.n_out, "the graph has no output wires: a loss has nothing to compare")
        if x.dim() == 2 and self.n_in == 1:
            x = x.unsqueeze(-1)
        _check_frames(x, self.n_in)
        if window is None:
            _require(x.dim() == 3, "run_block_grad takes time-major frames [T, n_streams, n_in]")
            T, ns, _ = x.shape
            gshape = (T, ns, self.n_out)
        else:
            _require(x.dim() == 3, "run_block_grad_stream_major takes stream-major buffers [n_streams, rows, n_in]")
            ns, rows, _ = x.shape
            row0, T, in_grad = window
            _require(0 <= row0 and 0 <= T and row0 + T <= rows, f"the window [{row0}, {row0 + T}) reaches beyond the {rows} rows of x")
            gshape = (ns, rows, self.n_out)
        dev = x.device
        if out_grad.dim() == 2 and self.n_out == 1:
            out_grad = out_grad.unsqueeze(-1)
        _check_dev(out_grad, gshape, "out_grad" if loss is None else "target")
        if state is None:
            state = torch.zeros((_bi.max(self.n_state, 1), ns), dtype=torch.float32, device=dev)
        if self.n_state:
            _check_dev(state, (self.n_state, ns), "state")
        if self.n_param:
            _require(params is not None, f"params: the graph has {self.n_param} per-stream coefficient(s), none given")
            _check_dev(params, (self.n_param, ns), "params")
        if state_grad is not None and self.n_state:
            _check_dev(state_grad, (self.n_state, ns), "state_grad")
        accum = dict(accum or {})
        out = {}
        if "x" in want:
            if window is None:
                out["x"] = torch.empty_like(x)
            elif in_grad is not None:
                out["x"] = _check_dev(in_grad.unsqueeze(-1) if in_grad.dim() == 2 and self.n_in == 1 else in_grad, tuple(x.shape), "in_grad")
            else:
                out["x"] = torch.empty_like(x) if (row0, T) == (0, rows) else torch.zeros_like(x)
        if "state" in want:
            out["state"] = torch.empty((_bi.max(self.n_state, 1), ns), dtype=torch.float32, device=dev)
        for key, nrow in (("params", self.n_param), ("consts", self.n_const)):
            if key in want:
                if key in accum:
                    out[key] = _check_dev(accum[key], (nrow, ns), f"accum[{key!r}]")
                else:
                    out[key] = torch.zeros((_bi.max(nrow, 1), ns), dtype=torch.float32, device=dev)
        if "loss" in want:
            out["loss"] = _check_dev(accum["loss"], (ns,), "accum['loss']") if "loss" in accum else torch.zeros((ns,), dtype=torch.float32, device=dev)
        if "out" in want:
            if loss[1] is not None:
                out["out"] = _check_dev(loss[1].unsqueeze(-1) if loss[1].dim() == 2 and self.n_out == 1 else loss[1], gshape, "out")
            else:
                out["out"] = torch.empty(gshape, dtype=torch.float32, device=dev) if window is None or (row0, T) == (0, rows) else \
                    torch.zeros(gshape, dtype=torch.float32, device=dev)
        state0_grad = out.get("state")
        if recording is None:
            wsb = (self.far_grad_workspace_bytes if far else self.ring_grad_workspace_bytes if ring else self.grad_workspace_bytes)(ns, T, checkpoint_rows)
        else:
            wsb = self.far_recording_workspace_bytes(ns, T, recording[0], checkpoint_rows) if far else \
                self.ring_recording_workspace_bytes(ns, T, recording[0], checkpoint_rows) if ring else \
                self.recording_workspace_bytes(ns, T, recording[0], checkpoint_rows, window is not None)
            if "state_out" in want:
                out["state_out"] = torch.zeros((_bi.max(self.n_state, 1), ns), dtype=torch.float32, device=dev)
            if state0_grad is None and self.n_state:        # (the blocks chain through it, asked for or not)
                state0_grad = torch.empty((self.n_state, ns), dtype=torch.float32, device=dev)
        if recording is not None and recording[1] is not None:
            ws = recording[1]
            _require(ws.is_cuda and ws.dtype == torch.float32 and ws.is_contiguous(), "workspace: a contiguous float32 tensor on the GPU")
        else:
            ws = torch.empty((_bi.max(wsb, 16) + 3) // 4, dtype=torch.float32, device=dev)

        def ptr(t, rows=1):
            return t.data_ptr() if t is not None and rows else None
        a = C.GradArgs() if loss is None else C.LossGradArgs()
        a.struct_size = ctypes.sizeof(a)
        a.checkpoint_rows = int(checkpoint_rows)
        a.in_ = ptr(x, self.n_in)
        a.state = ptr(state, self.n_state)
        a.params = ptr(params, self.n_param)
        if loss is None:
            a.out_grad = ptr(out_grad, self.n_out)
        else:
            a.target, a.grad_scale = ptr(out_grad, self.n_out), loss[0]
            a.loss, a.out = ptr(out.get("loss")), ptr(out.get("out"), self.n_out)
        a.state_grad = ptr(state_grad, self.n_state)
        a.in_grad = ptr(out.get("x"), self.n_in)
        a.state0_grad = ptr(state0_grad, self.n_state)
        a.param_grad = ptr(out.get("params"), self.n_param)
        a.const_grad = ptr(out.get("consts"), self.n_const)
        a.workspace = ws.data_ptr()
        a.workspace_bytes = ws.numel() * 4
        # (the workspace goes back to torch's caching allocator when this returns: it reuses the memory in the order of the stream)
        hs = torch.cuda.current_stream().cuda_stream
        fn = getattr(C.lib, _FAR_GRAD_SM_ENTRY[(loss is not None, recording is not None)] if far and window is not None else
                     _FAR_GRAD_ENTRY[(loss is not None, recording is not None)] if far else _GRAD_ENTRY[(bool(ring), loss is not None, window is not None, recording is not None)])
        if recording is not None and far and window is not None:      # far recording window: the layout is an argument
            C.check(fn(self._h, ctypes.byref(a), 1, int(ns), int(rows), row0, int(T), recording[0],    # (1: FZ_GRAD_STREAM_MAJOR)
                       ptr(out.get("state_out"), self.n_state), hs))
        elif recording is not None and ring and window is not None:   # ring recording window
            C.check(fn(self._h, ctypes.byref(a), int(ns), int(rows), row0, int(T), recording[0], ptr(out.get("state_out"), self.n_state), hs))
        elif recording is not None and ring:                          # ring recording
            C.check(fn(self._h, ctypes.byref(a), int(ns), int(T), recording[0], ptr(out.get("state_out"), self.n_state), hs))
        elif recording is not None:                                   # recording, either layout
            w = (int(rows), row0) if window is not None else (0, 0)
            C.check(fn(self._h, ctypes.byref(a), int(window is not None), int(ns), w[0], w[1], int(T), recording[0],
                       ptr(out.get("state_out"), self.n_state), hs))
        elif window is None:                                          # block
            C.check(fn(self._h, ctypes.byref(a), int(ns), int(T), hs))
        else:                                                         # block window
            C.check(fn(self._h, ctypes.byref(a), int(ns), int(rows), row0, T, hs))
        return out


def _tune(self, x, state=None, params=None, out=None):
    """Measure the candidate kernel variants for this shape on these buffers (fz_program_tune) and
    remember the fastest: later run_block calls of the same shape without a variant use it.
    x as for run_block; `state` advances (a scratch one is used when None), `out` is overwritten.
    Returns (Variant, milliseconds per block)."""
    import torch

    _check_frames(x, x.shape[-1])
    if x.dim() == 4:
        n_tiles, T, tile, _ = x.shape
        ns = n_tiles * tile
        oshape = (n_tiles, T, tile, self.n_out)
    else:
        T, ns, _ = x.shape
        tile = 0
        oshape = (T, ns, self.n_out)
    if out is None:
        out = torch.empty(oshape, dtype=torch.float32, device=x.device)
    if state is None:
        state = torch.zeros((_bi.max(self.n_state, 1), ns), dtype=torch.float32, device=x.device)
    _check_dev(out, oshape, "out")
    _check_dev(state, (_bi.max(self.n_state, 1), ns), "state")
    pp = _check_dev(params, (self.n_param, ns), "params").data_ptr() if self.n_param else None
    chosen, ms = Variant(0, 0, 0, 0), ctypes.c_float(0)
    C.check(C.lib.fz_program_tune(self._h, x.data_ptr() if self.n_in else None, out.data_ptr(),
                                  state.data_ptr() if self.n_state else None, pp, ns, T, tile,
                                  torch.cuda.current_stream().cuda_stream, ctypes.byref(chosen), ctypes.byref(ms)))
    return chosen, float(ms.value)


Program.tune = _tune


class Bank:
    """Device-resident closure state of n_streams streams of one program (fz_bank: the `state_` member of
    the reference's stateful_lambda, flowz.hpp:1190-1191, times n_streams)."""

    def __init__(self, prog: Program, n_streams: int):
        self.prog, self.n_streams = prog, int(n_streams)
        h = ctypes.c_void_p()
        C.check(C.lib.fz_bank_create(prog._h, self.n_streams, ctypes.byref(h)))
        self._h = h

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and C is not None:
            C.lib.fz_bank_destroy(h)

    def reset(self):
        C.check(C.lib.fz_bank_reset(self._h))

    def set_params(self, params):
        """params: numpy float32 [n_param, n_streams]"""
        import numpy as np
        p = np.ascontiguousarray(params, dtype=np.float32)
        _require(p.shape == (self.prog.n_param, self.n_streams), "p: wrong shape, dtype, layout or device for this call")
        C.check(C.lib.fz_bank_set_params_host(self._h, p.ctypes.data))

    def process_blocks(self, x, out, block_len: int, params_blocks=None, variant: Optional[Variant] = None):
        """Control-rate modulation: the frame buffers x / out (CUDA, time-major or stream-tiled) are processed in
        blocks of block_len samples, block k with the per-stream coefficient set params_blocks[k]
        (CUDA float32 [n_blocks, n_param, n_streams]); fz_bank_process_blocks."""
        import torch

        _require(x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.shape[-1] == _bi.max(self.prog.n_in, 1), "x: wrong shape, dtype, layout or device for this call")
        rows, tile = (x.shape[1], x.shape[2]) if x.dim() == 4 else (x.shape[0], 0)
        ns = x.shape[0] * x.shape[2] if x.dim() == 4 else x.shape[1]
        if ns != self.n_streams:
            raise FlowzError(C.FZ_E_INVALID, f"frames hold {ns} streams, the bank {self.n_streams}")
        _check_dev(out, tuple(x.shape[:-1]) + (self.prog.n_out,), "out")
        pp = None
        if params_blocks is not None:
            nb = (rows + block_len - 1) // block_len
            pp = _check_dev(params_blocks, (nb, self.prog.n_param, self.n_streams), "params_blocks").data_ptr()
        vp = ctypes.byref(variant) if variant is not None else None
        C.check(C.lib.fz_bank_process_blocks(self._h, x.data_ptr() if self.prog.n_in else None, out.data_ptr(), rows,
                                             int(block_len), pp, tile, vp, torch.cuda.current_stream().cuda_stream))
        return out

    def process_host_stream_major(self, x, out=None):
        """Host buffers, one contiguous row per stream: x [n_streams, T, n_in] -> [n_streams, T, n_out] (numpy
        arrays or CPU torch tensors; pinned memory overlaps the PCIe directions)."""
        import numpy as np

        is_torch = hasattr(x, "data_ptr")
        T = int(x.shape[1])
        if is_torch:
            import torch
            _require(x.dtype == torch.float32 and x.is_contiguous() and not x.is_cuda, "x: wrong shape, dtype, layout or device for this call")
            if out is None:
                out = torch.empty((self.n_streams, T, self.prog.n_out), dtype=torch.float32, pin_memory=x.is_pinned())
            xp, op = x.data_ptr(), out.data_ptr()
        else:
            x = np.ascontiguousarray(x, dtype=np.float32)
            if out is None:
                out = np.empty((self.n_streams, T, self.prog.n_out), np.float32)
            xp, op = x.ctypes.data, out.ctypes.data
        _require(tuple(x.shape) in ((self.n_streams, T, _bi.max(self.prog.n_in, 1)), (self.n_streams, T)), x.shape)
        _require(tuple(out.shape) == (self.n_streams, T, self.prog.n_out) and (out.is_contiguous() if is_torch else out.flags.c_contiguous), "out: wrong shape, dtype, layout or device for this call")
        _require((out.dtype == torch.float32) if is_torch else (out.dtype == np.float32), "out: wrong shape, dtype, layout or device for this call")
        C.check(C.lib.fz_bank_process_host_stream_major(self._h, xp if self.prog.n_in else None, op, T))
        return out

    def process_host(self, x, out=None, out_f64: bool = False):
        """Host frames in, host frames out (time-major [T, n_streams, n_in] float32 -> [T, n_streams, n_out]).
        x / out: numpy arrays or CPU torch tensors; pinned tensors let both PCIe directions overlap with
        the kernels (long blocks are pipelined in time chunks)."""
        import numpy as np

        is_torch = hasattr(x, "data_ptr")
        T = int(x.shape[0])
        if is_torch:
            import torch
            _require(x.dtype == torch.float32 and x.is_contiguous() and not x.is_cuda, "x: wrong shape, dtype, layout or device for this call")
            if out is None:
                out = torch.empty((T, self.n_streams, self.prog.n_out), dtype=torch.float64 if out_f64 else torch.float32,
                                  pin_memory=x.is_pinned())
            xp, op = x.data_ptr(), out.data_ptr()
        else:
            x = np.ascontiguousarray(x, dtype=np.float32)
            if out is None:
                out = np.empty((T, self.n_streams, self.prog.n_out), np.float64 if out_f64 else np.float32)
            xp, op = x.ctypes.data, out.ctypes.data
        _require(tuple(x.shape[1:]) in ((self.n_streams, self.prog.n_in), (self.n_streams,)) or self.prog.n_in == 0, "x: wrong shape, dtype, layout or device for this call")
        _require(tuple(out.shape) == (T, self.n_streams, self.prog.n_out) and (out.is_contiguous() if is_torch else out.flags.c_contiguous), "out: wrong shape, dtype, layout or device for this call")
        want_dt = (torch.float64 if out_f64 else torch.float32) if is_torch else (np.float64 if out_f64 else np.float32)
        _require(out.dtype == want_dt, (out.dtype, want_dt))
        fn = C.lib.fz_bank_process_host_f64 if out_f64 else C.lib.fz_bank_process_host
        C.check(fn(self._h, xp if self.prog.n_in else None, op, T))
        return out

    def process_host_pcm16(self, x, out=None):
        """process_host for a caller that holds interleaved 16-bit PCM: int16 frames [T, n_streams, n_in] (or [T, n_streams]) in,
        int16 frames [T, n_streams, n_out] out -- numpy arrays or CPU torch tensors, half the PCIe bytes of process_host each way;
        the conversion rule of run_block_pcm16."""
        import numpy as np

        is_torch = hasattr(x, "data_ptr")
        T = int(x.shape[0])
        if is_torch:
            import torch
            _require(x.dtype == torch.int16 and x.is_contiguous() and not x.is_cuda, "x: wrong shape, dtype, layout or device for this call")
            if out is None:
                out = torch.empty((T, self.n_streams, self.prog.n_out), dtype=torch.int16, pin_memory=x.is_pinned())
            xp, op = x.data_ptr(), out.data_ptr()
        else:
            _require(np.asarray(x).dtype == np.int16, "x: int16 frames expected")
            x = np.ascontiguousarray(x)
            if out is None:
                out = np.empty((T, self.n_streams, self.prog.n_out), np.int16)
            xp, op = x.ctypes.data, out.ctypes.data
        _require(tuple(x.shape[1:]) in ((self.n_streams, self.prog.n_in), (self.n_streams,)) or self.prog.n_in == 0, "x: wrong shape, dtype, layout or device for this call")
        _require(tuple(out.shape) == (T, self.n_streams, self.prog.n_out) and (out.is_contiguous() if is_torch else out.flags.c_contiguous), "out: wrong shape, dtype, layout or device for this call")
        _require((out.dtype == torch.int16) if is_torch else (out.dtype == np.int16), "out: int16 frames expected")
        _require(x.ndim == 3 or self.prog.n_in <= 1, "x: [T, n_streams] only for one input wire")
        C.check(C.lib.fz_bank_process_host_pcm16(self._h, xp if self.prog.n_in else None, op, T))
        return out

    def process_pcm16_stream_major(self, x, out=None, out_dtype=None, row0=0, n_samples=None):
        """Program.run_block_pcm16_stream_major on the bank's state and per-stream coefficients (fz_bank_process_pcm16_stream_major):
        x CUDA int16 or float32 [n_streams, rows, n_in] (or [n_streams, rows]); returns out."""
        import torch

        if x.dim() == 2:
            x = x.unsqueeze(-1)
        it = Program._frame_type(x.dtype, "x")
        _require(x.is_cuda and x.dim() == 3 and x.is_contiguous() and x.shape[-1] == _bi.max(self.prog.n_in, 1),
                 "x: wrong shape, dtype, layout or device for this call")
        ns, rows, _ = x.shape
        if ns != self.n_streams:
            raise FlowzError(C.FZ_E_INVALID, f"buffers hold {ns} streams, the bank {self.n_streams}")
        row0 = int(row0)
        T = rows - row0 if n_samples is None else int(n_samples)
        _require(row0 >= 0 and T >= 0, "row0 / n_samples: a window inside the buffers")
        ot = Program._frame_type(x.dtype if out_dtype is None else out_dtype, "out_dtype")
        odt = torch.int16 if ot == C.FZ_FRAMES_I16 else torch.float32
        if out is None:
            out = torch.zeros((ns, rows, self.prog.n_out), dtype=odt, device=x.device)
        _check_dev(out, (ns, rows, self.prog.n_out), "out", odt)
        C.check(C.lib.fz_bank_process_pcm16_stream_major(self._h, x.data_ptr() if self.prog.n_in else None,
                                                         out.data_ptr() if self.prog.n_out else None, rows, row0, T, it, ot,
                                                         torch.cuda.current_stream().cuda_stream))
        return out

    def process_host_pcm16_stream_major(self, x, out=None):
        """process_host_stream_major for a caller that holds [batch, time] 16-bit PCM: int16 buffers [n_streams, T, n_in] (or
        [n_streams, T]) in, int16 [n_streams, T, n_out] out -- numpy arrays or CPU torch tensors, any T, half the PCIe bytes of
        process_host_stream_major each way; the conversion rule of run_block_pcm16."""
        import numpy as np

        is_torch = hasattr(x, "data_ptr")
        T = int(x.shape[1])
        if is_torch:
            import torch
            _require(x.dtype == torch.int16 and x.is_contiguous() and not x.is_cuda, "x: wrong shape, dtype, layout or device for this call")
            if out is None:
                out = torch.empty((self.n_streams, T, self.prog.n_out), dtype=torch.int16, pin_memory=x.is_pinned())
            xp, op = x.data_ptr(), out.data_ptr()
        else:
            _require(np.asarray(x).dtype == np.int16, "x: int16 buffers expected")
            x = np.ascontiguousarray(x)
            if out is None:
                out = np.empty((self.n_streams, T, self.prog.n_out), np.int16)
            xp, op = x.ctypes.data, out.ctypes.data
        _require(tuple(x.shape) in ((self.n_streams, T, _bi.max(self.prog.n_in, 1)), (self.n_streams, T)), "x: wrong shape, dtype, layout or device for this call")
        _require(x.ndim == 3 or self.prog.n_in <= 1, "x: [n_streams, T] only for one input wire")
        _require(tuple(out.shape) == (self.n_streams, T, self.prog.n_out) and (out.is_contiguous() if is_torch else out.flags.c_contiguous), "out: wrong shape, dtype, layout or device for this call")
        _require((out.dtype == torch.int16) if is_torch else (out.dtype == np.int16), "out: int16 buffers expected")
        C.check(C.lib.fz_bank_process_host_pcm16_stream_major(self._h, xp if self.prog.n_in else None, op, T))
        return out


Program.bank = lambda self, n_streams: Bank(self, n_streams)


def to_tiled(x, tile_streams: int):
    """time-major [T, n_streams, w] -> stream-tiled [n_tiles, T, tile_streams, w] (torch or numpy)."""
    T, ns, w = x.shape
    _require(ns % tile_streams == 0, "the stream count must be a multiple of tile_streams")
    y = x.reshape(T, ns // tile_streams, tile_streams, w)
    y = y.permute(1, 0, 2, 3).contiguous() if hasattr(y, "permute") else y.transpose(1, 0, 2, 3).copy()
    return y


def from_tiled(y):
    """stream-tiled [n_tiles, T, tile_streams, w] -> time-major [T, n_streams, w]."""
    n_tiles, T, tile, w = y.shape
    z = y.permute(1, 0, 2, 3) if hasattr(y, "permute") else y.transpose(1, 0, 2, 3)
    return z.reshape(T, n_tiles * tile, w)


def compile(expr, typed: bool = False, in_dtypes: Optional[Sequence[str]] = None) -> Program:  # noqa: A001  (mirrors flowz::compile)
    """typed / in_dtypes: fz_compile_typed -- every wire keeps its C++ type through inputs, state and outputs (ResultType,
    flowz.hpp:585-644); frames then hold 'f64' and 'cf32' wires in two float slots (see pack_typed / unpack_typed)."""
    return Program(expr, typed, in_dtypes)


def pack_typed(wires, dtypes):
    """numpy helper: per-wire arrays [T, n_streams] (float32 / float64 / complex64 / complex128) -> float32 frames [T, n_streams, slots]
    as a typed program reads them."""
    import numpy as np

    cols = []
    for w, dt in zip(wires, dtypes):
        if dt == "f32":
            cols.append(np.asarray(w, np.float32)[..., None])
        elif dt == "f64":
            cols.append(np.ascontiguousarray(np.asarray(w, np.float64)).view(np.float32).reshape(np.shape(w) + (2,)))
        elif dt == "cf64":
            cols.append(np.ascontiguousarray(np.asarray(w, np.complex128)).view(np.float32).reshape(np.shape(w) + (4,)))
        else:
            cols.append(np.ascontiguousarray(np.asarray(w, np.complex64)).view(np.float32).reshape(np.shape(w) + (2,)))
    return np.ascontiguousarray(np.concatenate(cols, axis=-1))


def unpack_typed(frames, dtypes):
    """inverse of pack_typed: float32 frames [T, n_streams, slots] -> list of per-wire arrays in their own dtype"""
    import numpy as np

    frames = np.ascontiguousarray(frames, np.float32)
    out, k = [], 0
    for dt in dtypes:
        if dt == "f32":
            out.append(frames[..., k].copy())
            k += 1
        elif dt == "cf64":
            quad = np.ascontiguousarray(frames[..., k:k + 4])
            out.append(quad.view(np.complex128)[..., 0])
            k += 4
        else:
            pair = np.ascontiguousarray(frames[..., k:k + 2])
            out.append(pair.view(np.float64 if dt == "f64" else np.complex64)[..., 0])
            k += 2
    return out


def manifest_build(path: str, workers: int = 0) -> dict:
    """Replay a kernel manifest (FLOWZ_HIP_MANIFEST=<file> records one while a process runs; *.gz is unpacked first): build, in `workers`
    parallel compiler processes and without a GPU, every kernel of it the kernel cache lacks.  Returns the counts."""
    import gzip
    import os
    import tempfile

    workers = workers or _bi.max(1, len(os.sched_getaffinity(0)))
    counts = (ctypes.c_uint32 * 4)()
    if path.endswith(".gz"):
        with tempfile.NamedTemporaryFile(suffix=".fzm") as tmp:
            tmp.write(gzip.open(path, "rb").read())
            tmp.flush()
            C.check(C.lib.fz_manifest_build(tmp.name.encode(), workers, counts))
    else:
        C.check(C.lib.fz_manifest_build(path.encode(), workers, counts))
    return dict(zip(("records", "at_hand", "built", "failed"), (int(c) for c in counts)))


def device_count() -> int:
    return C.lib.fz_device_count()


def synth_fill(dst, seed: int, stream0: int = 0, t0: int = 0):
    """Fill CUDA tensor dst with the deterministic hash noise: time-major [T, n_streams, n_wires]
    or stream-tiled [n_tiles, T, tile_streams, n_wires] (same values, tiled placement)."""
    import torch

    if dst.dim() == 4:
        n_tiles, T, tile, nw = dst.shape
        ns = n_tiles * tile
    else:
        T, ns, nw = dst.shape
        tile = 0
    _require(dst.is_cuda and dst.dtype == torch.float32 and dst.is_contiguous(), "dst: wrong shape, dtype, layout or device for this call")
    C.check(C.lib.fz_synth_fill(dst.data_ptr(), ns, T, nw, int(seed), int(stream0), int(t0), int(tile),
                                torch.cuda.current_stream().cuda_stream))
    return dst


def rbj_lowpass(freq, q, sample_rate: float, raw6=None, df1=None):
    """Per-stream RBJ low-pass coefficients on the device (reactive_filter_coeff.cpp:38-58).
    freq, q: CUDA float32 [n]; raw6: [6, n] (a0 a1 a2 b0 b1 b2) and/or df1: [5, n] rows
    (b0/a0 b1/a0 b2/a0 -a1/a0 -a2/a0), e.g. a slice of a `params` buffer."""
    import torch

    n = freq.numel()
    _require(freq.is_cuda and q.is_cuda and q.numel() == n and freq.dtype == q.dtype == torch.float32, "freq: wrong shape, dtype, layout or device for this call")
    for t, rows in ((raw6, 6), (df1, 5)):
        _require(t is None or (t.is_cuda and t.is_contiguous() and tuple(t.shape) == (rows, n)), "t: wrong shape, dtype, layout or device for this call")
    C.check(C.lib.fz_rbj_lowpass(freq.data_ptr(), q.data_ptr(), float(sample_rate), n,
                                 raw6.data_ptr() if raw6 is not None else None,
                                 df1.data_ptr() if df1 is not None else None,
                                 torch.cuda.current_stream().cuda_stream))


def frames_from_stream_major(x, tile_streams: int = 0, out=None):
    """x: CUDA float32 [n_streams, n_samples, n_wires] (one contiguous buffer per stream, as the reference's
    closures consume them) -> frames for run_block: [n_samples, n_streams, n_wires], or stream-tiled
    [n_tiles, n_samples, tile_streams, n_wires].  One device pass (fz_transpose_frames)."""
    import torch

    if x.dim() == 2:
        x = x.unsqueeze(-1)
    ns, T, w = x.shape
    _check_frames(x, x.shape[-1])
    tile = tile_streams if tile_streams and tile_streams < ns else 0
    shape = (ns // tile, T, tile, w) if tile else (T, ns, w)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=x.device)
    _require(tuple(out.shape) == shape and out.is_contiguous(), "out: wrong shape, dtype, layout or device for this call")
    C.check(C.lib.fz_transpose_frames(x.data_ptr(), out.data_ptr(), ns, T, w, tile, 0, torch.cuda.current_stream().cuda_stream))
    return out


def frames_to_stream_major(y, out=None):
    """frames ([n_samples, n_streams, w] or stream-tiled [n_tiles, n_samples, tile, w]) -> [n_streams, n_samples, w]."""
    import torch

    _require(y.is_cuda and y.dtype == torch.float32 and y.is_contiguous(), "y: wrong shape, dtype, layout or device for this call")
    if y.dim() == 4:
        n_tiles, T, tile, w = y.shape
        ns = n_tiles * tile
    else:
        T, ns, w = y.shape
        tile = 0
    if out is None:
        out = torch.empty((ns, T, w), dtype=torch.float32, device=y.device)
    _require(tuple(out.shape) == (ns, T, w) and out.is_contiguous(), "out: wrong shape, dtype, layout or device for this call")
    C.check(C.lib.fz_transpose_frames(y.data_ptr(), out.data_ptr(), ns, T, w, tile, 1, torch.cuda.current_stream().cuda_stream))
    return out


def copy_probe(src, dst):
    import torch

    _require(src.is_cuda and dst.is_cuda and src.numel() == dst.numel() and src.numel() % 4 == 0, "src: wrong shape, dtype, layout or device for this call")
    C.check(C.lib.fz_copy_probe(src.data_ptr(), dst.data_ptr(), src.numel(),
                                torch.cuda.current_stream().cuda_stream))
