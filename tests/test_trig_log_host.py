"""sin, cos and log as flow-graph functions, on the host: the C ABI values, lowering, refusals, recipes, the workloads against their
recurrences, the hiprtc builds (no scratch, no library call, no hardware approximation), accuracy of the numpy restatement
(tests/fn_ref_trig.py, which the GPU tests hold the kernels to bit for bit) on a sample, the cells' kernel names, the backward's
restatement against float64 autograd, and the kernel manifest of the GPU tests."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import adjoint_ref as A
import adjoint_ref_trig as AT
import fn_ref as R
import fn_ref_trig as RT
import grad_graphs as GG
import trig_cells as TC
from zignal_amd import flowz as F
from zignal_amd import workloads as W

F32, F64 = np.float32, np.float64
HERE = os.path.dirname(os.path.abspath(__file__))
_1, _2 = F.placeholder(1), F.placeholder(2)
# the maxima include/flowz_hip.h states (ulps of the correctly rounded result)
LOGF_MAX, LOGD_MAX, SINCOS_MAX = 0.840, 0.826, 0.500001


def kinds(prog):
    return [k for k, *_ in prog.ir()]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == F32 else np.uint64)


# ---- C ABI, lowering -----------------------------------------------------------------------------------------------------------
def test_symbols_and_enum_values():
    C = F.C
    assert (C.FZ_OP_SIN, C.FZ_OP_COS, C.FZ_OP_LOG) == (21, 22, 23)
    assert (C.FZ_IR_SIN, C.FZ_IR_COS, C.FZ_IR_LOG) == (27, 28, 29) and C.FZ_IR_MAX == 26
    assert [C.IR_KINDS[k] for k in (27, 28, 29)] == ["sin", "cos", "log"]
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "flowz_hip.h")).read()
    for text in ("FZ_OP_SIN = 21, FZ_OP_COS = 22, FZ_OP_LOG = 23", "FZ_IR_SIN = 27, FZ_IR_COS = 28", "FZ_IR_LOG = 29", "FZ_IR_MAX = 26"):
        assert text in hdr, text
    assert F._FN1["sin"] == 21 and F._FN1["cos"] == 22 and F._FN1["log"] == 23


def test_lowering_kinds_dtypes_n_ops_and_sharing():
    p = F.compile(F.sin(_1) + F.sin(_1) * F.cos(_1) + F.log(_2[1]) + F.log(_2[1]))
    k = kinds(p)
    assert k.count("sin") == 1 and k.count("cos") == 1 and k.count("log") == 1 and set(p.ir_dtypes()) == {"f32"}
    assert p.n_in == 2 and p.n_out == 1 and p.n_ops == 7       # sin (shared), cos, mul, add, log (shared), add, add
    d = F.compile(F.log(F.lit64(0.5) * _1))
    assert dict(zip(kinds(d), d.ir_dtypes()))["log"] == "f64"
    t = F.compile(F.log(_1), in_dtypes=["f64"])
    assert dict(zip(kinds(t), t.ir_dtypes()))["log"] == "f64"
    assert F.sin(_2).ins == 2 and F.log(_2[3]).ins == 2 and F.cos(_1).outs == 1
    assert not F.compile(F.seq(F.sin(_1), F.sin(_1))).stage_packable
    e = ("add", ("sin", ("in", 1)), ("mul", ("cos", ("in", 1)), ("log", ("lit", 0.5))))
    assert sorted(kinds(F.compile(F.from_sexpr(e)))) == sorted(["input", "sin", "cos", "const", "log", "mul", "add"])


def test_refusals():
    z = F.litc(0.5, 0.25) * _1
    for fn, word in ((F.sin, "complex"), (F.cos, "complex"), (F.log, "complex")):
        with pytest.raises(F.FlowzError) as e:
            F.compile(fn(z))
        assert e.value.code == F.C.FZ_E_UNSUPPORTED and word in str(e.value)
    for fn in (F.sin, F.cos):
        with pytest.raises(F.FlowzError) as e:
            F.compile(fn(F.lit64(0.5) * _1))
        assert e.value.code == F.C.FZ_E_UNSUPPORTED and "double" in str(e.value)
        with pytest.raises(F.FlowzError) as e:
            F.compile(fn(_1), in_dtypes=["f64"])
        assert e.value.code == F.C.FZ_E_UNSUPPORTED and "double" in str(e.value)
    for op in (F.C.FZ_OP_SIN, F.C.FZ_OP_COS, F.C.FZ_OP_LOG):
        assert F.C.lib.fz_arith(op, F.chan(_1, _1)._h, None) is None
    assert F.C.lib.fz_arith(24, _1._h, None) is None             # (no opcode behind FZ_OP_LOG)


def test_recipe_round_trip():
    C = F.C
    e = F.from_sexpr(W.log_compressor()) + F.sin(_1) * F.cos(F.tanh(_1)) + F.log(F.lit64(2.0) + _1 * _1)
    n = C.lib.fz_expr_recipe(e._h, None, 0)
    buf = ctypes.create_string_buffer(n + 1)
    C.lib.fz_expr_recipe(e._h, buf, n + 1)
    text = buf.value.decode()
    assert "\nG 21 " in text and "\nG 22 " in text and "\nG 23 " in text and "\nG 18 " in text
    back = F.Expr(C.lib.fz_expr_from_recipe(buf.value))
    a, b = F.compile(e), F.compile(back)
    assert a.ir() == b.ir() and a.ir_dtypes() == b.ir_dtypes()
    for bad in (b"P 1\nG 19 0\n", b"P 1\nG 20 0\n", b"P 1\nG 24 0\n", b"P 1\nG 14 0\n"):   # min / max are "A" lines; 24 and 14 are no functions
        assert C.lib.fz_expr_from_recipe(bad) is None, bad


@pytest.mark.parametrize("name", TC.WORKLOADS)
def test_workloads_match_their_recurrences_on_the_ir(name):
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((48, 16, 1)) * 2).astype(F32)
    inc = rng.uniform(0.001, 3.0, (1, 16)).astype(F32)
    prog = TC.graph(name)
    y, _ = R.run_ir(prog, x, params=inc if prog.n_param else None)
    assert np.array_equal(bits(y[:, :, 0]), bits(TC.recurrence(name, x, inc)))
    for g in ("pm_operator", "wavefolder", "log_compressor"):
        assert g not in W.BASELINE_GRAPHS


# ---- kernels -------------------------------------------------------------------------------------------------------------------
FORBIDDEN = re.compile(r"__ocml_|__builtin_\w*(sin|cos|exp2|log|rcp|rsq|fma)|\bsinf?\(|\bcosf?\(|\blogf?\(|\bsincosf?\(")


@pytest.mark.parametrize("P", [1, 2, 4])
def test_hiprtc_builds_use_no_scratch_no_library_calls_no_hardware_functions(P, tmp_path, monkeypatch):
    monkeypatch.setenv("FLOWZ_HIP_CACHE", str(tmp_path))
    g = F.sin(_1) + F.cos(_1) * F.log(abs(_1))
    d = F.log(F.lit64(0.5) * _1)
    for e in (g, d):
        p = F.compile(e)
        v = F.make_variant(P, 8)
        src = p.source(v)
        body = src.split("// ==== fz_graph_body.h ====")[1].split("// ==== ")[0]
        body = re.sub(r"//[^\n]*", "", body)
        assert "fz_log" in body and not FORBIDDEN.search(body), FORBIDDEN.search(body)
        r = p.kernel_resources(v, as_launched=False)
        assert r["scratch_bytes"] == 0 and r["vgpr_spills"] == 0, r
    dis = ""
    for f in tmp_path.rglob("*.hsaco"):
        dis += subprocess.check_output(["/opt/rocm/lib/llvm/bin/llvm-objdump", "-d", str(f)], text=True)
    # (v_fma_* does appear: the compiler's expansion of the correctly rounded division; the source has no contraction, -ffp-contract=off)
    assert dis and not re.search(r"v_(sin|cos|log|exp)_f32", dis)


def test_each_function_is_written_only_into_graphs_that_use_it():
    src = F.compile(F.from_sexpr(W.moog_ladder())).source(F.make_variant(2, 8))
    assert "fz_sin" not in src and "fz_cos" not in src and "fz_log" not in src and "FZ_CVT" not in src
    s = F.compile(F.sin(_1)).source(F.make_variant(1, 8))
    assert "fz_sin(" in s and "fz_cos" not in s and "fz_log" not in s
    lg = F.compile(F.log(_1)).source(F.make_variant(1, 8))
    assert "fz_log(" in lg and "fz_sincos_core" not in lg
    assert "fz_cos(" in F.compile(F.sin(_1)).grad_source()       # the adjoint rule of sin calls cos


def test_cells_resolve_to_their_bodies():
    for c in TC.CELLS:
        assert TC.cell_name(TC.graph(c[1]), c) == c[7], c[0]


# ---- accuracy of the restatement ---------------------------------------------------------------------------------------------
def ulps(y, ref, T):
    rf = ref.astype(T)
    fin = np.isfinite(rf)
    assert np.array_equal(np.isnan(y), np.isnan(rf)) and np.array_equal(y[~fin & ~np.isnan(rf)], rf[~fin & ~np.isnan(rf)])
    return np.abs(y[fin].astype(F64) - ref[fin]) / np.spacing(np.abs(rf[fin])).astype(F64)


def test_accuracy_on_the_sample_stays_within_the_stated_maxima():
    x = TC.accuracy_sample()
    assert x.size >= 1 << 18
    with np.errstate(all="ignore"):
        x64 = x.astype(F64)
        e = ulps(RT.log(x), np.log(x64), F32)
        print("log float32: %.4f ulp" % e.max())
        assert e.max() <= LOGF_MAX
        dom = np.abs(x) < F32(2.0 ** 20)
        for fn, ref in ((RT.sin, np.sin), (RT.cos, np.cos)):
            e = ulps(fn(x), np.where(dom, ref(x64), np.nan), F32)
            print("%s float32: %.7f ulp" % (fn.__name__, e.max()))
            assert e.max() <= SINCOS_MAX
    assert np.array_equal(bits(RT.sin(-x))[dom], bits(-RT.sin(x))[dom]) and np.array_equal(bits(RT.cos(-x))[dom], bits(RT.cos(x))[dom])
    assert np.all(np.abs(RT.sin(x)[dom]) <= 1) and np.all(np.abs(RT.cos(x)[dom]) <= 1)
    tiny = np.abs(x) < F32(2.0 ** -13)
    assert tiny.sum() > 1000 and np.array_equal(bits(RT.sin(x))[tiny], bits(x)[tiny])


def test_special_values():
    inf, nan = F32(np.inf), F32(np.nan)
    for T in (F32, F64):
        y = RT.log(np.array([0.0, -0.0, 1.0, np.inf, -1.0, -np.inf, np.nan], T))
        assert y[0] == -np.inf and y[1] == -np.inf and y[2] == 0 and not np.signbit(y[2]) and y[3] == np.inf and np.isnan(y[4:]).all()
    s = RT.sin(np.array([0.0, -0.0, 2.0 ** 20, -2.0 ** 20, inf, -inf, nan], F32))
    c = RT.cos(np.array([0.0, -0.0, 2.0 ** 20, -2.0 ** 20, inf, -inf, nan], F32))
    assert s[0] == 0 and not np.signbit(s[0]) and s[1] == 0 and np.signbit(s[1]) and c[0] == 1 and c[1] == 1
    assert np.isnan(s[2:]).all() and np.isnan(c[2:]).all()
    below = np.nextafter(F32(2.0 ** 20), F32(0))
    assert np.isfinite(RT.sin(np.array([below, -below], F32))).all()


def test_double_log_against_mpmath_on_a_stratified_sample():
    """every 8th of the tool's own stratified inputs in the chunks of the subnormals, of [2^-15, 2^1) and of the largest exponents"""
    pytest.importorskip("mpmath")
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
    import graph_functions_exhaustive as GE
    x = np.concatenate([GE.double_log_inputs(k)[::8] for k in (0, 63, 127)] + [[1.0, np.nextafter(1.0, 0), np.nextafter(1.0, 2), 5e-324]])
    worst = GE.double_log_worst(x)
    print("log float64: %.4f ulp" % worst)
    assert worst <= LOGD_MAX


def test_float_sine_and_cosine_equal_the_c_checker():
    from oracle import coracle
    if not hasattr(coracle, "sincos_f32"):
        pytest.skip("oracle/coracle.py exposes no sine / cosine")
    x = np.random.default_rng(3).uniform(-1000, 1000, 1 << 16).astype(F32)
    x = x[x != 0]
    sn, cs = coracle.sincos_f32(x)
    assert np.array_equal(bits(RT.sin(x)), bits(np.asarray(sn, F32))) and np.array_equal(bits(RT.cos(x)), bits(np.asarray(cs, F32)))


# ---- backward ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(GG.SUPPORTED))
def test_extended_restatement_gives_the_bits_of_adjoint_ref_on_graphs_without_the_new_kinds(name):
    from grad_harness import make_inputs, same
    p = F.compile(F.from_sexpr(GG.SUPPORTED[name]()))
    x, s0, par, yb, sb, ap, ac = make_inputs(p, name, 5, 7, 31)
    a, b = A.grad(p, x, yb, s0, par, sb, ap, ac), AT.grad(p, x, yb, s0, par, sb, ap, ac)
    for k in a:
        assert same(a[k], b[k]), (name, k)


GRAD_NAMES = ("all3",) + TC.WORKLOADS


def smooth_inputs(p, ns, T, seed):
    """inputs away from kinks that keep log's operand >= 0.05: |x| in [0.1, 0.9], a non-negative state"""
    rng = np.random.default_rng(seed)
    x = (rng.uniform(0.1, 0.9, (T, ns, p.n_in)) * rng.choice([-1.0, 1.0], (T, ns, p.n_in))).astype(F32)
    s0 = rng.uniform(0.1, 0.5, (p.n_state, ns)).astype(F32)
    par = rng.uniform(0.01, 0.5, (p.n_param, ns)).astype(F32) if p.n_param else None
    return x, s0, par, rng.standard_normal((T, ns, p.n_out)).astype(F32), rng.standard_normal((p.n_state, ns)).astype(F32)


@pytest.mark.parametrize("name", GRAD_NAMES)
def test_grad_check_accepts_and_the_restatement_follows_float64_autograd(name):
    pytest.importorskip("torch")
    p = TC.graph(name)
    assert p.grad_supported(), p.grad_unsupported_reason()
    x, s0, par, yb, sb = smooth_inputs(p, 6, 24, 41)
    got = AT.grad(p, x, yb, s0, par, sb)
    want = AT.torch_grad(p, x, yb, s0, par, sb)
    worst = max(AT.rel_err(got[k], want[k]) for k in got if np.asarray(want[k]).size)
    print(f"{name}: worst relative error against float64 autograd {worst:.3e}")
    assert worst <= 1e-4


def test_adjoint_kernels_are_pinned_and_free_of_scratch():
    pins = json.load(open(TC.PINS_FILE))
    got = {}
    for name in GRAD_NAMES:
        p = TC.graph(name)
        for sm in (False, True):
            r = p.grad_resources(0, stream_major=sm)
            assert r["scratch_bytes"] == 0 and r["vgpr_spills"] == 0, (name, sm, r)
            got[f"{name}/{'sm' if sm else 'tm'}"] = p.grad_kernel_symbol(0, stream_major=sm)
    assert got == pins, got


# ---- the manifest of the GPU tests' kernels -----------------------------------------------------------------------------------
def test_the_manifest_builds_every_kernel_of_the_gpu_tests(tmp_path):
    code = ("import sys, json\nsys.path.insert(0, %r)\nfrom zignal_amd import flowz as F\nprint(json.dumps(F.manifest_build(%r)))\n"
            % (os.path.dirname(HERE), TC.MANIFEST))
    env = {k: v for k, v in os.environ.items() if k != "FLOWZ_HIP_MANIFEST"}
    out = subprocess.check_output([sys.executable, "-c", code], env=dict(env, FLOWZ_HIP_CACHE=str(tmp_path)), cwd=os.path.dirname(HERE), text=True)
    r = json.loads(out.splitlines()[-1])
    assert r["failed"] == 0 and r["at_hand"] + r["built"] == r["records"] >= len(TC.CELLS), r
