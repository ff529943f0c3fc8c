"""Graph functions (abs, sqrt, exp, tanh, min, max) without a GPU: the accuracy of the numpy restatement the GPU tests hold the kernels to,
the lowering, recipes, the generated source, hiprtc builds -- and that no kernel of a graph without functions changed."""
import json
import os
import re
import subprocess

import mpmath
import numpy as np
import pytest

import fn_ref as R
import fn_pins
from test_cpp_edsl import build as build_cpp
from zignal_amd import flowz as F
from zignal_amd import workloads as W

HERE = os.path.dirname(os.path.abspath(__file__))
F32, F64 = np.float32, np.float64
LD = np.longdouble
_1, _2 = F.placeholder(1), F.placeholder(2)


def stratified(T, n, lo_exp, hi_exp, seed):
    """n inputs spread evenly over the binades 2^lo_exp .. 2^hi_exp, both signs, random mantissas"""
    rng = np.random.default_rng(seed)
    e = rng.integers(lo_exp, hi_exp, n)
    m = rng.random(n) + 1.0
    s = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    return (s * np.ldexp(m, e)).astype(T)


def ulp_err(got, want_ld, T):
    """|got - exact| in ulps of the correctly rounded result (subnormal spacing below the normal range)"""
    ref = want_ld.astype(T)
    sp = np.spacing(np.abs(ref).astype(T)).astype(LD)
    return np.abs(got.astype(LD) - want_ld) / sp


@pytest.mark.parametrize("T", [F32, F64])
def test_exp_within_two_ulp_on_2_22_stratified_inputs(T):
    lim = 88.0 if T == F32 else 709.0
    x = stratified(T, 1 << 22, -30, 10, 1)
    x = x[np.abs(x) < lim]
    u = ulp_err(R.exp(x), np.exp(x.astype(LD)), T)
    assert u.max() <= 2.0, (u.max(), x[np.argmax(u)])


@pytest.mark.parametrize("T", [F32, F64])
def test_tanh_within_two_ulp_odd_and_bounded_on_2_22_stratified_inputs(T):
    x = stratified(T, 1 << 22, -30 if T == F32 else -60, 6, 2)
    y = R.tanh(x)
    u = ulp_err(y, np.tanh(x.astype(LD)), T)
    assert u.max() <= 2.0, (u.max(), x[np.argmax(u)])
    assert np.array_equal(R.tanh(-x).view(np.uint8), (-y).view(np.uint8))            # odd bit for bit
    assert np.all(np.abs(y) <= 1)


@pytest.mark.parametrize("T", [F32, F64])
def test_special_values_and_binade_edges_against_mpmath(T):
    mpmath.mp.prec = 128
    fi = np.finfo(T)
    edges = [T(0), -T(0), fi.tiny, fi.smallest_subnormal, T(1), T(0.5), T(0.55), T(2.0) ** -12]
    for e in range(int(np.log2(fi.smallest_subnormal)), fi.maxexp):          # every binade, subnormal ones included
        b = T(2.0) ** e
        edges += [b, np.nextafter(b, T(0)), np.nextafter(b, T(np.inf))]
    xs = np.array(edges + [-v for v in edges], T)
    for fn, mfn, lim in ((R.exp, mpmath.exp, 88.7 if T == F32 else 709.7), (R.tanh, mpmath.tanh, np.inf)):
        got = fn(xs)
        for x, g in zip(xs, got):
            if abs(float(x)) > lim:
                continue
            want = mfn(mpmath.mpf(float(x)))
            r = T(float(want))
            sp = float(np.spacing(np.abs(r))) if r != 0 else float(fi.smallest_subnormal)
            assert abs(mpmath.mpf(float(g)) - want) <= 2 * sp, (fn.__name__, x, g, want)
    # exp: the specials; overflow exactly where the correctly rounded result overflows; gradual underflow
    xmax = T(88.72283172607422) if T == F32 else T(709.782712893383973096)
    e = R.exp(np.array([0, -0.0, -np.inf, np.inf, np.nan, xmax, np.nextafter(xmax, T(np.inf))], T))
    assert e[0] == 1 and e[1] == 1 and e[2] == 0 and not np.signbit(e[2]) and e[3] == np.inf and np.isnan(e[4])
    assert np.isfinite(e[5]) and e[6] == np.inf
    sub = R.exp(np.array([-100.0 if T == F32 else -740.0], T))[0]
    assert 0 < sub < fi.tiny
    # tanh: +-0 kept, +-1 at the ends and past saturation, x for tiny x
    t = R.tanh(np.array([0.0, -0.0, np.inf, -np.inf, 30.0, -30.0, 1e-30, -1e-30, fi.smallest_subnormal, np.nan], T))
    assert t[0] == 0 and not np.signbit(t[0]) and t[1] == 0 and np.signbit(t[1])
    assert t[2] == 1 and t[3] == -1 and t[4] == 1 and t[5] == -1
    assert t[6] == T(1e-30) and t[7] == T(-1e-30) and t[8] == fi.smallest_subnormal and np.isnan(t[9])


def test_min_max_abs_sqrt_follow_std():
    nan = F32(np.nan)
    a = np.array([nan, 1, 0.0, -0.0, 2, -1], F32)
    b = np.array([1, nan, -0.0, 0.0, 1, -3], F32)
    assert np.isnan(R.fmin(a, b)[0]) and R.fmin(a, b)[1] == 1
    assert np.signbit(R.fmin(a, b)[2]) == np.signbit(a[2]) and np.signbit(R.fmin(a, b)[3]) == np.signbit(a[3])   # equal: a
    assert list(R.fmin(a, b)[4:]) == [1, -3] and list(R.fmax(a, b)[4:]) == [2, -1]
    assert np.isnan(R.fmax(a, b)[0]) and R.fmax(a, b)[1] == 1
    assert np.signbit(R.fabs(np.array([-0.0], F32)))[0] == False and np.isnan(R.sqrt(np.array([-1.0], F32)))[0]   # noqa: E712
    assert np.signbit(R.sqrt(np.array([-0.0], F32)))[0]


# ---- lowering ------------------------------------------------------------------------------------------------------------------
def kinds(prog):
    return [k for k, *_ in prog.ir()]


def test_lowering_kinds_dtypes_arity_and_sharing():
    p = F.compile(F.tanh(_1) + F.tanh(_1) * F.min(_1, 0.5) + F.max(-1.0, F.sqrt(abs(_1))) + F.exp(_2[1]))
    k = kinds(p)
    assert k.count("tanh") == 1 and k.count("min") == 1 and k.count("max") == 1 and k.count("sqrt") == 1 and k.count("abs") == 1
    assert k.count("exp") == 1 and p.n_in == 2 and p.n_out == 1 and set(p.ir_dtypes()) == {"f32"}
    assert p.n_ops == 10                                       # tanh (shared), min, mul, add, abs, sqrt, max, add, exp, add
    d = F.compile(F.tanh(F.lit64(0.5) * _1) + F.min(_1, F.lit64(0.25)))
    dt = dict(zip(kinds(d), d.ir_dtypes()))
    assert dt["tanh"] == "f64" and dt["min"] == "f64"
    t = F.compile(F.exp(_1), in_dtypes=["f64"])                 # a typed double wire
    assert dict(zip(kinds(t), t.ir_dtypes()))["exp"] == "f64"
    assert F.exp(_2).ins == 2 and F.min(_1, _2[3]).ins == 2


def test_lowering_refuses_complex_operands_and_multi_wire_operands():
    z = F.litc(0.5, 0.25) * _1
    with pytest.raises(F.FlowzError) as e:
        F.compile(F.min(z, _1))
    assert e.value.code == F.C.FZ_E_GRAPH
    for fn in (F.abs, F.sqrt, F.exp, F.tanh):
        with pytest.raises(F.FlowzError) as e:
            F.compile(fn(z))
        assert e.value.code == F.C.FZ_E_UNSUPPORTED
    assert F.C.lib.fz_arith(F.C.FZ_OP_TANH, F.chan(_1, _1)._h, None) is None


def test_sexpr_keys_and_the_workloads_lower():
    e = ("add", ("tanh", ("in", 1)), ("min", ("abs", ("in", 1)), ("max", ("sqrt", ("in", 1)), ("exp", ("lit", 0.5)))))
    assert sorted(kinds(F.compile(F.from_sexpr(e)))) == sorted(["input", "tanh", "abs", "sqrt", "const", "exp", "max", "min", "add"])
    m = F.compile(F.from_sexpr(W.moog_ladder()))
    assert kinds(m).count("tanh") == 8 and m.n_param == 1 and m.n_state == 4
    for g in ("moog_ladder", "soft_clip_cascade", "envelope_follower"):
        assert g not in W.BASELINE_GRAPHS


def test_recipe_round_trip():
    """a recipe (what kernel manifests record) carries the function nodes: the expression read back lowers to the same IR"""
    import ctypes
    C = F.C
    e = F.from_sexpr(W.envelope_follower()) + F.tanh(_1) * F.min(F.exp(_1), F.sqrt(_1)) + F.max(F.lit64(2.0), _1)
    n = C.lib.fz_expr_recipe(e._h, None, 0)
    buf = ctypes.create_string_buffer(n + 1)
    C.lib.fz_expr_recipe(e._h, buf, n + 1)
    text = buf.value.decode()
    assert "\nG 15 " in text and "\nG 16 " in text and "\nG 17 " in text and "\nG 18 " in text
    assert re.search(r"\nA 19 ", text) and re.search(r"\nA 20 ", text)
    back = F.Expr(C.lib.fz_expr_from_recipe(buf.value))
    a, b = F.compile(e), F.compile(back)
    assert a.ir() == b.ir() and a.ir_dtypes() == b.ir_dtypes()
    assert C.lib.fz_expr_from_recipe(b"P 1\nG 5 0\n") is None          # (NEG is not a function opcode)


@pytest.mark.parametrize("name", ["moog_ladder", "soft_clip_cascade", "envelope_follower"])
def test_workloads_match_their_recurrences_on_the_ir(name):
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((48, 16)) * 2).astype(F32)
    g = rng.uniform(0.05, 0.7, 16).astype(F32)
    prog = F.compile(F.from_sexpr(getattr(W, name)()))
    y, _ = R.run_ir(prog, x, params=[g])
    want = {"moog_ladder": lambda: R.moog_ladder_ref(x, g, W.MOOG_RESONANCE),
            "soft_clip_cascade": lambda: R.soft_clip_cascade_ref(x, [W.SOFT_CLIP] * 4),
            "envelope_follower": lambda: R.envelope_follower_ref(x, W.ENV_ATTACK, W.ENV_RELEASE)}[name]()
    assert np.array_equal(y[:, :, 0].view(np.uint32), want.view(np.uint32))


# ---- kernels -------------------------------------------------------------------------------------------------------------------
FORBIDDEN = re.compile(r"__ocml_|__builtin_\w*(exp2|log|rcp|rsq)|\bexpf?\(|\blogf?\(|\btanhf?\(")


@pytest.mark.parametrize("P", [1, 2, 4])
def test_hiprtc_builds_use_no_scratch_no_library_calls_no_hardware_exp(P, tmp_path, monkeypatch):
    monkeypatch.setenv("FLOWZ_HIP_CACHE", str(tmp_path))
    g = F.tanh(_1) + F.min(F.max(_1, -0.5), 0.5) + F.sqrt(abs(_1)) + F.exp(_1)
    d = F.tanh(F.lit64(0.5) * _1) + F.exp(F.lit64(1.0) * _1) + F.max(F.sqrt(F.lit64(1.0) * _1), F.lit64(0.25))
    for e in (g, d):
        p = F.compile(e)
        v = F.make_variant(P, 8)
        src = p.source(v)
        body = src.split("// ==== fz_graph_body.h ====")[1].split("// ==== ")[0]        # the generated part (the skeleton is shared by all)
        body = re.sub(r"//[^\n]*", "", body)                                               # (code, not comments)
        assert "fz_tanh" in body and not FORBIDDEN.search(body), FORBIDDEN.search(body)
        r = p.kernel_resources(v, as_launched=False)
        assert r["scratch_bytes"] == 0 and r["vgpr_spills"] == 0, r
    dis = ""
    for f in tmp_path.rglob("*.hsaco"):
        dis += subprocess.check_output(["/opt/rocm/lib/llvm/bin/llvm-objdump", "-d", str(f)], text=True)
    assert dis and "v_exp_f32" not in dis and "v_log_f32" not in dis
    if P == 2:
        assert "v_pk_mul_f32" in dis and "v_pk_add_f32" in dis


def test_graphs_without_functions_get_no_function_code():
    src = F.compile(F.from_sexpr(W.df1_cascade(6))).source(F.make_variant(2, 8))
    assert "fz_tanh" not in src and "fz_vi" not in src


def test_stage_packing_and_wave_split_refuse_function_graphs():
    p = F.compile(F.from_sexpr(W.soft_clip_cascade(4)))
    assert not p.stage_packable
    for flags in (F.C.FZ_VF_STAGE_PACK, F.C.FZ_VF_WAVES(2)):
        try:
            name = p.kernel_name(F.make_variant(1, 16, 256, flags), 65536, 1024)
        except F.FlowzError as e:
            assert e.code in (F.C.FZ_E_UNSUPPORTED, F.C.FZ_E_INVALID)
            continue
        assert "s" not in name.split("b256")[1].split("f")[0]       # (stage packing dropped: no segment count in the name)


def test_moog_default_plan_uses_no_scratch():
    p = F.compile(F.from_sexpr(W.moog_ladder()))
    r = p.kernel_resources(None, 1 << 20, 4096)
    assert r["scratch_bytes"] == 0 and r["vgpr_spills"] == 0, r


# ---- nothing that existed changed ---------------------------------------------------------------------------------------------
def test_existing_graphs_keep_their_kernels_and_plans():
    """kernel_name / kernel_symbol / kernel_code_id of every graph builder at the BASELINE shapes, recorded before the functions
    were added (tests/golden/graph_pins.json): the same source, options and plan for every graph without functions"""
    want = json.load(open(os.path.join(HERE, "golden", "graph_pins.json")))
    got = fn_pins.pins()
    missing = sorted(set(want) - set(got))
    assert not missing, missing[:5]
    diff = {k: (want[k], got[k]) for k in want if want[k] != got[k]}
    assert not diff, list(diff.items())[:3]


def test_cpp_front_end_graph_functions():
    out = subprocess.run([build_cpp("test_fn_host")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all graph-function host checks passed" in out.stdout


# ---- the kernel bodies function graphs reach (tests/fn_bodies.py; run on the GPU by test_graph_functions_bodies_gpu.py) ----------
def test_body_matrix_cells_resolve_to_their_bodies():
    """every cell of the GPU matrix runs the body it is there for, and the block after its cut another one"""
    import fn_bodies as B
    for c in B.CELLS:
        prog = B.graph(c[1])
        assert B.cell_name(prog, c) == c[7], c[0]
        assert prog.kernel_name(B.variant(c[9], c[2]), c[4], c[5], c[6]) != c[7], c[0]


def test_default_plan_sends_function_graphs_to_the_matrix_bodies():
    """the library's own choice for the function graphs at full size -- among them the LDS-ring lockstep step-down (one row per chunk,
    three buffers) at 2^27 streams: every one of these bodies is a cell of the GPU matrix"""
    import fn_bodies as B
    cells = {(c[1], c[7]) for c in B.CELLS}
    for name, ns, T, tile, sm, want in B.DEFAULT_BODIES:
        prog = B.graph(name)
        assert B.default_name(prog, ns, T, tile, sm, name in B.OUT_F64) == want, (name, ns, T, tile, sm)
        if not sm:
            assert prog.kernel_name(None, ns, T, tile) == want, (name, ns, T, tile)
        assert any(w.startswith(want.rstrip("M")) for _, w in cells), want
    f64 = B.graph("f64lit")
    assert B.default_name(f64, 1 << 20, 4096, 0, False, True) == "fz_block_kernel_p4u1b1024f%dL" % (B.L | B.GS | B.P3 | B.OUT64)


@pytest.mark.parametrize("ns", [16384, 40000, 65536, 65600])
def test_flags_only_lockstep_request_resolves_to_the_frame_kernel(ns):
    """a variant that asks for the lockstep frame kernel by its flags alone gets it at every stream count -- also where the library's own
    choice is a wave-split kernel (<= 65 536 streams), which takes neither flag"""
    p = F.compile(F.from_sexpr(W.df1_cascade(6)))
    L, GS, SP = F.C.FZ_VF_LOCKSTEP, F.C.FZ_VF_GRID_SYNC, F.C.FZ_VF_STAGE_PACK
    for T in (4096, 1100):
        assert p.kernel_name(F.make_variant(0, 0, 0, L), ns, T) == "fz_block_kernel_p1u16b256s6f%d" % (L | SP)
        assert p.kernel_name(F.make_variant(0, 0, 0, L | GS), ns, T) == "fz_block_kernel_p1u16b256s6f%d" % (L | GS | SP)
    if ns <= 65536:                                            # (the library's own choice there stays the wave-split kernel)
        assert re.search(r"b\d+w\d", p.kernel_name(None, ns, 4096))


# ---- the evaluator on typed programs and modulators ---------------------------------------------------------------------------
def test_evaluator_double_lines_and_modulators_agree_with_ir_interp():
    """fn_ref.run_ir on function-free programs with double delay lines (typed) and sample-rate modulators: the bits and the state of
    tests/ir_interp.py"""
    import graphs as G
    import ir_interp
    rng = np.random.default_rng(11)
    ns, T = 24, 40
    t = F.compile(F.from_sexpr(W.df1_double()), typed=True)
    a = rng.standard_normal((T, ns)) * 2
    x = F.pack_typed([a], t.input_dtypes())
    st0 = ir_interp.run_ir(t, x[:7])[1]
    for args in ({}, {"state": st0}):
        y1, s1 = R.run_ir(t, x, **args)
        y2, s2 = ir_interp.run_ir(t, x, **args)
        assert "f64" in t.line_dtypes() and np.array_equal(y1.view(np.uint32), y2.view(np.uint32)) and np.array_equal(s1.view(np.uint32), s2.view(np.uint32))
    m = F.compile(F.from_sexpr(G.modulated_mix()))
    x = rng.standard_normal((T, ns, m.n_in)).astype(F32)
    mod = rng.uniform(-0.9, 0.9, (m.n_mod, T)).astype(F32)
    y1, s1 = R.run_ir(m, x, mod=mod)
    y2, s2 = ir_interp.run_ir(m, x, mod=mod)
    assert np.array_equal(y1.view(np.uint32), y2.view(np.uint32)) and np.array_equal(s1.view(np.uint32), s2.view(np.uint32))


def test_evaluator_typed_tanh_loop_and_double_output_frames_follow_their_equations():
    """y = tanh(0.9f * y[-1] + x) with a double input wire: a double recursion, its double output as two float words; tanh(0.5 * (x +
    x[-3])) with the double literal on float64 output frames: the double result unrounded"""
    import fn_bodies as B
    rng = np.random.default_rng(12)
    ns, T = 16, 30
    p = B.graph("typed")
    a = rng.standard_normal((T, ns)) * 3
    y, st = R.run_ir(p, F.pack_typed([a], ["f64"]))
    w, prev = np.empty((T, ns)), np.zeros(ns)
    for t in range(T):
        prev = R.tanh(F64(F32(0.9)) * prev + a[t])
        w[t] = prev
    assert np.array_equal(F.unpack_typed(y, ["f64"])[0].view(np.uint64), w.view(np.uint64))
    assert np.array_equal(st.view(np.uint64).reshape(-1), w[-1].view(np.uint64))        # (one double row: two float rows)
    p = B.graph("f64lit")
    x = (rng.standard_normal((T, ns)) * 3).astype(F32)
    y, _ = R.run_ir(p, x, out_f64=True)
    xd = np.concatenate([np.zeros((3, ns), F32), x])
    want = R.tanh(F64(0.5) * (xd[3:] + xd[:-3]).astype(F64))
    assert y.dtype == F64 and np.array_equal(y[..., 0].view(np.uint64), want.view(np.uint64))
