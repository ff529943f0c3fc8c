"""Host logic of the product (no GPU): C-ABI exports, EDSL analysis transforms, lowering.

The lowered IR is evaluated by a tests-only numpy interpreter and compared with the oracle."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import graphs as G
import workloads as W
from ir_interp import run_ir
from oracle import coracle as C
from oracle import flowz_oracle as O
from zignal_amd import _capi, flowz as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
KA = json.load(open(os.path.join(HERE, "golden", "tests_cpp_known_answers.json")))


def tup(x):
    return tuple(tup(v) for v in x) if isinstance(x, list) else x


def same(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def test_library_exports_every_declared_symbol():
    hdr = open(os.path.join(ROOT, "include", "flowz_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(fz_[a-z0-9_]+)\s*\(", hdr))
    assert len(declared) >= 35
    lib = ctypes.CDLL(_capi.LIB_PATH)
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in include/flowz_hip.h but not exported"
    assert set(_capi.EXPORTS) == declared


@pytest.mark.parametrize("case", KA["arity"], ids=lambda c: c["name"])
def test_arity_transforms_match_tests_cpp(case):
    e = F.from_sexpr(tup(case["graph"]))
    assert e.ins == case["ins"] and e.outs == case["outs"]
    if "max_input_delays" in case:
        assert list(e.max_input_delays()) == case["max_input_delays"]


@pytest.mark.parametrize("case", KA["evaluation"] + KA["readme"], ids=lambda c: c["name"])
def test_lowering_reproduces_tests_cpp_known_answers(case):
    p = F.compile(F.from_sexpr(tup(case["graph"])))
    x = np.array([c[0] for c in case["calls"]], np.float32)[:, None, :]
    y, _ = run_ir(p, x)
    want = np.array([c[1] for c in case["calls"]], np.float32)
    assert np.array_equal(y[:, 0, :], want)


def test_python_edsl_operators_build_the_same_graph():
    from zignal_amd.flowz import _1, _2
    b0, b1, b2, a1, a2 = (float(v) for v in (G.B0, G.B1, G.B2, G.A1, G.A2))
    fwd = b0 * _1 + b1 * _1[_1] + b2 * _1[_2]
    bwd = ~(_2 + a1 * _1[_1] + a2 * _1[-2])
    p1 = F.compile(fwd >> bwd)
    p2 = F.compile(F.from_sexpr(G.df1()))
    assert p1.ir() == p2.ir() and p1.outputs() == p2.outputs() and p1.lines() == p2.lines()
    assert (fwd >> bwd).ins == 1 and (fwd >> bwd).outs == 1
    assert F.seq(_1, _1, _1[_1]).ins == 1 and F.chan(_1, _2).outs == 2 and (_1 | _1).ins == 2


GRAPHS = {
    "df1": G.df1, "df2": G.df2, "df1t": G.df1t, "df2t": G.df2t, "cascade6": lambda: G.df1_cascade(6),
    "integrator": G.integrator, "one_quad": G.one_quad, "one_quad_chain": G.one_quad_chain,
    "cross_wire": G.cross_wire, "par4": G.par4_sum, "par4_fanout": G.par4_sum_fanout,
    "nested_fb": lambda: G.fb(G.seq(G.DEL(1, 1), G.fb(G.add(G.DEL(1, 1), G.IN(2))))),   # tests.cpp:60
    "long_delay": lambda: G.seq(G.add(G.IN(1), G.mul(G.lit(0.5), G.DEL(1, 40))),
                                G.fb(G.add(G.mul(G.lit(0.7), G.DEL(1, 23)), G.IN(2)))),
    "div_neg": lambda: ("div", ("neg", G.IN(1)), G.add(G.lit(2.5), G.mul(G.DEL(1, 1), G.DEL(1, 1)))),
    "far_delays": lambda: G.seq(G.add(G.IN(1), G.mul(G.lit(0.5), G.DEL(1, 400))),
                                G.fb(G.add(G.add(G.mul(G.lit(0.6), G.DEL(1, 333)), G.mul(G.lit(0.1), G.DEL(1, 2))), G.IN(2)))),
    "one_pole_double_literal": G.one_pole_readme,                      # flowz/README.md:52
    "mixed_precision_biquad": G.mixed_precision_biquad,
    "double_div": lambda: ("div", G.add(G.IN(1), G.lit64(1.5)), G.add(G.lit64(3.0), G.mul(G.DEL(1, 1), G.DEL(1, 1)))),
}


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_lowering_vs_oracle(name):
    g = GRAPHS[name]()
    p = F.compile(F.from_sexpr(g))
    ns, T = 3, (900 if name == "far_delays" else 96)
    assert p.n_in == O.input_arity(g) and p.n_out == O.output_arity(g)
    x = O.synth_input(11, np.arange(ns), T, n_wires=max(p.n_in, 1))
    want = O.compile(g, ns).run(x)
    got, _ = run_ir(p, x)
    assert same(got, want)


@pytest.mark.parametrize("name", sorted(G.canonical_shape_bodies()))
def test_feedback_expressions_of_the_canonical_shape_tests_lower_like_the_oracle(name):
    """test/tests.cpp:26-60 checks the canonical TYPE of ~X (un2bin: the split into a direct and a delayed part); this library orders
    a feedback loop by a delay-breaking topological sort instead, so the check is behavioural: same arities, same bits."""
    g = G.fb(G.canonical_shape_bodies()[name])
    p = F.compile(F.from_sexpr(g))
    assert (p.n_in, p.n_out) == (O.input_arity(g), O.output_arity(g))
    ns, T = 3, 40
    x = O.synth_input(13, np.arange(ns), T, n_wires=max(p.n_in, 1))
    got, _ = run_ir(p, x)
    assert same(got, O.compile(g, ns).run(x))


def test_graphs_the_shipped_reference_misroutes_are_flagged_and_their_values_pinned():
    """binary_feedback hands its future part the external inputs from position std::min(0, ...) = 0 on
    (flowz.hpp:1045-1050) -- wrong as soon as the promise part keeps external inputs for itself.  The reference only checks the ANALYSIS
    of such graphs (test/tests.cpp:67-77); evaluated, its shipped header gives 10, 30, 70 on (10,1),(20,2),(30,3) (SURVEY App. D.5's
    model).  This library routes per the arity table: y[n] = a[n-1] + v[n], a[n] = y[n] + u[n-1]  ->  1, 3, 16.  The choice is
    pinned here, and the program says that it differs."""
    ar = {c["name"]: c for c in KA["arity"]}
    g2, g3 = tup(ar["fb_two_inputs"]["graph"]), tup(ar["fb_three_inputs"]["graph"])
    p = F.compile(F.from_sexpr(g2))
    assert p.differs_from_reference == 1 and "flowz.hpp:1045-1050" in p.note and p.note.startswith("note:")
    x = np.array([[[10, 1]], [[20, 2]], [[30, 3]]], np.float32)
    y, _ = run_ir(p, x)
    assert y.ravel().tolist() == [1.0, 3.0, 16.0]
    assert O.compile(g2, 1).run(x).ravel().tolist() == [1.0, 3.0, 16.0]
    p3 = F.compile(F.from_sexpr(g3))
    assert p3.differs_from_reference == 2 and p3.n_in == 3
    assert F.compile(F.from_sexpr(g2), typed=True).differs_from_reference == 1
    # nested: the flag is the graph's, wherever the feedback sits
    assert F.compile(F.from_sexpr(G.seq(g2, G.df1()))).differs_from_reference == 1
    # every graph the reference EVALUATES in its tests, the BASELINE workloads and the canonical-shape bodies: no divergence
    clean = [tup(c["graph"]) for c in KA["evaluation"] + KA["readme"]] + [G.fb(b) for b in G.canonical_shape_bodies().values()]
    clean += [G.df1_cascade(6), G.par4_sum(), G.par4_sum_fanout(), G.osc_chain(6), G.df2(), G.df1t(), G.df2t(), G.lds_ring_comb(), G.far_comb(300),
              G.fb(G.seq(G.add(G.IN(1), G.IN(2)), G.DEL(1, 1)))]       # (a promise part with an input of its own and a future part with none: harmless)
    for g in clean:
        q = F.compile(F.from_sexpr(g))
        assert q.differs_from_reference == 0 and q.note == "", g


def test_remainder_kernel_of_a_far_line_with_a_shallow_tap_builds(tmp_path, monkeypatch):
    """A plain time-major block whose laps leave a few streams over runs a remainder kernel next to them.  Its chunk must respect the
    cap the HBM rings put on every kernel -- half the youngest ring read: with a tap 20 samples back, 10 rows -- or the shape is refused
    although the same graph runs at 1 048 576 streams (round-5 advisor finding: the remainder asked for 16)."""
    monkeypatch.setenv("FLOWZ_HIP_CACHE", str(tmp_path))
    g = G.fb(G.add(G.add(G.mul(G.lit(0.5), G.DEL(1, 300)), G.mul(G.lit(0.25), G.DEL(1, 20))), G.IN(2)))
    p = F.compile(F.from_sexpr(g))
    assert p.max_delay == 300
    for ns in (1048576, 1049600, 1052672):
        p.build(None, ns, 4096)                              # main kernel + remainder kernel, both resolved as a launch would
        name = p.kernel_name(None, ns, 4096)
        assert name.startswith("fz_block_kernel_p"), name


def test_reserved_variant_flag_bits_are_refused():
    """Round 6 took the experiment knobs of rounds 1-5 out of the variant flags (plain loads / block order, the SLP vectoriser, cache-policy
    fields, the persistent launch): they are compile-time switches of the kernel source now (FLOWZ_HIP_EXTRA_OPTS=-DFZ_DBG_...).  A caller
    that still sets one of those bits is told so instead of silently getting the default kernel under another name."""
    p = F.compile(F.from_sexpr(G.df1_cascade(2)))
    for bit in (1, 2, 4, 1 << 12, 5 << 16, 1 << 27):
        with pytest.raises(F.FlowzError) as ei:
            p.kernel_name(F.make_variant(2, 8, 256, bit), 1 << 20, 4096)
        assert ei.value.code == _capi.FZ_E_INVALID and "reserved" in str(ei.value)
    assert not any(hasattr(_capi, n) for n in ("FZ_VF_NO_NT", "FZ_VF_NO_XCD_REMAP", "FZ_VF_SLP"))
    hdr = open(os.path.join(ROOT, "include", "flowz_hip.h")).read()
    assert "FZ_VF_SLP" not in hdr and "FZ_VF_NO_NT" not in hdr and "FZ_VF_NO_XCD_REMAP" not in hdr


CMP_GRAPHS = {
    "hard_clipper": G.hard_clipper,
    "clipped_biquad": G.clipped_biquad,
    "clipped_biquad_cascade": lambda: G.seq(G.clipped_biquad(), G.clipped_biquad(-0.25, 0.4), G.df1()),
    "logic": lambda: ("chan", ("chan", ("not", G.IN(1)), ("or", G.IN(1), G.lit(0.0))), ("mul", ("lit64", 2.0), ("lt", G.IN(1), ("lit64", 0.25)))),
    "compare_in_double": lambda: G.mul(("ge", G.mul(("lit64", 1.0000000001), G.IN(1)), G.IN(1)), G.IN(1)),     # x * 1.0000000001 >= x decided in double
    "gated_feedback": lambda: G.fb(G.add(G.mul(G.mul(G.lit(0.9), G.DEL(1, 1)), ("lt", G.DEL(1, 1), G.lit(0.8))), G.IN(2))),   # an integrator that drops its state above 0.8
    "two_wire_select": lambda: G.add(G.mul(G.IN(1), ("gt", G.IN(1), G.IN(2))), G.mul(G.IN(2), ("le", G.IN(1), G.IN(2)))),          # max(_1, _2), as C++ spells it without <algorithm>
}


def edge_input(seed, ns, T, n_wires=1):
    """noise with the values comparisons are sensitive to: +-0, the thresholds themselves, NaN, +-inf, denormals"""
    x = O.synth_input(seed, np.arange(ns), T, n_wires=n_wires)
    special = np.array([0.0, -0.0, 0.5, -0.5, 0.8, 0.25, np.nan, np.inf, -np.inf, 1e-40, -1e-40, np.float32(0.5) - np.float32(2 ** -25)], np.float32)
    rng = np.random.default_rng(seed)
    k = rng.integers(0, T, 4 * len(special)), rng.integers(0, ns, 4 * len(special)), rng.integers(0, n_wires, 4 * len(special))
    x[k] = np.tile(special, 4)
    return x


@pytest.mark.parametrize("name", sorted(CMP_GRAPHS))
def test_comparison_and_logical_operators_lower_like_the_oracle(name):
    """SURVEY 8 row a4, widened in round 6: proto::_default applies whatever C++ operator a node is (flowz.hpp:51-55, :769-772), so < <= > >= == != !
    && || are legal in a flow-graph.  They yield the operator's bool as it behaves in arithmetic: 1 or 0, a float until it meets a double;
    operands are compared in their common type; IEEE rules for NaN.  Lowering == oracle on inputs with +-0, the thresholds, NaN, +-inf, denormals."""
    g = CMP_GRAPHS[name]()
    p = F.compile(F.from_sexpr(g))
    assert (p.n_in, p.n_out) == (O.input_arity(g), O.output_arity(g)) and not p.stage_packable
    ns, T = 5, 120
    x = edge_input(31, ns, T, n_wires=max(p.n_in, 1))
    with np.errstate(all="ignore"):
        want = O.compile(g, ns).run(x)
        got, _ = run_ir(p, x)
    nan = np.isnan(got) & np.isnan(want)
    assert np.array_equal(np.where(nan, 0, got).view(np.uint32), np.where(nan, 0, want).view(np.uint32))
    assert all(d == "f32" for d, (k, *_r) in zip(p.ir_dtypes(), p.ir()) if k in ("lt", "le", "gt", "ge", "eq", "ne"))
    # the recipe of a kernel manifest carries the new operators
    lib = _capi.lib
    buf = ctypes.create_string_buffer(1 << 16)
    e1 = F.from_sexpr(g)                                         # (kept alive across the call: the handle is the object's)
    n = lib.fz_expr_recipe(e1._h, buf, len(buf))
    e2 = F.Expr(lib.fz_expr_from_recipe(buf.raw[:n]))
    assert F.compile(e2).ir() == p.ir()


def test_comparison_operators_python_spelling_typing_and_isa(tmp_path, monkeypatch):
    monkeypatch.setenv("FLOWZ_HIP_CACHE", str(tmp_path))
    x = F._1
    a = F.compile(x * ((x > -0.5).logical_and(x < 0.5)) + 0.5 * (x >= 0.5) + -0.5 * (x <= -0.5))
    assert a.ir() == F.compile(F.from_sexpr(G.hard_clipper())).ir() and a.n_ops == 12
    assert F.compile(x.eq(F._2).logical_or(x.ne(1.0)).logical_not()).n_in == 2
    with pytest.raises(TypeError):
        max(x, F._2)                                              # a comparison is a graph node, not a Python truth value
    # the bool takes the type of what it meets: a float multiplication, a double one
    assert F.compile((x < F.lit64(1.0)) * x, typed=True).output_dtypes() == ["f32"]
    assert F.compile((x < 1.0) * F.lit64(2.0), typed=True).output_dtypes() == ["f64"]
    with pytest.raises(F.FlowzError) as ei:
        F.compile(F.litc(1.0, 0.0) * x < x)                       # std::complex has no ordering
    assert ei.value.code == _capi.FZ_E_GRAPH
    # the kernel: compares and selects, and still no contraction anywhere
    import subprocess
    for P in (1, 2, 4):
        F.compile(F.from_sexpr(G.clipped_biquad())).build(F.make_variant(P, 8))
    objs = list(tmp_path.glob("*.hsaco"))
    assert len(objs) == 3
    for obj in objs:
        dis = subprocess.check_output(["/opt/rocm/lib/llvm/bin/llvm-objdump", "-d", str(obj)], text=True)
        assert "v_cmp_" in dis and "v_cndmask" in dis
        assert not re.search(r"v_(pk_)?(fma|fmac|mad|mac)(_mix|_mixlo|_mixhi|_legacy)?_(f16|f32|f64|bf16)", dis)


def test_kernel_experiment_switches_are_compile_time_options(tmp_path):
    """What rounds 1-5 had as variant flags (plain loads and stores, the plain block order, cache-policy fields) are -D switches of the kernel source now,
    handed over through FLOWZ_HIP_EXTRA_OPTS (read once per process, part of the kernel-cache key): every one of them still builds, under a name of its own."""
    import subprocess
    import sys
    code = ("import sys\nfrom zignal_amd import flowz as F, workloads as W\n"
            "p = F.compile(F.from_sexpr(W.df1_cascade(2)))\n"
            "for v in ((2, 8, 256, 0), (1, 4, 1024, F.C.FZ_VF_LOCKSTEP | F.C.FZ_VF_GRID_SYNC), (1, 32, 0, F.C.FZ_VF_STREAM_MAJOR)):\n"
            "    p.build(F.make_variant(*v))\nprint(p.kernel_code_id(F.make_variant(2, 8, 256, 0)))\n")
    ids = set()
    for opts in ("", "-DFZ_DBG_NO_NT", "-DFZ_DBG_NO_XCD_REMAP", "-DFZ_DBG_AUX_LD=0 -DFZ_DBG_AUX_ST=16"):
        env = dict(os.environ, FLOWZ_HIP_CACHE=str(tmp_path / ("c" + str(len(ids)))), FLOWZ_HIP_EXTRA_OPTS=opts)
        out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=ROOT)
        assert out.returncode == 0, opts + ": " + out.stderr[-1500:]
        ids.add(out.stdout.split()[-1])
    assert len(ids) == 4


def test_lowering_osc_chain_with_stream_params():
    g = G.osc_chain(6)
    p = F.compile(F.from_sexpr(g))
    assert p.n_param == 31 and p.n_state == 14 and p.n_ops == 3 + 54   # resonator line is shared with stage 1
    ns, T = 4, 128
    P = W.osc_chain_params(20160513, np.arange(ns))
    x = np.zeros((T, ns, 1), np.float32)
    x[0] = 1
    got, _ = run_ir(p, x, params=P)
    assert same(got, O.compile(g, ns, params=P).run(x))


def test_state_sharing_and_minimal_state():
    p = F.compile(F.from_sexpr(G.df1_cascade(6)))
    # 2 + 2N floats for an N-stage DF1 chain, 54 unfused float32 ops per sample
    assert (p.n_state, p.n_lines, p.n_ops, p.n_const, p.max_delay) == (14, 7, 54, 5, 2)
    assert F.compile(F.from_sexpr(G.df2())).n_state == 2
    assert F.compile(F.from_sexpr(G.par4_sum())).n_state == 16


def test_block_chaining_through_state_rows():
    g = G.df1_cascade(2)
    p = F.compile(F.from_sexpr(g))
    x = O.synth_input(3, np.arange(2), 64)
    whole, st_w = run_ir(p, x)
    a, st = run_ir(p, x[:40])
    b, st = run_ir(p, x[40:], state=st)
    assert same(np.concatenate([a, b]), whole) and same(st, st_w)


def test_malformed_graphs_are_rejected():
    with pytest.raises(F.FlowzError) as ei:
        F.compile(~(F._1 + F._2))                      # delay-free loop
    assert ei.value.code == _capi.FZ_E_GRAPH and "delay" in str(ei.value)
    with pytest.raises(F.FlowzError):
        F.compile(~F._1)                               # wire fed straight back to itself
    with pytest.raises(F.FlowzError):
        (F._1 | F._1) + F._2                           # arithmetic on a 2-wire bundle
    with pytest.raises(F.FlowzError):
        F._1[0]                                        # delay 0 is not a delay


def test_kernel_source_and_jit_build_for_gfx950_without_gpu(tmp_path, monkeypatch):
    monkeypatch.setenv("FLOWZ_HIP_CACHE", str(tmp_path))
    p = F.compile(F.from_sexpr(G.df1_cascade(2)))
    src = p.source(F.make_variant(2, 4))
    assert "#define FZ_P 2" in src and "fz_block_kernel" in src and "struct fz_graph" in src
    p.build(F.make_variant(2, 4))
    objs = list(tmp_path.glob("*.hsaco"))
    assert len(objs) == 1 and objs[0].stat().st_size > 1000
    # cache hit: same key, no new file
    F.compile(F.from_sexpr(G.df1_cascade(2))).build(F.make_variant(2, 4))
    assert len(list(tmp_path.glob("*.hsaco"))) == 1


def test_kernel_cache_rejects_damaged_files_and_ignores_literal_values(tmp_path, monkeypatch):
    """a truncated / foreign cache file is detected (trailer: magic, size, hash), deleted and rebuilt; graphs that
    differ only in coefficient VALUES share one code object (coefficients travel in the kernarg)."""
    monkeypatch.setenv("FLOWZ_HIP_CACHE", str(tmp_path))
    F.compile(F.from_sexpr(G.df1(0.5, 0.25, 0.125, 0.2, -0.8))).build(F.make_variant(1, 4))
    (obj,) = tmp_path.glob("*.hsaco")
    good = obj.read_bytes()
    F.compile(F.from_sexpr(G.df1(0.75, 0.25, 0.125, 0.3, -0.7))).build(F.make_variant(1, 4))      # other literals: same file
    assert [o.name for o in tmp_path.glob("*.hsaco")] == [obj.name]
    for bad in (good[: len(good) // 2], b"\x7fELF" + b"x" * 4000, good[:-1] + bytes([good[-1] ^ 1])):
        obj.write_bytes(bad)
        F.compile(F.from_sexpr(G.df1(0.5, 0.25, 0.125, 0.2, -0.8))).build(F.make_variant(1, 4))
        assert obj.read_bytes() == good


def test_no_fma_contraction_in_generated_kernel(tmp_path, monkeypatch):
    """contraction changes the 4th impulse-response sample."""
    import subprocess
    monkeypatch.setenv("FLOWZ_HIP_CACHE", str(tmp_path))
    for P in (1, 2, 4):
        F.compile(F.from_sexpr(G.df1_cascade(2))).build(F.make_variant(P, 4))
    for obj in tmp_path.glob("*.hsaco"):
        dis = subprocess.check_output(["/opt/rocm/lib/llvm/bin/llvm-objdump", "-d", str(obj)], text=True)
        assert "v_pk_mul_f32" in dis or "v_mul_f32" in dis
        assert not re.search(r"v_(pk_)?(fma|fmac|mad|mac)(_mix|_mixlo|_mixhi|_legacy)?_(f16|f32|f64|bf16)", dis)
        notes = subprocess.check_output(["/opt/rocm/lib/llvm/bin/llvm-readelf", "--notes", str(obj)], text=True)
        assert ".vgpr_spill_count: 0" in notes and ".private_segment_fixed_size: 0" in notes


def _main_loop_histogram(dis):
    """opcode counts of the LARGEST loop of a disassembled kernel (its chunk loop): between a backward branch and its target"""
    rows = []
    for ln in dis.splitlines():
        m = re.match(r"\s+(\S+).*//\s*([0-9A-Fa-f]+):", ln)
        if m:
            rows.append((int(m.group(2), 16), m.group(1), ln))
    labels, pending = {}, None
    for ln in dis.splitlines():
        m = re.match(r"^([0-9a-f]+) <(.+)>:", ln)
        if m:
            pending = m.group(2)
        elif pending and "//" in ln:
            labels[pending] = int(ln.split("//")[1].split(":")[0].strip(), 16)
            pending = None
    best = {}
    for addr, op, ln in rows:
        m = re.search(r"s_cbranch\w+.*<(.+?)(?:\+0x([0-9a-f]+))?>", ln)
        if not m or m.group(1) not in labels:
            continue
        tgt = labels[m.group(1)] + (int(m.group(2), 16) if m.group(2) else 0)
        if tgt < addr:
            body = [o for a, o, _ in rows if tgt <= a <= addr]
            if len(body) > sum(best.values()):
                best = {}
                for o in body:
                    best[o] = best.get(o, 0) + 1
    return best


def test_lds_rings_are_vectorised_in_time_in_the_isa(tmp_path, monkeypatch):
    """Round 5: the LDS rings of the frame kernels are lane-major and accessed 16 bytes at a time -- 4 / P time steps per ds_read_b128 /
    ds_write_b128, reads fetched and pushes flushed per sub-chunk of G steps.  The two combs of the bench line's lds_ring graph
    (reads 40 and 23 samples back, two pushes per step: 4 LDS instructions per step in round 4) issue less than a quarter of that with
    one stream per lane and less than half with two; no dword-sized LDS access is left in the chunk loop."""
    import subprocess
    monkeypatch.setenv("FLOWZ_HIP_CACHE", str(tmp_path))
    from zignal_amd import workloads as ZW
    g = ZW.lds_ring_comb()
    for P, block, bound in ((1, 256, 1.0), (2, 128, 2.0)):
        for f in tmp_path.glob("*.hsaco"):
            f.unlink()
        p = F.compile(F.from_sexpr(g))
        v = F.make_variant(P, 32, block)
        src = p.source(v)
        assert "#define FZ_RING_G 16" in src                                # the largest power of two <= the youngest read (23)
        p.build(v)
        (obj,) = tmp_path.glob("*.hsaco")
        dis = subprocess.check_output(["/opt/rocm/lib/llvm/bin/llvm-objdump", "-d", str(obj)], text=True)
        h = _main_loop_histogram(dis)
        steps = h.get("buffer_store_dword" if P == 1 else "buffer_store_dwordx2", 0)     # one frame store per step
        assert steps >= 32 and steps % 32 == 0, h
        lds = sum(n for o, n in h.items() if o.startswith("ds_"))
        assert lds / steps < bound, (P, lds, steps, h)
        assert not any(o in h for o in ("ds_read_b32", "ds_write_b32", "ds_read_b64", "ds_write_b64") if h.get(o, 0) > 2), h
        assert not re.search(r"v_(pk_)?(fma|fmac|mad|mac)(_mix|_mixlo|_mixhi|_legacy)?_(f16|f32|f64|bf16)", dis)
        notes = subprocess.check_output(["/opt/rocm/lib/llvm/bin/llvm-readelf", "--notes", str(obj)], text=True)
        assert ".vgpr_spill_count: 0" in notes and ".private_segment_fixed_size: 0" in notes
    # a read younger than a 16-byte access of the lane (1 sample back on a ring: a deep line with a shallow tap) keeps the rings in place
    shallow = ("seq", ("in", 1), ("add", ("del", 1, 40), ("del", 1, 1)))
    assert "#define FZ_RING_G 0" in F.compile(F.from_sexpr(shallow)).source(F.make_variant(1, 16, 256))


def test_wave_split_kernels_in_the_isa(tmp_path, monkeypatch):
    """the wave-split / I/O-wave code objects, disassembled: no contraction, no scratch, no waterfall loop around a buffer access
    (a descriptor built from a VGPR would cost one per load), the cut wire moves as 16-byte LDS accesses, one s_barrier per round
    body, and a part of the 6-biquad cascade issues 18 arithmetic instructions per step instead of the 27 of the whole graph."""
    import subprocess
    monkeypatch.setenv("FLOWZ_HIP_CACHE", str(tmp_path))
    p = F.compile(F.from_sexpr(G.df1_cascade(6)))
    for fl in (F.C.FZ_VF_WAVES(2), F.C.FZ_VF_WAVES(3), F.C.FZ_VF_IO_WAVE, F.C.FZ_VF_WAVES(2) | F.C.FZ_VF_IO_WAVE):
        p.build(F.make_variant(1, 16, 0, fl))
    objs = list(tmp_path.glob("*.hsaco"))
    assert len(objs) == 4
    for obj in objs:
        dis = subprocess.check_output(["/opt/rocm/lib/llvm/bin/llvm-objdump", "-d", str(obj)], text=True)
        notes = subprocess.check_output(["/opt/rocm/lib/llvm/bin/llvm-readelf", "--notes", str(obj)], text=True)
        assert not re.search(r"v_(pk_)?(fma|fmac|mad|mac)(_mix|_mixlo|_mixhi|_legacy)?_(f16|f32|f64|bf16)", dis)
        assert ".vgpr_spill_count: 0" in notes and ".private_segment_fixed_size: 0" in notes
        assert "v_cmp_eq_u64" not in dis and dis.count("v_readfirstlane_b32") < 16            # no waterfall loops (readfirstlane x 4 + 64-bit compares per access)
        assert "ds_write_b128" in dis and "ds_read_b128" in dis and "s_barrier" in dis
        assert "scratch_" not in dis and "flat_load" not in dis and "flat_store" not in dis
    # instruction count of an unmasked round of a two-part wave: between two barriers with no v_cndmask in between
    dis = subprocess.check_output(["/opt/rocm/lib/llvm/bin/llvm-objdump", "-d", str(
        [o for o in objs if "w2f1024" in subprocess.check_output(["/opt/rocm/lib/llvm/bin/llvm-readelf", "--notes", str(o)], text=True)][0])], text=True)
    ops = [ln.split()[0] for ln in dis.splitlines() if ln.startswith("\t")]
    rounds, cur = [], []
    for op in ops:
        if op == "s_barrier":
            rounds.append(cur)
            cur = []
        else:
            cur.append(op)
    plain = [r for r in rounds if r and not any(o.startswith("v_cndmask") for o in r) and sum(o.startswith("v_pk_") for o in r) >= 16 * 9]
    assert plain, "no unmasked round found"
    arith = min(sum(o.startswith(("v_pk_mul", "v_pk_add", "v_mul_f32", "v_add_f32", "v_sub_f32")) for o in r) for r in plain)
    assert arith == 16 * 18, arith                                        # 9 packed + 9 scalar per step, 16 steps per round


def test_stream_major_pair_long_run_body_rules_and_code(tmp_path, monkeypatch):
    """The pair long-run body of the stream-major kernel (host side): the default for deep 1-in/1-out graphs with uniform
    coefficients from 2^19 even streams on, on request otherwise (streams_per_lane = 2 with FZ_VF_SM_LONG, unroll 64 only);
    its code object: no contraction, no scratch, no waterfall loops, the patch of [64 lanes][2 x 64 + 4] floats per wave, and
    a loop whose steps are nothing but the graph's packed operations (no moves: the patch rows are the register pairs)."""
    import subprocess
    monkeypatch.setenv("FLOWZ_HIP_CACHE", str(tmp_path))
    SMF, LONG = F.C.FZ_VF_STREAM_MAJOR, F.C.FZ_VF_SM_LONG
    sm = F.make_variant(0, 0, 0, SMF)
    p = F.compile(F.from_sexpr(G.df1_cascade(6)))
    assert p.kernel_name(sm, 1 << 20, 4096) == "fz_block_kernel_p2u64b64f384"
    assert p.kernel_name(sm, 1 << 19, 256) == "fz_block_kernel_p2u64b64f384"
    assert p.kernel_name(sm, 1 << 18, 4096).startswith("fz_block_kernel_p1u128b64s6f")           # below 2^19 streams the one-stream body (round 6: level or ahead on every bench line)
    assert p.kernel_name(sm, 1 << 17, 4096).startswith("fz_block_kernel_p1u128b64s6f") and p.kernel_name(sm, 3 << 16, 4096).startswith("fz_block_kernel_p1u128b64s6f")
    assert p.kernel_name(sm, 1 << 16, 4096).startswith("fz_block_kernel_p1u128b64s6f")            # the pair body would leave half of the CUs idle; one-wave workgroups at <= one wave per SIMD
    assert p.kernel_name(sm, (1 << 20) + 1, 4096).startswith("fz_block_kernel_p1u128b64s6f")      # an odd count has no pairs
    assert p.kernel_name(sm, 1 << 20, 128).startswith("fz_block_kernel_p1u")                        # shorter than a long-run block
    assert p.kernel_name(F.make_variant(0, 0, 0, SMF | F.C.FZ_VF_SM_SHORT), 1 << 20, 4096).startswith("fz_block_kernel_p1u32")   # anything asked for: as before
    assert F.compile(F.from_sexpr(G.df1_cascade(2))).kernel_name(sm, 1 << 20, 4096).startswith("fz_block_kernel_p1u128b64f")     # shallow graphs
    assert F.compile(F.from_sexpr(G.osc_chain(6))).kernel_name(sm, 1 << 20, 4096) == "fz_block_kernel_p2u64b64f384"              # per-stream coefficients ride along as packed pairs (round 4)
    for bad in (F.make_variant(2, 128, 0, SMF | LONG), F.make_variant(2, 32, 0, SMF | LONG)):
        with pytest.raises(F.FlowzError):
            p.kernel_name(bad, 1024, 512)
    with pytest.raises(F.FlowzError):
        p.kernel_name(F.make_variant(2, 64, 0, SMF | LONG), 1023, 512)                              # n_streams % streams_per_lane
    with pytest.raises(F.FlowzError):
        F.compile(F.from_sexpr(G.par4_sum())).kernel_name(F.make_variant(2, 64, 0, SMF | LONG), 1024, 512)   # 4-wire frames
    r = p.kernel_resources(F.make_variant(2, 64, 0, SMF | LONG), 1 << 20, 4096)
    assert r["scratch_bytes"] == 0 and r["lds_bytes"] == 64 * (2 * 64 + 4) * 4 and r["vgprs"] <= 512 and r["unroll"] == 64
    obj = [o for o in tmp_path.glob("*.hsaco")
           if p.kernel_symbol(F.make_variant(2, 64, 0, SMF | LONG), 1 << 20, 4096) in subprocess.check_output(["/opt/rocm/lib/llvm/bin/llvm-readelf", "--notes", str(o)], text=True)][0]
    dis = subprocess.check_output(["/opt/rocm/lib/llvm/bin/llvm-objdump", "-d", str(obj)], text=True)
    assert not re.search(r"v_(pk_)?(fma|fmac|mad|mac)(_mix|_mixlo|_mixhi|_legacy)?_(f16|f32|f64|bf16)", dis)
    assert "scratch_" not in dis and "flat_load" not in dis and "v_cmp_eq_u64" not in dis and dis.count("v_readfirstlane_b32") < 8
    # the blocks of straight-line code between branches that hold most of the arithmetic: the 16-step loop bodies of the two halves
    ops = [ln.split()[0] for ln in dis.splitlines() if ln.startswith("\t")]
    blocks, cur = [], []
    for op in ops:
        cur.append(op)
        if op.startswith(("s_cbranch", "s_branch", "s_endpgm")):
            blocks.append(cur)
            cur = []
    loops = [b for b in blocks if sum(o.startswith("v_pk_") for o in b) >= 10 * 54]
    assert len(loops) == 2, [len(b) for b in blocks]
    for b in loops:
        packed = sum(o.startswith(("v_pk_mul_f32", "v_pk_add_f32")) for o in b)
        assert packed % 54 == 0 and packed >= 13 * 54                    # whole steps of two streams: 54 packed operations each
        other_valu = [o for o in b if o.startswith("v_") and not o.startswith("v_pk_")]
        assert len(other_valu) <= 8, other_valu                          # address arithmetic of the loop (either compiler), no pair assembly: a move per step would be 14+
        assert sum(o == "s_nop" for o in b) <= 4                         # the stages of consecutive steps overlap (iterative ILP scheduling)


def test_product_fails_loudly_without_gpu():
    if F.device_count() > 0:
        pytest.skip("GPU present")
    p = F.compile(F.from_sexpr(G.df1()))
    with pytest.raises(F.NoDeviceError):
        p.run_block_ptr(ctypes.c_void_p(256), ctypes.c_void_p(512), ctypes.c_void_p(1024), None, 64, 8)
    bank = ctypes.c_void_p()
    assert _capi.lib.fz_bank_create(p._h, 4, ctypes.byref(bank)) == _capi.FZ_E_NO_DEVICE
    assert "no CPU fallback" in _capi.last_error()


def test_argument_checks_do_not_depend_on_assert_statements():
    """The Python mirror hands raw pointers to the C ABI: its shape / dtype / device checks must survive `python -O`
    (ADVICE round 2), so none of them may be an `assert`; a host tensor is refused before anything is launched."""
    import torch
    src = open(os.path.join(ROOT, "zignal_amd", "flowz.py")).read()
    assert not [ln for ln in src.splitlines() if ln.lstrip().startswith("assert ")]
    p = F.compile(F.from_sexpr(G.df1()))
    with pytest.raises(F.NoDeviceError):
        p.run_block(torch.zeros((8, 64, 1)))
    with pytest.raises(F.FlowzError):
        p.run_window(torch.zeros((8, 64, 1)), torch.zeros((8, 64, 1)), torch.zeros((p.n_state, 64)), 0, 4)


def test_product_never_imports_the_oracle():
    for dirpath, _, files in os.walk(os.path.join(ROOT, "zignal_amd")):
        for f in files:
            if f.endswith((".py", ".cpp", ".hip", ".hpp", ".inc", ".h")):
                txt = open(os.path.join(dirpath, f)).read()
                assert "oracle" not in txt.replace("no CPU", ""), f"{f} mentions the oracle"
    hdr = open(os.path.join(ROOT, "include", "flowz_hip.h")).read()
    assert "oracle" not in hdr


def test_stage_split_detection_and_packed_kernel_builds(tmp_path, monkeypatch):
    import subprocess
    monkeypatch.setenv("FLOWZ_HIP_CACHE", str(tmp_path))
    want = {"cascade6": (G.df1_cascade(6), 1), "cascade2": (G.df1_cascade(2), 1), "cascade5": (G.df1_cascade(5), 1),
            "df1": (G.df1(), 0), "osc": (G.osc_chain(6), 1), "one_quad_chain": (G.one_quad_chain(), 1),
            "par4": (G.par4_sum(), 0), "cross_wire": (G.cross_wire(), 0),
            # a scalar suffix behind the chain (output gain; prefix + suffix)
            "cascade6_gain": (G.seq(G.df1_cascade(6), G.mul(G.lit(0.7), G.IN(1))), 1),
            "osc_cascade_mix": (G.seq(G.osc_chain(6), G.add(G.mul(G.lit(0.6), G.IN(1)), G.mul(G.lit(0.3), G.DEL(1, 2)))), 1)}
    for name, (g, ok) in want.items():
        assert F.compile(F.from_sexpr(g)).stage_packable == ok, name
    p = F.compile(F.from_sexpr(G.df1_cascade(6)))
    p.build(F.make_variant(1, 8, 256, _capi.FZ_VF_STAGE_PACK))
    (obj,) = tmp_path.glob("*.hsaco")
    dis = subprocess.check_output(["/opt/rocm/lib/llvm/bin/llvm-objdump", "-d", str(obj)], text=True)
    assert dis.count("v_pk_mul_f32") > 100 and not re.search(r"v_(pk_)?(fma|fmac|mad|mac)(_mix|_mixlo|_mixhi|_legacy)?_(f16|f32|f64|bf16)", dis)
    F.compile(F.from_sexpr(G.osc_chain(6))).build(F.make_variant(1, 8, 256, _capi.FZ_VF_STAGE_PACK))   # scalar prefix + 6 segments
    with pytest.raises(F.FlowzError):
        F.compile(F.from_sexpr(G.df1())).build(F.make_variant(1, 8, 256, _capi.FZ_VF_STAGE_PACK))
    ps = F.compile(F.from_sexpr(want["osc_cascade_mix"][0]))
    src = ps.source(F.make_variant(1, 8, 256, _capi.FZ_VF_STAGE_PACK))
    assert "#define FZ_NSEG 6" in src and "6 isomorphic segments" in src   # still six packed segments (one atom each: three pairs are ILP enough), prefix and suffix scalar
    ps.build(F.make_variant(1, 8, 256, _capi.FZ_VF_STAGE_PACK))


@pytest.mark.parametrize("case", KA["result_types"], ids=lambda c: "tests.cpp:" + c["lines"])
def test_output_dtypes_match_tests_cpp_result_types(case):
    p = F.compile(F.from_sexpr(tup(case["graph"])))
    assert p.output_dtypes() == case["types"]
    # fz_compile_typed == ResultType itself (tests.cpp:219 included: the delayed read of a double wire is double)
    pt = F.compile(F.from_sexpr(tup(case["graph"])), typed=True)
    assert pt.output_dtypes() == case.get("result_type", case["types"]) and pt.typed == 1 and p.typed == 0
    x = O.synth_input(9, np.arange(3), 12, n_wires=max(pt.n_in, 1))
    want = O.run_typed(O.compile(tup(case["graph"]), 3, typed=True), [x[:, :, i] for i in range(pt.n_in)], T=12)
    got = F.unpack_typed(run_ir(pt, x)[0], pt.output_dtypes())
    assert all(a.dtype == b.dtype and np.array_equal(a, b) for a, b in zip(got, want))


def test_complex_wires_lower_to_float_pairs():
    """std::complex<float> terminals (tests.cpp:206-207) expand into (re, im) float nodes; the frame
    has one slot per part; what C++ would not compile is rejected."""
    p = F.compile(F.from_sexpr(G.complex_mix()))
    assert p.output_dtypes() == ["cf32", "f32"] and p.n_out == 3 and p.info.n_out_wires == 3 - 1
    assert all(dt == "f32" for dt in p.ir_dtypes())
    # evaluate the lowered IR on the CPU (test interpreter) against the oracle
    x = O.synth_input(3, np.arange(5), 33)
    assert np.array_equal(run_ir(p, x)[0].view(np.uint32), O.compile(G.complex_mix(), 5).run(x).view(np.uint32))
    # Python complex numbers are complex terminals
    q = F.compile(F._1 * (0.5 + 2j))
    assert q.output_dtypes() == ["cf32"] and q.n_out == 2
    for bad in (("mul", ("litc", 1.0, 0.0), ("lit64", 2.0)),
                ("seq", ("mul", ("litc", 1.0, 0.0), ("in", 1)), ("del", 1, 1)),
                ("fb", ("mul", ("litc", 1.0, 0.0), ("add", ("del", 1, 1), ("in", 2))))):
        with pytest.raises(F.FlowzError):
            F.compile(F.from_sexpr(bad))


def test_typed_programs_lowering_vs_oracle_and_std_complex():
    """fz_compile_typed: complex and double STATE, complex division (both spellings of __divsc3), double
    and complex INPUT wires -- lowered IR (test interpreter) == typed Python oracle == std::complex<float> compiled by g++."""
    x = O.synth_input(5, np.arange(7), 60)
    for g, want in ((G.complex_one_pole(), C.complex_one_pole(x, std=True)), (G.complex_div_mix(), C.complex_div_mix(x, std=True))):
        p = F.compile(F.from_sexpr(g), typed=True)
        assert p.output_dtypes() == ["cf32"] and p.n_out == 2 and p.info.n_out_wires == 1
        assert np.array_equal(run_ir(p, x)[0].view(np.uint32), want.view(np.uint32))
        y = O.run_typed(O.compile(g, 7, typed=True), [x[:, :, 0]])[0]
        assert np.array_equal(np.stack([y.real, y.imag], -1).view(np.uint32), want.view(np.uint32))
    p = F.compile(F.from_sexpr(G.complex_one_pole()), typed=True)
    assert p.line_dtypes() == ["re", "im"] and p.n_state == 2
    # untyped division works too (no state involved); complex state does not
    assert np.array_equal(run_ir(F.compile(F.from_sexpr(G.complex_div_mix())), x)[0].view(np.uint32), C.complex_div_mix(x, std=True).view(np.uint32))
    with pytest.raises(F.FlowzError):
        F.compile(F.from_sexpr(G.complex_one_pole()))
    # double state: the accumulator of tests.cpp:223 is a double; two float rows per slot, double lines first
    p = F.compile(F.from_sexpr(G.double_accumulator()), typed=True)
    assert p.line_dtypes() == ["f64"] and p.n_state == 2 and p.output_dtypes() == ["f64"] and p.n_out == 2
    y, st = run_ir(p, x)
    want = C.double_accumulator(x)
    assert np.array_equal(F.unpack_typed(y, ["f64"])[0], want[:, :, 0])
    assert np.array_equal(st.reshape(-1)[:14].view(np.float64), want[-1, :, 0])          # the state row IS the accumulator
    # the same graph under compile(): float state, double arithmetic above it (different values!)
    assert not np.array_equal(run_ir(F.compile(F.from_sexpr(G.double_accumulator())), x)[0][:, :, 0].astype(np.float64), want[:, :, 0])
    # mixed: a float line next to a double line -- double lines come first in the state layout
    g = G.chan(G.fb(G.add(G.DEL(1, 2), G.IN(2))), G.fb(G.add(G.DEL(1, 1), G.mul(G.lit64(0.5), G.IN(2)))))
    p = F.compile(F.from_sexpr(g), typed=True)
    assert p.line_dtypes() == ["f64", "f32"] and p.n_state == 4 and p.output_dtypes() == ["f32", "f64"]
    got = F.unpack_typed(run_ir(p, x)[0], p.output_dtypes())
    want = O.run_typed(O.compile(g, 7, typed=True), [x[:, :, 0]])
    assert all(a.dtype == b.dtype and np.array_equal(a, b) for a, b in zip(got, want))
    # a double line deeper than the register cap is an LDS ring of (low word, high word) pairs
    g = G.chan(G.fb(G.add(G.mul(G.lit(0.5), G.DEL(1, 12)), G.mul(G.lit64(0.25), G.IN(2)))), G.add(G.IN(1), G.DEL(1, 20)))
    p = F.compile(F.from_sexpr(g), typed=True)
    assert p.line_dtypes() == ["f64", "f32"] and p.n_state == 2 * 12 + 20 and p.n_lds_slots == 2 * 16 + 32
    got = F.unpack_typed(run_ir(p, x)[0], p.output_dtypes())
    want = O.run_typed(O.compile(g, 7, typed=True), [x[:, :, 0]])
    assert all(a.dtype == b.dtype and np.array_equal(a, b) for a, b in zip(got, want))
    # typed INPUT wires (the reference's callable is a template over its argument types): double, complex, float
    g = G.chan(G.chan(G.mul(G.IN(1), G.lit(0.5)), G.add(G.IN(2), G.DEL(2, 1))), G.mul(G.IN(3), G.IN(3)))
    dts = ["f64", "cf32", "f32"]
    p = F.compile(F.from_sexpr(g), in_dtypes=dts)
    assert (p.n_in, p.n_in_wires, p.input_dtypes(), p.output_dtypes()) == (5, 3, dts, dts)
    rng = np.random.default_rng(1)
    w = [rng.standard_normal((20, 3)), (rng.standard_normal((20, 3)) + 1j * rng.standard_normal((20, 3))).astype(np.complex64),
         rng.standard_normal((20, 3)).astype(np.float32)]
    got = F.unpack_typed(run_ir(p, F.pack_typed(w, dts))[0], p.output_dtypes())
    want = O.run_typed(O.compile(g, 3, typed=True, in_dtypes=dts), w)
    assert all(a.dtype == b.dtype and np.array_equal(a, b) for a, b in zip(got, want))
    # what C++ would not compile / this build does not offer
    for bad, kw in ((("fb", ("add", ("mul", ("litc", 1.0, 0.0), ("del", 1, 1)), ("mul", ("lit64", 1.0), ("in", 2)))), {}),   # complex meets double
                    (("add", ("in", 1), ("lit64", 1.0)), {"in_dtypes": ["cf32"]}),
                    (("fb", ("add", ("del", 1, 300), ("mul", ("lit64", 1.0), ("in", 2)))), {})):                             # double line beyond the LDS rings
        with pytest.raises(F.FlowzError):
            F.compile(F.from_sexpr(bad), typed=True, **kw)
    with pytest.raises(F.FlowzError):
        F.compile(F.from_sexpr(G.df1()), in_dtypes=["f32", "f32"])                   # one dtype per input wire


def test_complex_double_programs_lowering_vs_oracle_and_std_complex():
    """std::complex<double> (fz_literal_c64, FZ_DT_CF64): two double lines per delayed wire, four frame slots per wire,
    __divdc3 as FZ_IR_ABSLT / FZ_IR_SELECT over both sides of Smith's branch -- lowered IR (test interpreter) == typed Python
    oracle == std::complex<double> compiled by g++."""
    from test_oracle_c import _cdouble_input
    x = _cdouble_input(90, 5)
    g = G.cdouble_resonator()
    p = F.compile(F.from_sexpr(g), in_dtypes=["f64"])
    assert (p.n_in, p.n_in_wires, p.n_out, p.n_out_wires) == (2, 1, 4, 1) and p.output_dtypes() == ["cf64"]
    assert p.line_dtypes() == ["re64", "im64"] and p.output_slot_codes() == [6, 7, 8, 9] and p.n_state == 4
    kinds = [n[0] for n in p.ir()]
    assert kinds.count("abslt") == 1 and kinds.count("select") == 4 and set(p.ir_dtypes()) == {"f64"}   # |c| < |d| is shared by z/w and x/w
    got = F.unpack_typed(run_ir(p, F.pack_typed([x], ["f64"]))[0], ["cf64"])[0]
    assert got.dtype == np.complex128 and np.array_equal(got.view(np.int64), C.cdouble_resonator(x, std=True).view(np.int64))
    # complex<double> INPUT wires next to the other three types; a complex<double> wire through a depth-3 line
    g = G.chan(G.chan(("div", G.IN(1), G.add(G.IN(2), G.DEL(1, 3))), G.mul(G.IN(3), G.IN(4))), G.sub(G.IN(2), G.IN(1)))
    dts = ["cf64", "f64", "cf32", "f32"]
    p = F.compile(F.from_sexpr(g), in_dtypes=dts)
    assert (p.n_in, p.n_in_wires, p.input_dtypes(), p.output_dtypes()) == (9, 4, dts, ["cf64", "cf32", "cf64"])
    rng = np.random.default_rng(11)
    cplx = lambda dt: (rng.standard_normal((24, 3)) + 1j * rng.standard_normal((24, 3))).astype(dt)   # noqa: E731
    w = [cplx(np.complex128), rng.standard_normal((24, 3)), cplx(np.complex64), rng.standard_normal((24, 3)).astype(np.float32)]
    got = F.unpack_typed(run_ir(p, F.pack_typed(w, dts))[0], p.output_dtypes())
    want = O.run_typed(O.compile(g, 3, typed=True, in_dtypes=dts), w)
    assert all(a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(got, want))
    # untyped compile(): the wire computes in complex<double> and narrows to the float frame (re, im)
    g = ("div", G.mul(G.litc64(0.3, 0.4), G.mul(G.lit64(1.0), G.IN(1))), G.litc64(2.0, -1.0))
    p = F.compile(F.from_sexpr(g))
    xf = O.synth_input(3, np.arange(4), 16)
    assert np.array_equal(run_ir(p, xf)[0], O.compile(g, 4).run(xf)) and p.n_out == 2
    # the absorber: a float recursion variable that meets a complex<double> becomes one; a wire that stays float does not compile
    p = F.compile(F.from_sexpr(G.fb(G.add(G.mul(G.litc64(0.5, 0.5), G.DEL(1, 1)), G.mul(G.lit64(1.0), G.IN(2))))), typed=True)
    assert p.output_dtypes() == ["cf64"] and p.line_dtypes() == ["re64", "im64"]
    for bad, dts in ((G.mul(G.litc64(1, 0), G.IN(1)), ["f32"]), (G.mul(G.litc64(1, 0), G.litc(1, 0)), None),
                     (G.add(G.IN(1), G.IN(2)), ["cf64", "cf32"]), (G.add(G.IN(1), G.IN(2)), ["cf32", "f64"]),
                     (G.fb(G.chan(G.add(G.DEL(1, 1), G.IN(3)), G.mul(G.litc64(1, 0), G.DEL(1, 1)))), None),
                     (G.fb(G.add(G.mul(G.litc64(1, 0), G.DEL(1, 1)), G.mul(G.litc(1, 0), G.IN(2)))), None)):
        with pytest.raises(F.FlowzError):
            F.compile(F.from_sexpr(bad), typed=True, in_dtypes=dts)


def test_no_headline_kernel_uses_scratch_memory_and_unroll_is_lowered_until_nothing_spills():
    """fz_program_kernel_resources (the code object's metadata): every kernel fz_program_tune would try for the BASELINE
    graphs at the BASELINE shapes, and their stream-major kernels, keep everything in registers; a frame kernel whose
    prefetch buffers do not fit (3-wire frames, 4 streams per lane, 16 rows in flight) gets its unroll halved."""
    from zignal_amd.workloads import BASELINE_GRAPHS
    for name, mk in BASELINE_GRAPHS.items():
        p = F.compile(F.from_sexpr(mk()))
        for ns in (65536, 1 << 20):
            for tile in (0, p.recommended_tile_streams()):            # the library chooses per layout (time-major rows / stream tiles)
                for k, v in enumerate(p.tune_candidates(ns, 4096, tile)):
                    r = p.kernel_resources(v, ns, 4096, as_launched=True, tile_streams=tile)   # (the library's own lockstep choice steps down until it fits)
                    if k and (v.flags & F.C.FZ_VF_LOCKSTEP) and r["scratch_bytes"]:
                        continue        # a 1024-lane lockstep candidate this graph's registers do not fit: fz_program_tune skips it
                    # (vgpr_spills > 0 with no scratch bytes: values parked in accumulation registers, not in memory)
                    assert r["scratch_bytes"] == 0 and 0 < r["vgprs"] <= 512, (name, ns, tile, r)
        r = p.kernel_resources(F.make_variant(0, 0, 0, F.C.FZ_VF_STREAM_MAJOR), 1 << 20, 4096, as_launched=False)
        assert r["scratch_bytes"] == 0 and r["lds_bytes"] > 0, (name, r)
    import randgraphs as R
    p = F.compile(F.from_sexpr(R.make(1339)[0]))                 # 3 inputs, 2 outputs, 13 state rows
    v = F.make_variant(4, 32, 256)                               # (16 rows in flight fit since the state rows go through buffer descriptors: round 4)
    given, run = p.kernel_resources(v, 200, 61, as_launched=False), p.kernel_resources(v, 200, 61)
    assert given["scratch_bytes"] > 0 and given["unroll"] == 32
    assert run["scratch_bytes"] == 0 and run["unroll"] == 16 and run["vgprs"] <= 512
    assert p.kernel_name(v, 200, 61).startswith("fz_block_kernel_p4u16b256")


def test_any_host_process_builds_with_the_installations_compiler(tmp_path):
    """A process that imported PyTorch first is bound to the hiprtc / comgr bundled with the wheel (an older ROCm whose code for the
    four-streams-per-lane headline kernel needs scratch memory).  The library notices and hands every build to fz_rtc_worker -- the
    installation's hiprtc in a process of its own: same kernel symbol, same registers, byte-identical code objects under the same
    cache names with and without torch, for a graph nobody pre-built.  Only without the worker does the host's compiler build
    (under names of its own, with a warning) -- and objects the installation's compiler built are still found first."""
    import hashlib
    import shutil
    import subprocess
    import sys
    prog = (
        "import os, sys\n"
        "sys.path.insert(0, %r)\n"
        "if sys.argv[1] != 'plain': import torch\n"
        "from zignal_amd import flowz as F, workloads as G, _capi as C\n"
        "p = F.compile(F.from_sexpr(G.df1_cascade(6)))\n"
        "v = F.make_variant(4, 1, 1024, C.FZ_VF_LOCKSTEP | C.FZ_VF_GRID_SYNC | C.FZ_VF_PREFETCH3)\n"
        "r = p.kernel_resources(v, 1 << 20, 4096, as_launched=False)\n"
        "print(r['scratch_bytes'], r['vgprs'], p.kernel_name(None, 1 << 20, 4096, 0))\n"
        "q = F.compile(F.from_sexpr(G.seq(G.df1_cascade(3), G.mul(G.lit(0.37), G.IN(1)), G.df2())))\n"      # (in nobody's cache)
        "r = q.kernel_resources(None, 1 << 20, 4096)\n"
        "print(r['scratch_bytes'], r['vgprs'], q.kernel_name(None, 1 << 20, 4096, 0))\n"
    ) % os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    want_name = "fz_block_kernel_p4u1b1024f%d" % (F.C.FZ_VF_LOCKSTEP | F.C.FZ_VF_GRID_SYNC | F.C.FZ_VF_PREFETCH3)

    def run(who, cache, **extra):
        env = dict(os.environ, FLOWZ_HIP_CACHE=str(tmp_path / cache), FLOWZ_HIP_NO_PLAN_CACHE="1", **extra)
        r = subprocess.run([sys.executable, "-c", prog, who], env=env, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        files = {n: hashlib.sha1(open(tmp_path / cache / n, "rb").read()).hexdigest() for n in os.listdir(tmp_path / cache) if n.endswith(".hsaco")}
        return r.stdout.split(), files, r.stderr

    plain_out, plain_files, _ = run("plain", "a")
    torch_out, torch_files, torch_err = run("torch", "b")
    assert plain_out[0] == "0" and int(plain_out[1]) <= 128 and plain_out[2] == want_name
    assert torch_out == plain_out and torch_files == plain_files           # the same symbols, registers, file names and BYTES
    assert "warning" not in torch_err
    # without the worker: the host's compiler, under names of its own, and it says so once; pre-built objects still come first
    lib_dir = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "zignal_amd", "lib")
    moved = os.path.join(lib_dir, "fz_rtc_worker.away")
    shutil.move(os.path.join(lib_dir, "fz_rtc_worker"), moved)
    try:
        lone_out, lone_files, lone_err = run("torch", "c")
        if lone_out != plain_out:                                # (a wheel built with the installation's ROCm would not differ)
            assert "warning" in lone_err and not set(lone_files) & set(plain_files)
            both_out, both_files, _ = run("torch", "a")
            assert both_out == plain_out and set(plain_files) <= set(both_files) and all(both_files[n] == h for n, h in plain_files.items())
    finally:
        shutil.move(moved, os.path.join(lib_dir, "fz_rtc_worker"))


def test_time_major_geometry_follows_the_cu_count():
    """Plain time-major frames of many streams (host side of time_major_geometry): streams per lane x lanes per workgroup x laps are
    derived from the CU count (256 on a box without a GPU) and the measured table; counts just above whole laps run whole laps + a
    remainder launch; counts that are not a multiple of the streams per lane set the internal FZ_VF_RAGGED."""
    p = F.compile(F.from_sexpr(G.df1_cascade(6)))
    L, GS, P3 = F.C.FZ_VF_LOCKSTEP, F.C.FZ_VF_GRID_SYNC, F.C.FZ_VF_PREFETCH3      # (internal bits show as letters behind the flags: R ragged, M merging stores)
    name = lambda n: p.kernel_name(None, n, 4096, 0)                                   # noqa: E731
    assert name(1 << 18) == "fz_block_kernel_p2u4b512f%d" % (L | GS)
    assert name(3 << 17) == "fz_block_kernel_p2u2b768f%d" % (L | GS)                   # 393 216 = 256 x 768 x 2
    assert name(1 << 19) == "fz_block_kernel_p2u2b1024f%d" % (L | GS)
    assert name(3 << 18) == "fz_block_kernel_p4u1b768f%d" % (L | GS | P3)              # 786 432 = 256 x 768 x 4
    assert name(1_000_000) == "fz_block_kernel_p4u1b1024f%d" % (L | GS | P3)           # 245 workgroups of 1024 lanes
    assert name(1 << 20) == "fz_block_kernel_p4u1b1024f%d" % (L | GS | P3)
    # rows that start off the 64-byte store grid: FZ_VF_ST_MERGE (stores that let L2 merge the sectors neighbouring waves share)
    assert name((1 << 20) + 1) == "fz_block_kernel_p4u1b1024f%dM" % (L | GS | P3)       # one lap + a remainder launch of one stream: not ragged
    assert name(1_000_001) == "fz_block_kernel_p4u1b1024f%dRM" % (L | GS | P3)  # fits the workgroups: the last lane is partial
    assert name(1_000_008) == "fz_block_kernel_p4u1b1024f%dM" % (L | GS | P3) and name(1_000_016) == "fz_block_kernel_p4u1b1024f%d" % (L | GS | P3)
    assert name(1 << 21) == "fz_block_kernel_p2u2b1024f%d" % (L | GS)                  # four laps of two streams per lane (0.75 against 0.70 for two laps of four)
    assert "b1024" not in name(1 << 17) and "f%d" % (L | GS) not in name((1 << 18) - 1024)   # below one wave per SIMD and CU: the few-stream kernels
    # tiles
    assert p.kernel_name(None, 1 << 20, 4096, 8192) == "fz_block_kernel_p2u2b1024f%d" % (L | GS)        # (round 6: light graphs walk their tiles in lockstep too)
    assert p.kernel_name(None, 1 << 20, 512, 8192) == p.kernel_name(None, 1 << 20, 4096, 1024) == "fz_block_kernel_p2u16b256f%d" % F.C.FZ_VF_MAX_WG(2)
    assert F.compile(F.from_sexpr(G.osc_chain(6))).kernel_name(None, 1 << 20, 4096, 8192) == "fz_block_kernel_p2u16b256f%d" % F.C.FZ_VF_MAX_WG(2)
    # LDS rings (vectorised in time: one stream per lane, a wave on every SIMD) walk along at the geometry their rings allow since round 6: 256 lanes,
    # 16-row chunks, the resident workgroups as one lap of many; free-running on tiles, on short blocks and below CUs x 1024 streams
    ring = F.compile(F.from_sexpr(G.lds_ring_comb()))
    assert ring.kernel_name(None, 1 << 20, 4096, 0) == "fz_block_kernel_p1u16b256f%d" % (L | GS) and ring.kernel_name(None, 1 << 18, 1024, 0) == "fz_block_kernel_p1u16b256f%d" % (L | GS)
    assert ring.kernel_name(None, 1 << 20, 4096, 8192) == ring.kernel_name(None, 1 << 20, 512, 0) == ring.kernel_name(None, 1 << 17, 4096, 0) == "fz_block_kernel_p1u32b256f0"
    # wide frames (the 4-wire sum): one stream per lane in 1024-lane workgroups; one lap: one row per buffer, more: chunks of three rows
    p4 = F.compile(F.from_sexpr(G.par4_sum()))
    assert p4.kernel_name(None, 1 << 18, 4096, 0) == "fz_block_kernel_p1u1b1024f%d" % (L | GS | P3)
    assert p4.kernel_name(None, 1 << 20, 4096, 0) == "fz_block_kernel_p1u3b1024f%d" % (L | GS)
    assert p4.kernel_name(None, 1 << 16, 4096, 0) == "fz_block_kernel_p1u16b256f0" and p4.kernel_name(None, 1 << 20, 4096, 4096) == "fz_block_kernel_p1u32b256f0"
    # a register-heavy graph steps down: with many per-stream coefficients (the oscillator chain: 31) straight to one stream per lane,
    # stage-packed (packing by stages costs no registers per stream)
    assert F.compile(F.from_sexpr(G.osc_chain(6))).kernel_name(None, 1 << 20, 4096, 0) == "fz_block_kernel_p1u4b1024s6f%d" % (L | GS | F.C.FZ_VF_STAGE_PACK)
    assert F.compile(F.from_sexpr(G.osc_chain(8))).kernel_name(None, 1 << 20, 4096, 0) == "fz_block_kernel_p1u4b1024s8f%d" % (L | GS | F.C.FZ_VF_STAGE_PACK)


def test_wave_split_is_chosen_below_128_streams_per_cu_and_only_for_two_isomorphic_halves():
    """FZ_VF_WAVE_SPLIT (host side): the serial graph is cut at the middle wire of its stage split, each half is a stage-packed
    body of its own; automatic up to 32 768 streams for blocks of >= 256 samples; never for graphs with a scalar prefix /
    suffix, per-stream coefficients, several wires, an odd or a single pair of segments."""
    from zignal_amd.workloads import BASELINE_GRAPHS
    p = F.compile(F.from_sexpr(G.df1_cascade(6)))
    assert p.kernel_name(None, 32768, 4096) == "fz_block_kernel_p1u32b128w2iof33792"          # two compute waves + an I/O wave per 64 streams
    assert p.kernel_name(None, 16384, 4096) == "fz_block_kernel_p1u32b64w3iof34816"           # 256 workgroups: three compute waves of two biquads each + an I/O wave
    # one wave per SIMD (32 768 < streams <= 65 536): the stage-packed wave next to a loader and a storer (round 6: ahead in paired bursts on four boards) ...
    assert p.kernel_name(None, 65536, 4096) == p.kernel_name(None, 40960, 4096) == "fz_block_kernel_p1u16b256w1io2f%d" % (F.C.FZ_VF_IO_WAVE | F.C.FZ_VF_IO_WAVE2)
    assert p.kernel_name(None, 65536, 4096, 8192) == "fz_block_kernel_p1u16b256w1io2f%d" % (F.C.FZ_VF_IO_WAVE | F.C.FZ_VF_IO_WAVE2)
    # ... where four tuples fit a workgroup and the graph is not all arithmetic: 12 stages settle at two tuples (0.23 against 0.39 of peak) and keep the lone wave, 8 stages too
    assert F.compile(F.from_sexpr(G.df1_cascade(12))).kernel_name(None, 65536, 4096) == "fz_block_kernel_p1u16b256s8f8"
    assert F.compile(F.from_sexpr(G.df1_cascade(8))).kernel_name(None, 65536, 4096) == "fz_block_kernel_p1u16b256s8f8"
    assert F.compile(F.from_sexpr(G.df1_cascade(4))).kernel_name(None, 65536, 4096).endswith("w1io2f%d" % (F.C.FZ_VF_IO_WAVE | F.C.FZ_VF_IO_WAVE2))
    assert p.kernel_name(None, 65537, 4096).startswith("fz_block_kernel_p1u16b256s6f") and p.kernel_name(None, 65536, 200).startswith("fz_block_kernel_p1u16b256s6f")
    assert p.kernel_name(F.make_variant(1, 16, 0, F.C.FZ_VF_STAGE_PACK), 65536, 4096) == "fz_block_kernel_p1u16b256s6f8"        # the lone wave on request
    assert p.kernel_name(F.make_variant(0, 0, 0, F.C.FZ_VF_IO_WAVE), 65536, 4096) == "fz_block_kernel_p1u16b256w1iof32768"   # ... or one I/O wave next to it
    assert p.kernel_name(None, 32768, 200).startswith("fz_block_kernel_p1u16b256s6f")        # short blocks: the ends would dominate
    assert p.kernel_name(F.make_variant(0, 0, 0, 16), 32768, 4096) == "fz_block_kernel_p1u16b256f0"   # FZ_VF_NO_STAGE_PACK: the plain kernel
    src = p.source(F.make_variant(1, 16, 0, F.C.FZ_VF_WAVE_SPLIT))
    assert "namespace fz_r0 {" in src and "namespace fz_r1 {" in src and "#define FZ_WS_K0 4" in src and "#define FZ_WS_K1 4" in src   # (two segments of two atoms per part)
    r = p.kernel_resources(F.make_variant(1, 16, 0, F.C.FZ_VF_WAVE_SPLIT), 32768, 4096)
    assert r["scratch_bytes"] == 0 and r["lds_bytes"] == 2 * 8 * 64 * 16 and r["vgprs"] < 128   # two pairs x ring of 8 groups x 64 lanes x 16 B
    IO = F.C.FZ_VF_IO_WAVE
    r = p.kernel_resources(F.make_variant(0, 0, 0, IO), 65536, 4096)
    assert r["scratch_bytes"] == 0 and r["lds_bytes"] == 4 * 2 * 16 * 64 * 16                   # four (compute, I/O) pairs x two rings of 16 groups
    # what fz_program_tune measures there (round 6: only candidates some board of rounds 3-5 saw ahead): the split without its I/O wave, the single wave
    assert [v.flags for v in p.tune_candidates(32768, 4096)] == [0, F.C.FZ_VF_WAVES(2), 8]
    assert [v.flags for v in p.tune_candidates(16384, 4096)] == [0, F.C.FZ_VF_WAVES(3), 8]
    assert [v.flags for v in p.tune_candidates(65536, 4096)] == [0, 8, IO, F.C.FZ_VF_WAVES(3), 8]      # (the lone wave with 16- and 24-row chunks, one I/O wave, a packed pair per wave)
    assert sum(len(p.tune_candidates(n, 4096, t)) for n in (16384, 65536, 1 << 20) for t in (0, 8192)) <= 26
    q = F.compile(F.from_sexpr(G.df1_cascade(8)))
    assert q.kernel_name(None, 16384, 4096) == "fz_block_kernel_p1u32b64w4f3072" and "#define FZ_WS_W 4" in q.source(F.make_variant(1, 16, 0, F.C.FZ_VF_WAVES(4)))
    src = p.source(F.make_variant(1, 16, 0, IO))
    assert "#define FZ_WS_IO 1" in src and "#define FZ_WS_W 1" in src and "#define FZ_WS_K0 6" in src
    for name in ("par4_sum", "par4_sum_fanout"):
        q = F.compile(F.from_sexpr(BASELINE_GRAPHS[name]()))
        assert "w" not in q.kernel_name(None, 32768, 4096).split("b", 2)[2]
        with pytest.raises(F.FlowzError):
            q.kernel_name(F.make_variant(1, 16, 0, F.C.FZ_VF_WAVE_SPLIT), 32768, 4096)
    q = F.compile(F.from_sexpr(BASELINE_GRAPHS["osc_chain6"]()))          # scalar prefix + per-stream coefficients: they go with part 0
    assert q.kernel_name(None, 32768, 4096) == "fz_block_kernel_p1u32b128w2iof33792" and q.kernel_name(None, 16384, 4096) == "fz_block_kernel_p1u32b64w3iof34816"
    assert [q.wave_part(3, k).n_ops for k in range(3)] == [21, 18, 18] and q.wave_part(3, 0).n_param == q.n_param
    for bad in (G.df1_cascade(2), G.df1_cascade(3), G.par4_sum()):
        with pytest.raises(F.FlowzError):
            F.compile(F.from_sexpr(bad)).kernel_name(F.make_variant(1, 16, 0, F.C.FZ_VF_WAVE_SPLIT), 4096, 4096)


def test_wave_parts_with_prefix_suffix_and_per_stream_coefficients_compose():
    """a scalar prefix (an oscillator, an odd first stage) goes with the first part, a scalar suffix (output gain, smoothing
    one-pole) with the last, per-stream coefficients with whoever reads them: the parts' IR composed == the oracle"""
    ns = 3
    cases = {"osc6": G.osc_chain(6), "c6gain": G.seq(G.df1_cascade(6), G.mul(G.lit(0.7), G.IN(1))), "c7": G.df1_cascade(7),
             "int_c4_gain": G.seq(G.fb(G.add(G.mul(G.lit(0.5), G.DEL(1, 1)), G.IN(2))), G.seq(G.df1_cascade(4), G.mul(G.IN(1), G.lit(1.5)))),
             "c4_onepole": G.seq(G.df1_cascade(4), G.fb(G.add(G.mul(G.lit(0.5), G.DEL(1, 1)), G.mul(G.lit(0.5), G.IN(2)))))}
    for name, g in cases.items():
        p = F.compile(F.from_sexpr(g))
        P = W.osc_chain_params(5, np.arange(ns)) if p.n_param else None
        x = O.synth_input(3, np.arange(ns), 60)
        want = O.compile(g, ns, params=P).run(x)
        done = 0
        for Wn in (2, 3):
            try:
                parts = [p.wave_part(Wn, k) for k in range(Wn)]
            except F.FlowzError:
                continue
            y = x
            for q in parts:
                y, _ = run_ir(q, y, params=P)
            assert np.array_equal(y.view(np.uint32), want.view(np.uint32)) and sum(q.n_ops for q in parts) == p.n_ops, (name, Wn)
            done += 1
        assert done >= 1, name


@pytest.mark.parametrize("seed", range(12))
def test_wave_parts_compose_to_the_whole_graph(seed):
    """find_wave_roles on the GPU-less box: fz_program_wave_part hands out every part of every split as a program of its own;
    their lowered IR, evaluated one after the other through the test interpreter, is the oracle of the whole graph bit for bit;
    the parts share the operations of the graph exactly, and each is stage-packable by itself."""
    rng = np.random.default_rng(9500 + seed)
    form = ["df1", "df2", "df1t"][seed % 3]
    n = [4, 6, 8, 10, 12, 16][seed % 6]

    def stage():
        if form == "df1t":
            return G.df1t()
        r, th = rng.uniform(0.3, 0.95), rng.uniform(0.1, 3.0)
        c = (rng.uniform(0.1, 1.0), rng.uniform(-1, 1), rng.uniform(-1, 1), 2 * r * np.cos(th), -r * r)
        return (G.df1 if form == "df1" else G.df2)(*[float(np.float32(v)) for v in c])

    g = stage()
    for _ in range(n - 1):
        g = G.seq(g, stage())
    p = F.compile(F.from_sexpr(g))
    x = O.synth_input(seed, np.arange(3), 70)
    want = O.compile(g, 3).run(x)
    splits = 0
    for W in (1, 2, 3, 4):
        try:
            parts = [p.wave_part(W, k) for k in range(W)]
        except F.FlowzError:
            continue
        assert sum(q.n_ops for q in parts) == p.n_ops and all(q.stage_packable and (q.n_in, q.n_out) == (1, 1) for q in parts)
        y = x
        for q in parts:
            y, _ = run_ir(q, y)
        assert np.array_equal(y.view(np.uint32), want.view(np.uint32)), (form, n, W)
        splits += 1
    assert splits >= 2                                    # at least the whole graph (I/O wave) and two parts
    with pytest.raises(F.FlowzError):
        p.wave_part(2, 2)
    with pytest.raises(F.FlowzError):
        F.compile(F.from_sexpr(G.par4_sum())).wave_part(2, 0)


def test_sample_rate_modulators_lower_like_the_oracle():
    """fz_modulator: the std::ref terminal at sample rate (flowz/README.md:42-61).  Lowered IR == oracle; the graph is never
    stage-packed; launching without a modulation array is refused."""
    rng = np.random.default_rng(3)
    x = O.synth_input(4, np.arange(5), 40)
    m = rng.uniform(-0.9, 0.9, (2, 40)).astype(np.float32)
    for g in (G.one_pole_modulated(), G.modulated_mix(), G.seq(G.df1_cascade(4), G.mul(G.mod(1), G.IN(1)))):
        p = F.compile(F.from_sexpr(g))
        assert p.n_mod == (1 if g == G.one_pole_modulated() else 2) and p.stage_packable == 0
        want = O.compile(g, 5).run(x, mod=m)
        got, _ = run_ir(p, x, mod=m)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # per-call semantics of the reference: the same as calling sample by sample with the variable changed in between
    f = O.compile(G.one_pole_modulated(), 1)
    ys = [f.step(1.0, mod=[a])[0][0] for a in (0.5, 0.25, -0.5)]
    assert ys == [1.0, 1.25, 0.375]
    with pytest.raises(F.FlowzError):                     # a graph without modulators takes no modulation array
        plain = F.compile(F.from_sexpr(G.df1()))
        _capi.check(_capi.lib.fz_program_set_modulation(plain._h, None, 16))


def test_kernel_symbols_keep_graphs_apart_in_a_profile():
    """The symbol in the code object is the variant's name + a tag of the graph's structure: two graphs that run the same variant are two
    rows of `rocprofv3 --stats` (the bench line's roofline.kernel is such a symbol); graphs that differ in coefficient VALUES only share it
    (and the code object: the values travel in the kernarg)."""
    import re
    a, b = F.compile(F.from_sexpr(G.df1_cascade(6))), F.compile(F.from_sexpr(G.df1()))
    na, nb = a.kernel_name(None, 1 << 20, 4096, 0), b.kernel_name(None, 1 << 20, 4096, 0)
    sa, sb = a.kernel_symbol(None, 1 << 20, 4096, 0), b.kernel_symbol(None, 1 << 20, 4096, 0)
    assert na == nb and sa != sb
    assert re.fullmatch(re.escape(na) + r"_g[0-9a-f]{8}", sa) and sb.startswith(nb + "_g")
    c = F.compile(F.from_sexpr(G.df1_cascade(6, coeffs=[(0.3, 0.1, 0.05, 0.2, -0.1)] * 6)))
    assert c.kernel_symbol(None, 1 << 20, 4096, 0) == sa
    assert sa in a.source(F.make_variant(4, 1, 1024, F.C.FZ_VF_LOCKSTEP | F.C.FZ_VF_GRID_SYNC | F.C.FZ_VF_PREFETCH3))


def test_launch_rejects_stream_counts_its_descriptors_cannot_address():
    """State and coefficient rows go through one-row buffer descriptors (32-bit sizes and offsets): 2^30 streams and more are refused --
    on tiles and stream-major buffers too, where the row check of plain time-major frames does not catch them (checked before any device
    is touched: the pointers here are never dereferenced)."""
    p = F.compile(F.from_sexpr(G.df1_cascade(2)))
    fake = ctypes.c_void_p(1 << 20)                                   # 16-byte aligned, never read
    for ns, tile, flags in ((1 << 30, 8192, 0), (1 << 31, 8192, 0), (1 << 30, 0, _capi.FZ_VF_STREAM_MAJOR), ((1 << 30) + 8192, 8192, 0)):
        with pytest.raises(F.FlowzError) as e:
            if flags:
                _capi.check(_capi.lib.fz_run_block_stream_major(p._h, fake, fake, fake, None, ns, 4096, 0, 4096, ctypes.byref(F.make_variant(0, 0, 0, flags)), None))
            else:
                p.run_block_ptr(fake, fake, fake, None, ns, 64, tile_streams=tile)
        assert e.value.code == _capi.FZ_E_UNSUPPORTED and "2^30" in str(e.value), str(e.value)


def test_expression_recipes_round_trip():
    """An expression serialised (what a kernel manifest records of a program) and parsed back lowers to the same DAG, coefficient values
    included: named graphs, typed graphs, 120 random ones."""
    import randgraphs as R
    cases = [(G.df1_cascade(6), False), (G.par4_sum(), False), (G.osc_chain(6), False), (G.cross_wire(), False), (G.df2t(), False),
             (G.mixed_precision_biquad(), True), (G.complex_mix(), True), (("seq", ("in", 1), ("add", ("del", 1, 40), ("del", 1, 5000))), False)]
    cases += [(R.make(seed)[0], False) for seed in range(80)] + [(R.make_typed(seed)[0], True) for seed in range(40)]
    lib = _capi.lib
    lib.fz_expr_recipe.restype = ctypes.c_long
    lib.fz_expr_recipe.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
    lib.fz_expr_from_recipe.restype = ctypes.c_void_p
    lib.fz_expr_from_recipe.argtypes = [ctypes.c_char_p]
    for g, typed in cases:
        e = F.from_sexpr(g)
        n = lib.fz_expr_recipe(e._h, None, 0)
        buf = ctypes.create_string_buffer(n + 1)
        lib.fz_expr_recipe(e._h, buf, n + 1)
        h = lib.fz_expr_from_recipe(buf.value)
        assert h, _capi.lib.fz_last_error()
        e2 = F.Expr(h)
        assert (e2.ins, e2.outs) == (e.ins, e.outs)
        a, b = F.compile(e, typed=typed), F.compile(e2, typed=typed)
        assert a.ir() == b.ir() and a.lines() == b.lines() and a.outputs() == b.outputs() and a.consts() == b.consts(), g
    assert not lib.fz_expr_from_recipe(b"A 0 0 1\n") and not lib.fz_expr_from_recipe(b"Z 1\n") and not lib.fz_expr_from_recipe(b"")


def test_kernel_manifest_records_and_replays_without_a_gpu(tmp_path):
    """FLOWZ_HIP_MANIFEST records (expression, input types, variant) of every kernel a process resolves; fz_manifest_build rebuilds them
    into an empty kernel cache in parallel compiler processes: the same code objects, byte for byte; a second replay finds them all."""
    import subprocess
    import sys
    man, c1, c2 = tmp_path / "m.fzm", tmp_path / "c1", tmp_path / "c2"
    code = ("from zignal_amd import flowz as F, workloads as W\n"
            "p = F.compile(F.from_sexpr(W.df1_cascade(6))); p.build(None, 1 << 20, 4096); p.build(None, 65536, 4096); p.build(None, (1 << 20) + 1, 4096)\n"
            "q = F.compile(F.from_sexpr(W.complex_one_pole()), typed=True); q.build(None, 1 << 20, 4096)\n"
            "r = F.compile(F.from_sexpr(W.lds_ring_comb())); r.build(F.make_variant(1, 32, 256))\n")
    env = dict(os.environ, FLOWZ_HIP_CACHE=str(c1), FLOWZ_HIP_MANIFEST=str(man))
    subprocess.check_call([sys.executable, "-c", code], env=env, cwd=ROOT)
    first = sorted(f.name for f in c1.glob("*.hsaco"))
    assert len(first) >= 6                                           # (1 048 577 streams: the lap's kernel AND the remainder launch's, pre-built by build_for)
    env = dict(os.environ, FLOWZ_HIP_CACHE=str(c2))
    out = subprocess.check_output([sys.executable, "-c", f"from zignal_amd import flowz as F; print(F.manifest_build({str(man)!r}, 4)); print(F.manifest_build({str(man)!r}, 4))"],
                                  env=env, cwd=ROOT, text=True).splitlines()
    a, b = eval(out[0]), eval(out[1])
    assert a["failed"] == 0 and a["built"] == a["records"] >= len(first) and a["at_hand"] == 0, a
    assert b["at_hand"] == b["records"] and b["built"] == 0, b
    assert sorted(f.name for f in c2.glob("*.hsaco")) == first
    for f in first:
        assert (c1 / f).read_bytes() == (c2 / f).read_bytes(), f
    # a manifest is data from elsewhere (round-5 advisor finding): records with a variant no launch could have resolved (P = 0 would divide by
    # zero, a block that is no multiple of 64) are counted as failed and skipped; a record whose length runs past the file is refused
    text = man.read_bytes()
    head, _, rest = text.partition(b"\n")
    f = head.split()
    bad = tmp_path / "bad.fzm"
    bad.write_bytes(b" ".join([f[0], b"0"] + f[2:]) + b"\n" + rest[:int(f[5])] + b" ".join(f[:3] + [b"100"] + f[4:]) + b"\n" + rest[:int(f[5])] + text)
    r = F.manifest_build(str(bad), 2)
    assert r["failed"] == 2 and r["records"] == a["records"] + 2 and r["at_hand"] + r["built"] == a["records"], r
    bad.write_bytes(b" ".join(f[:5] + [b"18446744073709551000"]) + b"\n" + rest)
    with pytest.raises(F.FlowzError):
        F.manifest_build(str(bad), 2)


def test_typed_frames_take_lane_pairs(tmp_path, monkeypatch):
    """Round 5: a lane of four streams whose output slice would leave as TWO 16-byte stores (typed frames: 8 bytes per stream) takes two
    PAIRS of streams 128 apart instead -- every store instruction then writes whole 32-byte sectors and the frames are written through like
    all others (0.76 against 0.68 of peak for the complex one-pole in lockstep).  Internal flag, letter L in the kernel name; not for float
    frames, not when the waves are not whole."""
    import subprocess
    from zignal_amd import workloads as ZW
    monkeypatch.setenv("FLOWZ_HIP_CACHE", str(tmp_path))
    L, GS, P3 = F.C.FZ_VF_LOCKSTEP, F.C.FZ_VF_GRID_SYNC, F.C.FZ_VF_PREFETCH3
    for g in (ZW.complex_one_pole(), ZW.df1_double()):
        p = F.compile(F.from_sexpr(g), typed=True)
        assert p.kernel_name(None, 1 << 20, 4096) == "fz_block_kernel_p4u1b1024f%dL" % (L | GS | P3)
        assert p.kernel_name(F.make_variant(4, 8, 256), 1 << 20, 4096) == "fz_block_kernel_p4u8b256f0L"
        assert p.kernel_name(F.make_variant(4, 8, 256), (1 << 20) + 4, 4096) == "fz_block_kernel_p4u8b256f0M"       # not whole waves of 256 streams (and rows off the 64-byte grid: M)
        assert p.kernel_name(F.make_variant(2, 16, 256), 1 << 20, 4096) == "fz_block_kernel_p2u16b256f0"           # two streams per lane: one 16-byte store as it is
    assert F.compile(F.from_sexpr(G.df1_cascade(6))).kernel_name(None, 1 << 20, 4096).endswith("f%d" % (L | GS | P3))   # float frames: one b128 per lane already
    p = F.compile(F.from_sexpr(ZW.complex_one_pole()), typed=True)
    p.build(F.make_variant(4, 8, 256), 1 << 20, 4096)
    obj = tmp_path / (p.kernel_code_id(F.make_variant(4, 8, 256), 1 << 20, 4096) + ".hsaco")      # (the code id IS the cache file's name)
    dis = subprocess.check_output(["/opt/rocm/lib/llvm/bin/llvm-objdump", "-d", str(obj)], text=True)
    h = _main_loop_histogram(dis)
    # per step: the lane's two pairs as two 8-byte loads (4 bytes per stream in) and two 16-byte stores (8 bytes per stream out), nothing narrower
    assert h["buffer_load_dwordx2"] == h["buffer_store_dwordx4"] == 32 and "buffer_store_dwordx2" not in h and "buffer_store_dword" not in h, h
    assert " nt sc1" in [ln for ln in dis.splitlines() if "buffer_store_dwordx4" in ln][0]                              # written through, like every whole-sector frame store


def test_a_wheel_imported_after_the_library_does_not_lend_it_its_compiler(tmp_path):
    """The library imported first, PyTorch (which bundles an older comgr) after it, the first kernel built after that: hiprtc would load the
    compiler that is already in the process.  The library notices the foreign comgr and builds in the compiler worker -- the same kernel as
    a process without torch settles on (with the wheel's compiler the pair long-run body of the oscillator chain spills and steps down) --
    and loads nothing into the host process: the only comgr mapped afterwards is still the wheel's, so the wheel's libraries keep theirs."""
    import subprocess
    import sys
    code = ("from zignal_amd import flowz as F\nimport torch, os\nfrom zignal_amd import workloads as W\n"
            "print(F.compile(F.from_sexpr(W.osc_chain(6))).kernel_name(F.make_variant(0, 0, 0, F.C.FZ_VF_STREAM_MAJOR), 1 << 20, 4096))\n"
            "print(sorted({os.path.realpath(l.split()[-1]) for l in open('/proc/self/maps') if 'libamd_comgr' in l}))\n")
    out = subprocess.check_output([sys.executable, "-c", code], env=dict(os.environ, FLOWZ_HIP_CACHE=str(tmp_path)), cwd=ROOT, text=True).splitlines()
    assert out[-2].split()[-1] == "fz_block_kernel_p2u64b64f384", out
    mapped = eval(out[-1])
    assert mapped and all("/torch/" in m for m in mapped), mapped
