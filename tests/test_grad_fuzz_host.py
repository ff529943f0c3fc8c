"""The fuzz cells of the backward (tests/grad_fuzz_cells.py) without a GPU: every cell resolves to the kernels pinned for it
(tests/golden/grad_fuzz_pins.json; `python tests/grad_fuzz_cells.py` rewrites it), the set covers what the adjoint kernels are
parametrised over, tests/adjoint_ref.py -- what test_grad_fuzz_gpu.py holds the kernels to -- agrees with float64 autograd and central
differences on them, the GPU test's inputs put a signal on every adjoint, both kernels of every cell compile for gfx950 without
scratch, and the kernel manifest next to the pins builds all of them."""
import os
import subprocess
import sys

import numpy as np
import pytest

import adjoint_ref as A
import grad_fuzz_cells as GC
import grad_graphs as GG
from grad_host_harness import ADJOINT, ADJOINT_SM, HERE, ROOT, code_objects, fd_check, inputs as smooth_inputs, replay, write_manifest
from zignal_amd import _capi as C
from zignal_amd import flowz as F

F32 = np.float32
PINS = GC.load_pins()
N_CHUNKS = 8
KEYS = ("x", "state", "params", "consts")
CR_PAIRS = {(2, 8), (4, 32), (8, 32), (16, 16), (16, 32), (2, 16), (4, 8), (4, 16), (8, 8), (8, 16)}
# every node kind adjoint_takes accepts (fz_codegen.cpp), by the names of Program.ir()
ADJOINT_KINDS = ("input", "const", "param", "delay", "add", "sub", "mul", "div", "neg", "lt", "le", "gt", "ge", "eq", "ne", "abs", "sqrt", "exp", "tanh",
                 "min", "max")


def test_every_cell_is_pinned_and_no_pin_is_left_over():
    assert set(PINS) == set(GC.CELLS) and len(GC.CELLS) <= 48


def test_the_committed_selection_is_what_the_rule_selects():
    assert GC.select() == GC.SELECTED


def test_the_stride_cells_are_the_c1_cell_and_a_depth_8_cell():
    c1, deep = GC.STRIDE_CELLS
    assert GC.strides(GC.prog(c1))[0] == 1 and GC.strides(GC.prog(deep))[0] not in (1, 4)
    assert "depth8" in GC.features(GC.prog(deep)) and deep not in GC.CRAFTED


def test_cells_resolve_to_their_pinned_symbols_and_sizes():
    for cell in GC.CELLS:
        got = GC.resolved(cell)
        assert got == {k: PINS[cell][k] for k in got}, (cell, got, PINS[cell])


def test_the_crafted_graphs_are_what_they_are_for():
    p = GC.prog("cascade9_depth8")
    assert p.n_state == 72 and p.grad_kernel_symbol().startswith("fz_adjoint_kernel_c1b") and GC.strides(p)[0] == 1
    p = GC.prog("no_delay_line")
    assert p.n_state == 0 and p.grad_workspace_bytes(1000, 100) == 0
    p = GC.prog("passes_input_and_delayed_input")
    assert [p.ir()[o][0] for o in p.outputs()] == ["input", "delay"]
    p = GC.prog("generator_without_input")                       # (the backward takes a graph without an input wire)
    assert p.n_in == 0 and p.n_param == 1 and C.lib.fz_program_grad_check(p._h) == C.FZ_OK, C.last_error()


def test_the_cells_cover_what_the_adjoint_kernels_are_parametrised_over(capsys):
    classes, feats, kinds, refused, shapes = {}, {}, {}, [], set()
    named = {GC.strides(F.compile(F.from_sexpr(b()))) for b in GG.SUPPORTED.values()}
    for cell in GC.CELLS:
        p = GC.prog(cell)
        c, r = GC.strides(p)
        classes.setdefault((c, r), []).append(cell)
        shapes.add((c, r, p.n_in, p.n_out))
        if r is None:
            refused.append(cell)
        for f in GC.features(p):
            feats.setdefault(f, []).append(cell)
        for k in GC.kinds(p):
            kinds[k] = kinds.get(k, 0) + 1
    with capsys.disabled():
        print("\n(C, R) classes of the fuzz cells (* = no named graph of grad_graphs.py compiles it):")
        for cr in sorted(classes, key=str):
            print(f"  C={cr[0]:<2} R={cr[1]!s:<4} {len(classes[cr]):2} cells{' *' if cr not in named else ''}")
        print(f"  {len(shapes)} distinct (C, R, n_in, n_out); n_in 0..{max(s[2] for s in shapes)}, n_out 1..{max(s[3] for s in shapes)}")
        print("features:", ", ".join(f"{f} {len(feats.get(f, []))}" for f in GC.FEATURES))
        print("node kinds:", ", ".join(f"{k} {kinds.get(k, 0)}" for k in ADJOINT_KINDS))
    assert {c for c, _ in classes} == {1, 2, 4, 8, 16}
    assert CR_PAIRS <= set(classes), CR_PAIRS - set(classes)
    assert all(len(feats.get(f, [])) >= 1 for f in GC.FEATURES), {f: len(feats.get(f, [])) for f in GC.FEATURES}
    assert all(kinds.get(k, 0) >= 2 for k in ADJOINT_KINDS), kinds
    assert set(kinds) <= set(ADJOINT_KINDS), set(kinds) - set(ADJOINT_KINDS)
    # cells whose stream-major patch does not fit the LDS run the time-major kernel only (the GPU test asserts the refusal): a few at most
    assert len(refused) <= 3, refused
    assert any(GC.prog(c).n_in == 0 for c in GC.CELLS) and any(GC.prog(c).n_state == 0 for c in GC.CELLS)
    assert max(d for c in GC.CELLS for _, d in GC.prog(c).lines()) == 8


_worst = {}


@pytest.mark.parametrize("part", range(N_CHUNKS))
def test_restatement_matches_float64_autograd(part, capsys):
    """the bound of test_grad_host.test_reference_matches_float64_autograd: relative error <= 1e-4 per tensor.  Continuous random inputs:
    no sample sits on a tie of ABS / MIN / MAX or a comparison"""
    ns, T = 4, 64
    for cell in GC.CELLS[part::N_CHUNKS]:
        p = GC.prog(cell)
        x, s0, _, yb, sb = smooth_inputs(p, ns, T, 11)
        par = GC.draw_params(p, ns, np.random.default_rng(7))
        got, want = A.grad(p, x, yb, s0, par, sb), A.torch_grad(p, x, yb, s0, par, sb)
        for k in KEYS:
            if np.asarray(want[k]).size == 0:
                continue
            e = A.rel_err(got[k][:want[k].shape[0]] if k != "x" else got[k], want[k])
            if e > _worst.get(k, (0.0, ""))[0]:
                _worst[k] = (e, cell)
            assert e <= 1e-4, (cell, k, e)
    with capsys.disabled():
        print(f"\nrestatement against float64 autograd, worst relative error so far (part {part}):", {k: (f"{e:.2e}", c) for k, (e, c) in _worst.items()})


def fd_cells():
    """six cells for the central differences: the C = 1 cascade, a random graph with a line of depth 8, the graph without state, the one
    without input, and two more random ones without a tie to sit on"""
    smooth = [c for c in GC.CELLS if c not in GC.CRAFTED and not GC.has_ties(GC.prog(c))]
    deep = [c for c in smooth if "depth8" in GC.features(GC.prog(c))]
    rest = [c for c in smooth if c not in deep[:1] and GC.prog(c).n_param]
    return ["cascade9_depth8", deep[0], "no_delay_line", "generator_without_input", rest[0], smooth[0]]


@pytest.mark.parametrize("k", range(6))
def test_restatement_matches_central_differences(k):
    cell = fd_cells()[k]
    p = GC.prog(cell)
    ns, T = 3, 24
    x, s0, _, yb, sb = smooth_inputs(p, ns, T, 5)
    fd_check(p, x, s0, GC.draw_params(p, ns, np.random.default_rng(1)), yb, sb)


@pytest.mark.parametrize("part", range(N_CHUNKS))
def test_the_gpu_tests_inputs_put_a_signal_on_every_adjoint(part):
    """grad_fuzz_cells.signal_gaps: with the GPU test's inputs of the longest block, every input wire, state row, parameter and coefficient
    an adjoint reaches gets a finite one that is not zero in every stream without a NaN or infinity: a dropped contribution changes bits"""
    for cell in GC.CELLS[part::N_CHUNKS]:
        assert not GC.signal_gaps(cell), (cell, GC.signal_gaps(cell))


@pytest.mark.parametrize("part", range(N_CHUNKS))
def test_both_adjoint_kernels_jit_compile_without_scratch_or_vgpr_spills(part, capsys):
    """scratch_bytes == 0 and vgpr_spills == 0 for both kernels of every cell; sgpr_spills are printed next to the recorded ones (they
    follow the compiler's register allocation: tests/golden/grad_fuzz_pins.json records, nothing asserts them)"""
    lines = []
    for cell in GC.CELLS[part::N_CHUNKS]:
        p = GC.prog(cell)
        c, r = GC.strides(p)
        tm = p.grad_resources()
        assert tm["scratch_bytes"] == 0 and tm["vgpr_spills"] == 0 and tm["unroll"] == c, (cell, tm)
        now = [tm["sgpr_spills"], None]
        if r is None:
            with pytest.raises(F.FlowzError) as ei:
                p.grad_resources(stream_major=True)
            assert ei.value.code == C.FZ_E_UNSUPPORTED and "does not fit the LDS" in str(ei.value)
        else:
            sm = p.grad_resources(stream_major=True)
            assert sm["scratch_bytes"] == 0 and sm["vgpr_spills"] == 0 and sm["unroll"] == c, (cell, sm)
            assert sm["lds_bytes"] == 4 * 64 * (r * (p.n_in + p.n_out) + 4) * 4 <= 160 * 1024
            now[1] = sm["sgpr_spills"]
        lines.append(f"  {cell:32} C={c:<2} R={r!s:<4} sgpr_spills time-major {now[0]:3}, stream-major {now[1]!s:>4}   (recorded {PINS[cell]['sgpr_spills']})")
    with capsys.disabled():
        print("\n" + "\n".join(lines))


def test_the_wide_frame_graph_that_once_spilled_vgprs_does_not():
    """make_cmp_grad(13), 3 in / 2 out at C = 4, R = 16: with all 12 + 8 float4 pieces of a patch in flight its stream-major kernel took
    306 registers, 48 of them spilled; no cell now (its inputs leave a coefficient without a signal), so it is held here"""
    p = GC.prog("cmp13")
    assert GC.strides(p) == (4, 16) and (p.n_in, p.n_out) == (3, 2)
    r = p.grad_resources(stream_major=True)
    assert r["scratch_bytes"] == 0 and r["vgpr_spills"] == 0 and r["vgprs"] + r["agprs"] <= 256, r


def test_the_manifest_of_the_cells_builds_every_adjoint_kernel(tmp_path):
    """tests/golden/grad_fuzz_kernels.fzm.gz (recorded on a CPU: grad_fuzz_cells.kernel_requests, both kernels of every cell and of every
    grad_graphs.SUPPORTED graph) replayed into an empty cache: nothing fails, and resolving them all afterwards builds nothing more"""
    r = replay(GC.MANIFEST, {"FLOWZ_HIP_CACHE": str(tmp_path)})
    objects = sorted(code_objects(tmp_path))
    code = ("import sys\nsys.path[:0] = [%r, %r]\nfrom zignal_amd import flowz as F\nimport grad_fuzz_cells as GC\n"
            "n = 0\n"
            "for p, c, sm in GC.kernel_requests():\n"
            "    try:\n        p.grad_resources(c, stream_major=sm); n += 1\n    except F.FlowzError:\n        pass\n"
            "print(n)\n") % (ROOT, HERE)
    env = {k: v for k, v in os.environ.items() if k != "FLOWZ_HIP_MANIFEST"}
    n = int(subprocess.check_output([sys.executable, "-c", code], env=dict(env, FLOWZ_HIP_CACHE=str(tmp_path)), cwd=ROOT, text=True).splitlines()[-1])
    assert r["failed"] == 0 and r["at_hand"] + r["built"] == r["records"] >= 2 * len(GC.CELLS), r
    assert sorted(code_objects(tmp_path)) == objects and len(objects) <= n


def test_a_manifest_with_adjoint_variants_nobody_could_have_made_builds_only_the_sound_ones(tmp_path):
    """a manifest is data from elsewhere: stream-major adjoint records with patch rows that are no power of two, a checkpoint stride beyond
    32, a patch this graph's frames do not fit, a forward flag mixed in, or a time-major one with P = 2 are counted as failed, not built"""
    import gzip
    import re
    text = gzip.open(GC.MANIFEST, "rb").read()
    m = None
    for m in re.finditer(rb"FZM1 (\d+) (\d+) 256 (\d+) (\d+)\n", text):
        if int(m.group(3)) == ADJOINT | ADJOINT_SM and int(m.group(1)) == 16:       # a stream-major record with R = 16: two wires at least
            break
    P, U, flags, n = (int(x) for x in m.groups())
    assert flags == ADJOINT | ADJOINT_SM and P == 16
    recipe = text[m.end():m.end() + n]
    rec = lambda P_, U_, f_, block=256: (P_, U_, block, f_, recipe)   # noqa: E731
    bad = [rec(3, U, flags), rec(P, 64, flags), rec(128, U, flags), rec(P, U, flags | 256), rec(2, U, ADJOINT), rec(P, U, flags, 128), rec(P, 3, flags)]
    write_manifest(tmp_path / "bad.fzm", bad + [rec(P, U, flags)])
    r = replay(tmp_path / "bad.fzm", {"FLOWZ_HIP_CACHE": str(tmp_path / "cache")}, jobs=2)
    assert r["records"] == len(bad) + 1 and r["failed"] == len(bad) and r["built"] + r["at_hand"] == 1, r
    assert len(code_objects(tmp_path / "cache")) == 1
