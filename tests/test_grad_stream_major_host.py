"""The backward on stream-major buffers without a GPU (fz_run_block_grad_stream_major): the exports, the stream-major adjoint kernel's
JIT for gfx950 (no scratch, no spills, a symbol of its own that names C and R), the per-layout inspection calls, the refusals, the
argument checks, and the time-major adjoint kernel's text and symbol held to what they were before the stream-major kernel existed."""
import ctypes
import os
import re

import pytest

import grad_graphs as GG
from grad_host_harness import FakeCall, code_pins, empty_args, invalid
from zignal_amd import _capi as C
from zignal_amd import flowz as F

HERE = os.path.dirname(os.path.abspath(__file__))
NEW_EXPORTS = ("fz_run_block_grad_stream_major", "fz_program_grad_resources_for", "fz_program_grad_kernel_symbol_for", "fz_program_grad_source_for")


def prog_of(name):
    return F.compile(F.from_sexpr(GG.SUPPORTED[name]()))


def test_the_new_entry_points_are_declared_and_exported():
    header = open(os.path.join(HERE, "..", "include", "flowz_hip.h")).read()
    for name in NEW_EXPORTS:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in C.EXPORTS and getattr(C.lib, name)
    assert re.search(r"FZ_GRAD_TIME_MAJOR\s*=\s*0\b", header) and re.search(r"FZ_GRAD_STREAM_MAJOR\s*=\s*1\b", header)


@pytest.mark.parametrize("name", sorted(GG.SUPPORTED))
def test_stream_major_adjoint_kernel_jit_compiles_without_scratch_or_spills(name):
    p = prog_of(name)
    r = p.grad_resources(stream_major=True)
    assert r["scratch_bytes"] == 0 and r["vgpr_spills"] == 0 and r["sgpr_spills"] == 0, r
    sym, tm = p.grad_kernel_symbol(stream_major=True), p.grad_kernel_symbol()
    assert sym != tm
    m = re.fullmatch(r"fz_adjoint_sm_kernel_c(\d+)r(\d+)b256_g([0-9a-f]{8})", sym)
    assert m, sym
    c, rows = int(m.group(1)), int(m.group(2))
    # the same default stride and graph tag as the time-major kernel; the patch a multiple of the stride and of 4 rows
    assert tm == f"fz_adjoint_kernel_c{c}b256_g{m.group(3)}"
    assert r["unroll"] == c and rows % c == 0 and rows % 4 == 0
    # the patches of the workgroup's four waves: [64 streams][rows x (n_in + n_out) + 4 floats], within what one workgroup may declare
    assert r["lds_bytes"] == 4 * 64 * (rows * (p.n_in + p.n_out) + 4) * 4 <= 160 * 1024
    if name in ("df1_cascade6", "moog_ladder"):
        for cr in (1, 4):
            rc = p.grad_resources(cr, stream_major=True)
            assert rc["scratch_bytes"] == 0 and rc["unroll"] == cr
            assert p.grad_kernel_symbol(cr, stream_major=True).startswith(f"fz_adjoint_sm_kernel_c{cr}r")


@pytest.mark.parametrize("name", ["df1_cascade6", "moog_ladder", "rules"])
def test_layout_zero_answers_what_the_existing_functions_answer(name):
    p = prog_of(name)
    for cr in (0, 1, 4):
        a, b = C.KernelResources(), C.KernelResources()
        assert C.lib.fz_program_grad_resources(p._h, cr, ctypes.byref(a)) == C.FZ_OK
        assert C.lib.fz_program_grad_resources_for(p._h, cr, 0, ctypes.byref(b)) == C.FZ_OK
        assert bytes(a) == bytes(b)
        s1, s2 = ctypes.create_string_buffer(160), ctypes.create_string_buffer(160)
        n1 = C.lib.fz_program_grad_kernel_symbol(p._h, cr, s1, 160)
        n2 = C.lib.fz_program_grad_kernel_symbol_for(p._h, cr, 0, s2, 160)
        assert n1 == n2 > 0 and s1.value == s2.value
    r = C.KernelResources()
    assert C.lib.fz_program_grad_resources_for(p._h, 0, 2, ctypes.byref(r)) == C.FZ_E_INVALID
    assert C.lib.fz_program_grad_kernel_symbol_for(p._h, 0, 7, None, 0) == C.FZ_E_INVALID


def test_the_two_kernels_have_texts_of_their_own():
    p = prog_of("df1_cascade6")
    tm, sm = p.grad_source(), p.grad_source(stream_major=True)
    assert "fz_adj_sm_args" in sm and "FZ_R" in sm and "fz_adj_sm_args" not in tm and "FZ_R" not in tm
    # the generated body is the same text in both: the order of operations is one
    body = lambda s: s.split("// ==== fz_graph_body.h ====\n")[1].split("// ==== fz_block_kernel.hip.inc ====\n")[0]
    assert body(tm) == body(sm)
    assert "fz_adj" not in p.source()


@pytest.mark.parametrize("name", ["df1_cascade6", "moog_ladder"])
def test_time_major_adjoint_kernel_text_and_symbol_are_the_parents(name):
    """tests/golden/adjoint_code_pins.json holds the kernel's symbol and the hashes of its code; test_adjoint_code_pins_host.py holds the
    code the library builds now to them"""
    pin = code_pins()["adjoint/tm/" + name]
    assert prog_of(name).grad_kernel_symbol() == pin["symbol"] and all(len(pin[s]) == 64 for s in (".text", ".rodata", ".note"))


@pytest.mark.parametrize("name", sorted(GG.REFUSED))
def test_refusals_are_the_time_major_refusals(name):
    build, typed, word = GG.REFUSED[name]
    p = F.compile(F.from_sexpr(build()), typed=typed)
    a = empty_args()
    assert C.lib.fz_run_block_grad(p._h, ctypes.byref(a), 64, 16, None) == C.FZ_E_UNSUPPORTED
    why_tm = C.last_error()
    assert C.lib.fz_run_block_grad_stream_major(p._h, ctypes.byref(a), 64, 16, 0, 16, None) == C.FZ_E_UNSUPPORTED
    assert C.last_error() == why_tm and word.lower() in why_tm.lower()
    with pytest.raises(F.FlowzError) as ei:
        p.grad_kernel_symbol(stream_major=True)
    assert ei.value.code == C.FZ_E_UNSUPPORTED and word.lower() in str(ei.value).lower()
    with pytest.raises(F.FlowzError) as ei:
        p.grad_resources(stream_major=True)
    assert ei.value.code == C.FZ_E_UNSUPPORTED


# ---- argument checks: every one fails before the device is needed ----------------------------------------------------------------
def test_argument_checks():
    p = prog_of("df1_cascade_params6")                            # 1 in, 1 out
    b = FakeCall(p, 1000, 37, window=(48, 0))
    assert invalid(b.run(b.args(), rows=47), "rows_total")        # rows_total * n_in and * n_out off the float4 grid (one wire each)
    assert invalid(b.run(b.args(), row0=2, T=8), "row0")          # row0 * n_in and * n_out
    two_in, two_out = prog_of("rules"), prog_of("cross_wire")     # 2 in / 1 out and 1 in / 2 out: each of the four rules on its own
    bi, bo = FakeCall(two_in, 100, 8, window=(48, 0)), FakeCall(two_out, 100, 8, window=(48, 0))
    assert invalid(bi.run(bi.args(), rows=46), "rows_total * n_in") and invalid(bo.run(bo.args(), rows=46), "rows_total * n_in")
    assert invalid(bi.run(bi.args(), row0=2), "row0 * n_in") and invalid(bo.run(bo.args(), row0=2), "row0 * n_in")
    assert invalid(b.run(b.args(), row0=12), "beyond rows_total")  # 12 + 37 > 48
    assert invalid(b.run(b.args(), row0=48, T=1), "beyond rows_total")
    assert invalid(b.run(b.args(in_=b.addr["in_"] + 4)), "aligned")
    assert invalid(b.run(b.args(workspace_bytes=b.ws - 4)), "workspace")
    assert invalid(b.run(b.args(workspace=None)), "workspace")
    assert invalid(b.run(b.args(out_grad=None)), "out_grad")
    for size in (ctypes.sizeof(C.GradArgs) - 8, ctypes.sizeof(C.GradArgs) + 8, 0):
        assert invalid(b.run(b.args(struct_size=size)), "struct_size")
    assert invalid(b.run(b.args(checkpoint_rows=3)), "checkpoint_rows")
    assert C.lib.fz_run_block_grad_stream_major(p._h, None, 10, 12, 0, 10, None) == C.FZ_E_INVALID
    # overlaps are computed on the stream-major extents, n_streams * rows_total * wires: an in_grad that starts behind the WINDOW's
    # share of `in` (ns * T floats) but inside the buffer's (ns * rows floats) overlaps it
    inside = b.addr["in_"] + (b.ns * b.T * 4 + 15) // 16 * 16
    assert inside < b.addr["in_"] + b.size["in_"]
    assert invalid(b.run(b.args(in_grad=inside)), "overlap")
    assert invalid(b.run(b.args(state0_grad=b.addr["out_grad"] + b.size["out_grad"] - 16)), "overlap")
    # the same buffers pass every check: without a device the call stops at FZ_E_NO_DEVICE (with one, fake addresses are not launched on)
    if C.lib.fz_device_count() == 0:
        assert b.run(b.args()) == C.FZ_E_NO_DEVICE, C.last_error()
        assert b.run(b.args(), row0=8, T=40) == C.FZ_E_NO_DEVICE, C.last_error()


def test_an_empty_block_is_ok_and_needs_no_buffer():
    p, q = prog_of("df1_cascade_params6"), prog_of("moog_ladder")
    empty = empty_args()
    for ns, rows, T in ((0, 100, 100), (100, 100, 0), (0, 0, 0)):
        assert C.lib.fz_run_block_grad_stream_major(p._h, ctypes.byref(empty), ns, rows, 0, T, None) == C.FZ_OK, C.last_error()
        assert C.lib.fz_run_block_grad_stream_major(q._h, ctypes.byref(empty), ns, rows, 0, T, None) == C.FZ_OK, C.last_error()
    empty.struct_size = 8
    assert C.lib.fz_run_block_grad_stream_major(p._h, ctypes.byref(empty), 0, 0, 0, 0, None) == C.FZ_E_INVALID


def test_a_patch_that_cannot_fit_the_lds_is_refused_with_a_reason():
    p = prog_of("par4_sum")                                       # 5 wires: 32 checkpoint rows would need 168 KB of patches
    with pytest.raises(F.FlowzError) as ei:
        p.grad_resources(32, stream_major=True)
    assert ei.value.code == C.FZ_E_UNSUPPORTED and "checkpoint_rows" in str(ei.value)
    assert p.grad_resources(16, stream_major=True)["scratch_bytes"] == 0
