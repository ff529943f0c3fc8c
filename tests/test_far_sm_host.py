"""The far backward on stream-major buffers without a GPU (fz_run_block_far_grad_stream_major,
fz_run_block_far_loss_grad_stream_major): its scope and the refusals that stay, the calls it IS for a graph without a far line, the
rule that chooses the workgroup and the patch length together over the LDS ring slots alone (restated in tests/far_sm_graphs.py), the
argument checks, the workspace (the time-major query's), the kernels' resources and instructions (JIT for gfx950), the static rule
that picks the path, the kernel manifest of the GPU tests, and the restatement on transposed arrays."""
import ctypes
import os
import re

import numpy as np
import pytest

import far_grad_ref as FR
import far_sm_graphs as FS
import grad_graphs as GG
import ring_grad_graphs as RG
from grad_host_harness import (ADJOINT, ADJOINT_LOSS, ADJOINT_RING, ADJOINT_SM, LDS_BYTES, STATES, FakeCall, assert_no_contraction, empty_args, invalid,
                               kernel_ops, recorded_recipe, replay, write_manifest)
from zignal_amd import _capi as C
from zignal_amd import flowz as F

F32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
ADJOINT_FAR = 1                                                    # fz_internal.hpp: FZ_VF_ADJOINT_FAR
FAR_SM = ADJOINT | ADJOINT_RING | ADJOINT_FAR | ADJOINT_SM
FAR_LOSS_SM = FAR_SM | ADJOINT_LOSS
NEW_EXPORTS = ("fz_run_block_far_grad_stream_major", "fz_run_block_far_loss_grad_stream_major", "fz_program_far_grad_resources_for",
               "fz_program_far_grad_kernel_symbol_for", "fz_program_far_grad_source_for", "fz_program_far_loss_grad_resources_for",
               "fz_program_far_loss_grad_kernel_symbol_for", "fz_program_far_loss_grad_source_for")
STRIDES = (0, 1, 4)                                                # checkpoint_rows the geometry is checked at


def run_sm(p, a, loss, ns, rows, row0, T):
    fn = C.lib.fz_run_block_far_loss_grad_stream_major if loss else C.lib.fz_run_block_far_grad_stream_major
    return fn(p._h, ctypes.byref(a) if a is not None else None, ns, rows, row0, T, None)


def test_the_new_entry_points_are_declared_and_exported():
    header = open(os.path.join(HERE, "..", "include", "flowz_hip.h")).read()
    for name in NEW_EXPORTS:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in C.EXPORTS and getattr(C.lib, name)
    p = FS.prog("far_comb")
    with pytest.raises(F.FlowzError) as ei:                       # the layout is FZ_GRAD_TIME_MAJOR or FZ_GRAD_STREAM_MAJOR
        C.check(C.lib.fz_program_far_grad_kernel_symbol_for(p._h, 0, 2, None, 0))
    assert ei.value.code == C.FZ_E_INVALID and "layout" in str(ei.value)
    # time-major through the _for calls: what the inspectors without a layout answer
    buf = ctypes.create_string_buffer(1 << 20)
    for c in (0, 1, 32):
        for stem, method in (("far_grad", p.far_grad_kernel_symbol), ("far_loss_grad", p.far_loss_grad_kernel_symbol)):
            n = getattr(C.lib, f"fz_program_{stem}_kernel_symbol")(p._h, c, buf, len(buf))
            assert n > 0 and buf.value.decode() == method(c) == method(c, stream_major=False)
        n = C.lib.fz_program_far_grad_source(p._h, c, buf, len(buf))
        assert n > 0 and buf.value.decode() == p.far_grad_source(c)
    res = C.KernelResources()
    assert C.lib.fz_program_far_grad_resources(p._h, 0, ctypes.byref(res)) == C.FZ_OK
    assert res.lds_bytes == p.far_grad_resources()["lds_bytes"] == 0 and res.vgprs == p.far_grad_resources()["vgprs"]
    for method in ("run_block_far_grad_stream_major", "run_block_far_loss_grad_stream_major"):
        assert hasattr(F.Program, method)


# ---- scope -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(FS.FARS))
def test_the_graphs_are_taken(name):
    p = FS.prog(name)
    assert C.lib.fz_program_far_grad_check(p._h) == C.FZ_OK, C.last_error()
    tag = p.far_grad_kernel_symbol().split("_g")[1]
    for loss in (False, True):
        sym = (p.far_loss_grad_kernel_symbol if loss else p.far_grad_kernel_symbol)(0, stream_major=True)
        assert re.fullmatch(r"fz_adjoint_far_%ssm_kernel_c(1|2|4|8|16)r(4|8|16|32|64)b(256|128|64)_g%s" % ("loss_" if loss else "", tag), sym), sym
        src = (p.far_loss_grad_source if loss else p.far_grad_source)(0, stream_major=True)
        assert "#define FZ_FAR 1 " in src and "#define FZ_LOSS %d " % loss in src and "#define FZ_R " in src and "#define FZ_FAR_SLOTS " in src
        assert "__syncthreads" not in src and "atomic" not in src.split("extern \"C\"")[1]
        assert ("static void out(" in src) == loss
        # the generated body is the time-major far kernel's: it is layout-free
        body = lambda s: s.split("// ==== fz_graph_body.h ====")[1].split("// ==== fz_block_kernel.hip.inc ====")[0]   # noqa: E731
        assert body(src) == body((p.far_loss_grad_source if loss else p.far_grad_source)(0))
        for ns, T in ((0, 100), (100, 0), (0, 0)):                # an empty block is FZ_OK with nothing touched
            assert run_sm(p, empty_args(loss), loss, ns, 100, 0, T) == C.FZ_OK, C.last_error()
    assert FS.symbol_geometry(p.far_grad_kernel_symbol(0, True)) == FS.symbol_geometry(p.far_loss_grad_kernel_symbol(0, True))
    plain = F.compile(F.from_sexpr(GG.SUPPORTED["df1_cascade6"]())).grad_source(0, stream_major=True).split("// ==== fz_graph_body.h ====")[0]
    assert "FZ_FAR" not in plain and "FZ_NFL" not in plain and "FZ_NFR" not in plain   # (the plain stream-major kernel names no far macro)


@pytest.mark.parametrize("name", sorted(n for n in GG.REFUSED if n not in ("lds_ring_comb", "far_comb")))
def test_refusals_keep_the_words_of_the_far_check(name):
    build, typed, word = GG.REFUSED[name]
    p = F.compile(F.from_sexpr(build()), typed=typed)
    assert C.lib.fz_program_far_grad_check(p._h) == C.FZ_E_UNSUPPORTED
    why = C.last_error()
    assert word.lower() in why.lower()
    for loss in (False, True):
        assert run_sm(p, empty_args(loss), loss, 64, 16, 0, 16) == C.FZ_E_UNSUPPORTED and C.last_error() == why
    for call in (p.far_grad_kernel_symbol, p.far_grad_source, p.far_grad_resources, p.far_loss_grad_kernel_symbol):
        with pytest.raises(F.FlowzError) as ei:
            call(0, stream_major=True)
        assert ei.value.code == C.FZ_E_UNSUPPORTED and str(ei.value).endswith(why)


def test_rings_that_fit_no_workgroup_keep_the_refusal_of_the_far_check():
    p = F.compile(F.from_sexpr(RG.six_lines_256()))
    assert C.lib.fz_program_far_grad_check(p._h) == C.FZ_E_UNSUPPORTED
    why = C.last_error()
    assert "393216 bytes" in why
    for loss in (False, True):
        for ns, T in ((64, 16), (0, 0)):
            assert run_sm(p, empty_args(loss), loss, ns, 16, 0, T) == C.FZ_E_UNSUPPORTED and C.last_error() == why


@pytest.mark.parametrize("name", sorted(RG.RINGS))
def test_for_a_graph_without_a_far_line_the_calls_are_the_stream_major_ring_calls(name):
    p = F.compile(F.from_sexpr(RG.RINGS[name]()))
    for c in STRIDES:
        assert p.far_grad_kernel_symbol(c, stream_major=True) == p.ring_grad_kernel_symbol(c, stream_major=True)
        assert p.far_grad_source(c, stream_major=True) == p.ring_grad_source(c, stream_major=True)
        assert p.far_loss_grad_kernel_symbol(c, stream_major=True) == p.ring_loss_grad_kernel_symbol(c, stream_major=True)
        assert p.far_loss_grad_source(c, stream_major=True) == p.ring_loss_grad_source(c, stream_major=True)
    assert "fz_adjoint_ring_sm_kernel" in p.far_grad_kernel_symbol(0, stream_major=True)
    assert p.far_grad_workspace_bytes(1000, 40) == p.ring_grad_workspace_bytes(1000, 40)


@pytest.mark.parametrize("name", sorted(GG.SUPPORTED))
def test_for_a_graph_without_a_ring_line_the_calls_are_the_plain_stream_major_calls(name):
    p = F.compile(F.from_sexpr(GG.SUPPORTED[name]()))
    for c in STRIDES:
        assert p.far_grad_kernel_symbol(c, stream_major=True) == p.grad_kernel_symbol(c, stream_major=True)
        assert p.far_grad_source(c, stream_major=True) == p.grad_source(c, stream_major=True)
        if p.n_out:
            assert p.far_loss_grad_kernel_symbol(c, stream_major=True) == p.loss_grad_kernel_symbol(c, stream_major=True)
            assert p.far_loss_grad_source(c, stream_major=True) == p.loss_grad_source(c, stream_major=True)
    assert "fz_adjoint_sm_kernel" in p.far_grad_kernel_symbol(0, stream_major=True)
    assert p.far_grad_workspace_bytes(1000, 40) == p.grad_workspace_bytes(1000, 40)


def test_every_other_stream_major_call_still_refuses_the_far_comb():
    """the one-launch stream-major ring call, the stream-major recording calls and the forward stream-major call, each in the words it
    had; and there is still no stream-major far recording call"""
    p = FS.prog("far_comb")
    g, l = empty_args(False), empty_args(True)
    hbm = "delay lines deeper than 256 samples (rings in HBM) are not supported by the backward"
    calls = (lambda: C.lib.fz_run_block_ring_grad_stream_major(p._h, ctypes.byref(g), 64, 16, 0, 16, None),
             lambda: C.lib.fz_run_block_ring_loss_grad_stream_major(p._h, ctypes.byref(l), 64, 16, 0, 16, None),
             lambda: C.lib.fz_run_block_grad_stream_major(p._h, ctypes.byref(g), 64, 16, 0, 16, None),
             lambda: C.lib.fz_run_block_loss_grad_stream_major(p._h, ctypes.byref(l), 64, 16, 0, 16, None),
             lambda: C.lib.fz_run_recording_ring_grad_stream_major(p._h, ctypes.byref(g), 64, 16, 0, 16, 0, None, None),
             lambda: C.lib.fz_run_recording_ring_loss_grad_stream_major(p._h, ctypes.byref(l), 64, 16, 0, 16, 0, None, None),
             lambda: C.lib.fz_run_recording_grad(p._h, ctypes.byref(g), 1, 64, 16, 0, 16, 0, None, None),
             lambda: C.lib.fz_run_recording_loss_grad(p._h, ctypes.byref(l), 1, 64, 16, 0, 16, 0, None, None))
    for i, call in enumerate(calls):
        assert call() == C.FZ_E_UNSUPPORTED and C.last_error().endswith(hbm), (i, C.last_error())
    for call in (p.ring_grad_kernel_symbol, p.ring_loss_grad_source, p.ring_states_kernel_symbol):
        with pytest.raises(F.FlowzError) as ei:
            call(stream_major=True)
        assert ei.value.code == C.FZ_E_UNSUPPORTED and str(ei.value).endswith(hbm)
    # the forward: no stream-major body for rings in HBM
    with pytest.raises(F.FlowzError) as ei:
        p.kernel_name(F.make_variant(0, 0, 0, C.FZ_VF_STREAM_MAJOR), 4096, 64)
    assert ei.value.code == C.FZ_E_UNSUPPORTED and "stream-major frames: delay lines beyond 256 samples are not supported" in str(ei.value)
    with pytest.raises(F.FlowzError) as ei:
        p.build(F.make_variant(0, 0, 0, C.FZ_VF_STREAM_MAJOR), 64, 16)
    assert ei.value.code == C.FZ_E_UNSUPPORTED and "stream-major frames: delay lines beyond 256 samples are not supported" in str(ei.value)
    assert not hasattr(C.lib, "fz_run_recording_far_grad_stream_major") and not hasattr(F.Program, "run_recording_far_grad_stream_major")
    assert not hasattr(C.lib, "fz_run_recording_far_loss_grad_stream_major")


def test_a_forward_variant_naming_the_bits_is_refused_as_reserved():
    p = FS.prog("far_comb")
    for flags in (FAR_SM, FAR_LOSS_SM):
        with pytest.raises(F.FlowzError) as ei:
            p.kernel_name(F.make_variant(1, 16, 256, flags), 4096, 64)
        assert ei.value.code == C.FZ_E_INVALID and "reserved" in str(ei.value)


# ---- the geometry rule ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(FS.FARS))
def test_the_geometry_is_the_restated_rule(name):
    p = FS.prog(name)
    for c in STRIDES:
        C_, R, block = FS.geometry(p, c)
        assert block and R >= max(4, C_) and R % 4 == 0 and R % C_ == 0 and R & (R - 1) == 0
        assert C_ == FS.stride(p, c)                              # C is the time-major far kernel's
        for loss in (False, True):
            sym = (p.far_loss_grad_kernel_symbol if loss else p.far_grad_kernel_symbol)(c, stream_major=True)
            assert FS.symbol_geometry(sym) == (C_, R, block), (c, sym)
        for res in (p.far_grad_resources(c, stream_major=True), p.far_loss_grad_resources(c, stream_major=True)):
            assert res["lds_bytes"] == FS.lds_bytes(p, block, R) <= LDS_BYTES and res["unroll"] == C_, (c, res)
    assert FS.lds_ring_slots(p) == (17 if name == "far_mixed" else 0)


def test_the_table_of_the_geometry_rule():
    """| graph | LDS ring slots | C | R | block | LDS bytes |, derived by hand from the rule.  One input and one output wire: the ring
    kernels' longest patch is 32 rows, so R0 = max(16, C).
    far_comb   0 slots: R = 16: 4 * 256 * (0 + 16 * 2 + 4) = 36 864, twice that fits 163 840: 256 lanes; C = 32: R = 32, 69 632, twice
               that is 139 264: 256 lanes;
    far_mixed 17 slots: R = 16: 4 * 256 * (17 + 32 + 4) = 54 272, twice that fits: 256 lanes; C = 32: R = 32, 4 * 256 * (17 + 64 + 4) =
               87 040, twice that is 174 080 > 163 840; 128 lanes: 43 520, twice fits"""
    table = {"far_comb": {0: (16, 16, 256, 36864), 1: (1, 16, 256, 36864), 4: (4, 16, 256, 36864), 32: (32, 32, 256, 69632)},
             "far_mixed": {0: (4, 16, 256, 54272), 1: (1, 16, 256, 54272), 4: (4, 16, 256, 54272), 32: (32, 32, 128, 43520)}}
    for name, rows in table.items():
        p = FS.prog(name)
        assert (p.n_in, p.n_out) == (1, 1)
        for c, (C_, R, block, lds) in rows.items():
            assert FS.geometry(p, c) == (C_, R, block)
            assert FS.symbol_geometry(p.far_grad_kernel_symbol(c, stream_major=True)) == (C_, R, block)
            assert FS.symbol_geometry(p.far_loss_grad_kernel_symbol(c, stream_major=True)) == (C_, R, block)
            assert FS.lds_bytes(p, block, R) == lds
    assert FS.prog("far_comb").far_grad_resources(0, stream_major=True)["lds_bytes"] == 36864
    assert FS.prog("far_mixed").far_loss_grad_resources(0, stream_major=True)["lds_bytes"] == 54272
    assert 2 * FS.lds_bytes(FS.prog("far_mixed"), 256, 32) == 174080 > LDS_BYTES
    # half the stream-major ring kernel's patch at the same C: lds_ring_comb, one wire each way, takes R = 32 there
    import ring_sm_graphs as RS
    assert RS.geometry(RS.prog("lds_ring_comb"))[1] == 32 == 2 * FS.geometry(FS.prog("far_comb"))[1]


def far_ring_612():
    """ring_sm_graphs.three_wires_612 with a far line on a fourth wire: 612 samples of LDS rings.  Default C = 4 (10 saved floats per
    row: 4 frames, 3 ring reads, 1 far read and its 2 slots of the adjoint ring): the shortest patch, R = 4 rows of 5 wires + 4 floats,
    makes 4 * 64 * (612 + 20 + 4) = 162 816 bytes: taken.  checkpoint_rows = 8: R = 8, 4 * 64 * (612 + 40 + 4) = 167 936 bytes: refused."""
    from graphs import DEL, add
    return add(add(add(DEL(1, 256), DEL(2, 256)), DEL(3, 100)), DEL(4, 300))


def test_lds_rings_plus_the_shortest_patch_that_fit_no_workgroup_are_refused_with_the_bytes():
    p = F.compile(F.from_sexpr(far_ring_612()))
    assert (p.n_in, p.n_out, FS.lds_ring_slots(p)) == (4, 1, 612)
    assert C.lib.fz_program_far_grad_check(p._h) == C.FZ_OK, C.last_error()       # the time-major far backward takes it
    assert re.match(r"fz_adjoint_far_kernel_c4b64_g", p.far_grad_kernel_symbol())
    assert FS.geometry(p, 8) == (8, 8, 0) and FS.lds_bytes(p, 64, 8) == 167936 > LDS_BYTES
    for loss in (False, True):
        a = empty_args(loss)
        a.checkpoint_rows = 8
        for ns, T in ((64, 16), (0, 0)):
            assert run_sm(p, a, loss, ns, 16, 0, T) == C.FZ_E_UNSUPPORTED
            why = C.last_error()
            assert "167936 bytes" in why and str(LDS_BYTES) in why and "LDS" in why and "checkpoint_rows" in why and "(612 samples)" in why, why
    for call in (p.far_grad_kernel_symbol, p.far_loss_grad_source):
        with pytest.raises(F.FlowzError) as ei:
            call(8, stream_major=True)
        assert ei.value.code == C.FZ_E_UNSUPPORTED and "167936" in str(ei.value)
    assert re.match(r"fz_adjoint_far_kernel_c8b64_g", p.far_grad_kernel_symbol(8))          # (the time-major far kernel takes C = 8)
    # the default stride's patch is shorter: 162 816 bytes, taken
    assert FS.geometry(p) == (4, 4, 64) and FS.lds_bytes(p, 64, 4) == 162816
    assert FS.symbol_geometry(p.far_grad_kernel_symbol(0, stream_major=True)) == (4, 4, 64)
    r = p.far_grad_resources(0, stream_major=True)
    assert r["lds_bytes"] == 162816 and r["scratch_bytes"] == 0


# ---- argument checks: those of fz_run_block_ring_grad_stream_major, before a device is needed -----------------------------------------
@pytest.mark.parametrize("loss", [False, True])
@pytest.mark.parametrize("name", ["far_comb", "far_two_in"])
def test_argument_checks_fail_one_by_one_with_their_reason(name, loss):
    p = FS.prog(name)
    with FS.far_entry_points():
        b = FakeCall(FS.AsRingFamily(p), 1000, 40, ring=True, loss=loss, window=(48, 0))
    assert b.fn is (C.lib.fz_run_block_far_loss_grad_stream_major if loss else C.lib.fz_run_block_far_grad_stream_major)
    second = "target" if loss else "out_grad"
    for c in (0, 1, 32):                                          # the workspace is the time-major query's: it answers both layouts
        with FS.far_entry_points():
            assert FakeCall(FS.AsRingFamily(p), 1000, 40, ring=True, loss=loss, window=(48, 0), c=c).ws == p.far_grad_workspace_bytes(1000, 40, c) > 0
    assert b.ws == p.far_grad_workspace_bytes(1000, 40)
    size = ctypes.sizeof(C.LossGradArgs if loss else C.GradArgs)
    for bad in (size - 8, size + 8, 0, ctypes.sizeof(C.GradArgs if loss else C.LossGradArgs)):
        assert invalid(b.run(b.args(struct_size=bad)), "struct_size")
    assert invalid(b.run(b.args(checkpoint_rows=3)), "checkpoint_rows") and invalid(b.run(b.args(checkpoint_rows=64)), "checkpoint_rows")
    # windows and alignment: fz_run_block_grad_stream_major's
    assert invalid(b.run(b.args(), row0=12), "beyond rows_total") and invalid(b.run(b.args(), rows=39), "beyond rows_total")
    odd = next(r for r in (41, 42, 43) if (r * p.n_in) % 4 or (r * p.n_out) % 4)
    assert invalid(b.run(b.args(), rows=odd), "rows_total * n_in and rows_total * n_out")
    odd0 = next(r for r in (1, 2, 3) if (r * p.n_in) % 4 or (r * p.n_out) % 4)
    assert invalid(b.run(b.args(), row0=odd0, T=8), "row0 * n_in and row0 * n_out")
    assert invalid(b.run(b.args(**{second: None})), "target" if loss else "out_grad")
    assert invalid(b.run(b.args(in_=None)), "in is null") and invalid(b.run(b.args(state=None)), "state")
    assert invalid(b.run(b.args(workspace=None)), "fz_program_far_grad_workspace")
    assert invalid(b.run(b.args(workspace_bytes=b.ws - 4)), "fz_program_far_grad_workspace")
    for k in ("in_", second, "in_grad", "workspace", "state0_grad") + (("loss", "out") if loss else ()):
        assert invalid(b.run(b.args(**{k: b.addr[k] + 4})), "aligned"), k
    pairs = [("in_grad", "in_"), ("in_grad", second), ("state0_grad", "state"), ("workspace", "in_grad"), ("workspace", second)]
    if loss:
        pairs += [("loss", "target"), ("loss", "workspace"), ("out", "target"), ("out", "in_grad"), ("out", "loss"), ("workspace", "out")]
    for k, other in pairs:
        assert invalid(b.run(b.args(**{k: b.addr[other]})), "overlap"), (k, other)
    assert invalid(b.run(b.args(state0_grad=b.addr["state_grad"] + 16)), "overlap")      # (only the exact alias of state_grad is allowed)
    # a stream-major buffer is touched over its whole extent: an output that starts inside the last rows of another overlaps it
    assert invalid(b.run(b.args(in_grad=b.addr["in_"] + b.size["in_"] - 16)), "overlap")
    assert run_sm(p, None, loss, 10, 12, 0, 10) == C.FZ_E_INVALID and "null arguments" in C.last_error()
    assert b.run(b.args(), ns=1 << 30) == C.FZ_E_UNSUPPORTED and "2^30" in C.last_error()
    empty = empty_args(loss)
    for ns, T in ((0, 40), (1000, 0), (0, 0)):
        assert b.run(empty, ns=ns, T=T) == C.FZ_OK, C.last_error()
    empty.struct_size = 8
    assert b.run(empty, ns=0, T=0) == C.FZ_E_INVALID
    # what passes every check stops at the missing device (with one, fake addresses are not launched on)
    if C.lib.fz_device_count() == 0:
        assert b.run(b.args()) == C.FZ_E_NO_DEVICE, C.last_error()
        assert b.run(b.args(), row0=8, T=40) == C.FZ_E_NO_DEVICE, C.last_error()
        assert b.run(b.args(state0_grad=b.addr["state_grad"])) == C.FZ_E_NO_DEVICE, C.last_error()
        none = dict(in_grad=None, state0_grad=None, param_grad=None, const_grad=None, state_grad=None)
        if loss:
            none.update(loss=None, out=None)
        assert b.run(b.args(**none)) == C.FZ_E_NO_DEVICE


# ---- the kernels for gfx950 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(FS.FARS))
def test_the_kernels_jit_compile_without_scratch_within_the_lds(name, capsys):
    p = FS.prog(name)
    lines = []
    for c in (0, 1):
        C_, R, block = FS.geometry(p, c)
        for loss in (False, True):
            r = (p.far_loss_grad_resources if loss else p.far_grad_resources)(c, stream_major=True)
            sym = (p.far_loss_grad_kernel_symbol if loss else p.far_grad_kernel_symbol)(c, stream_major=True)
            assert r["scratch_bytes"] == 0, (sym, r)
            assert r["lds_bytes"] == FS.lds_bytes(p, block, R) and r["vgprs"] + r["agprs"] <= 256, (sym, r)
            lines.append(f"{sym}: {r['vgprs']} VGPRs, {r['sgprs']} SGPRs, {r['vgpr_spills']} VGPR spills, {r['sgpr_spills']} SGPR spills, {r['lds_bytes']} B LDS")
    with capsys.disabled():                                       # (spills are reported, not asserted: DESIGN.md 9.13 records them)
        print("\n" + "\n".join(lines))


@pytest.mark.parametrize("c", [0, 1])
@pytest.mark.parametrize("loss", [False, True])
@pytest.mark.parametrize("name", sorted(FS.FARS))
def test_the_kernels_have_no_fma_no_barrier_and_no_atomic(name, loss, c, tmp_path, monkeypatch):
    """the no-contraction rule of grad_host_harness on every new kernel, at the default C and at C = 1; every one of them moves its
    frames through LDS, without a barrier and without an atomic"""
    _, r, _, every = kernel_ops(monkeypatch, tmp_path, FS.FARS[name](), "far_loss_grad_resources" if loss else "far_grad_resources", c, stream_major=True)
    assert_no_contraction(every, divides=name == "far_adjacent", lds=True)
    assert r["scratch_bytes"] == 0


# ---- the static rule that picks the path ---------------------------------------------------------------------------------------------
def fast(p, c=0):
    m = re.search(r"#define FZ_FAR_FAST ([01]) ", p.far_grad_source(c, stream_major=True))
    assert m
    assert "#define FZ_FAR_FAST %s " % m.group(1) in p.far_loss_grad_source(c, stream_major=True)
    assert "#define FZ_FAR_FAST %s " % m.group(1) in p.far_grad_source(c)      # the time-major kernel's choice: one rule
    return m.group(1) == "1"


def test_path_choice():
    assert {n: fast(FS.prog(n)) for n in FS.FARS} == FS.FAST
    assert all(fast(FS.prog(n), 1) for n in FS.FARS)
    assert not fast(FS.prog("far_tap1"), 32) and fast(FS.prog("far_comb"), 32)
    # the generated body follows it, and sweep 1's chunked reads are the time-major kernel's
    assert "const float* f2, float* fq)" in FS.prog("far_comb").far_grad_source(0, stream_major=True)
    assert "float* fa, const unsigned* fpt, size_t ns)" in FS.prog("far_tap1").far_grad_source(0, stream_major=True)
    assert "fz_fr_chunked[3] = {1u, 0u, 1u}" in FS.prog("far_tap1").far_grad_source(0, stream_major=True)


# ---- the kernel manifest of the GPU tests ------------------------------------------------------------------------------------------
def test_the_committed_manifest_holds_exactly_the_kernels_the_gpu_tests_launch():
    recs = FS.manifest_variants(FS.MANIFEST)
    for bits, loss in ((FAR_SM, False), (FAR_LOSS_SM, True)):
        got = sorted(v[:4] for v in recs if v[3] == bits)
        want = []
        for p, c, ls in FS.kernel_requests():
            if ls == loss:
                C_, R, block = FS.geometry(p, c)
                want.append((R, C_, block, bits))
        assert got == sorted(want) and len(got) == len({v for v in recs if v[3] == bits}), (loss, got, want)
    assert len(FS.kernel_requests()) == 22
    # nothing else but the time-major far kernels compared with and the time-major forward kernels
    others = [v for v in recs if v[3] not in (FAR_SM, FAR_LOSS_SM)]
    far_tm = ADJOINT | ADJOINT_RING | ADJOINT_FAR
    assert all(v[3] in (far_tm, far_tm | ADJOINT_LOSS) and v[0] == 1 for v in others if v[3] & ADJOINT)
    assert all(not (v[3] & (ADJOINT_LOSS | ADJOINT_RING | STATES | C.FZ_VF_STREAM_MAJOR)) for v in others if not v[3] & ADJOINT) and len(set(recs)) <= 64
    counts = replay(FS.MANIFEST)
    assert counts["failed"] == 0 and counts["records"] == len(set(recs)), counts


def test_a_manifest_cannot_ask_for_a_kernel_the_backward_would_not_make(tmp_path):
    """a wrong block, a wrong R (1, a non-power of two, below C, R / 2, 2 R), a C that is no power of two <= 32, the far bit without
    the ring bit, STATES next to the bits, a graph without a far line: counted as failed, nothing built"""
    p = FS.prog("far_comb")
    C_, R, block = FS.geometry(p)
    assert (C_, R, block) == (16, 16, 256)
    far_recipe = next(v[4] for v in FS.manifest_variants(FS.MANIFEST) if v[:4] == (R, C_, block, FAR_SM))
    ring_recipe = recorded_recipe(tmp_path, "ring_grad_graphs", "RINGS['fb9']()", "ring_grad_resources")
    bad = []
    for bits in (FAR_SM, FAR_LOSS_SM):
        bad += [(R, C_, 128, bits, far_recipe), (R, C_, 512, bits, far_recipe), (1, C_, block, bits, far_recipe), (24, C_, block, bits, far_recipe),
                (4, C_, block, bits, far_recipe), (R // 2, C_, block, bits, far_recipe), (2 * R, C_, block, bits, far_recipe), (R, 3, block, bits, far_recipe),
                (R, 64, block, bits, far_recipe), (R, 0, block, bits, far_recipe), (R, C_, block, bits & ~ADJOINT_RING, far_recipe),
                (R, C_, block, bits | STATES, far_recipe), (R, C_, block, bits, ring_recipe)]
    bad.append((R, 8, block, ADJOINT | STATES | ADJOINT_RING | ADJOINT_FAR | ADJOINT_SM, far_recipe))   # (stream-major far recordings are not built)
    write_manifest(tmp_path / "bad.fzm", bad)
    counts = replay(tmp_path / "bad.fzm", {"FLOWZ_HIP_CACHE": str(tmp_path / "cache")})
    assert counts["failed"] == len(bad) and counts["built"] == 0 and counts["at_hand"] == 0, counts
    # and the same record with the right numbers is built
    write_manifest(tmp_path / "good.fzm", [(R, C_, block, FAR_SM, far_recipe), (R, 4, block, FAR_LOSS_SM, far_recipe)])
    counts = replay(tmp_path / "good.fzm", {"FLOWZ_HIP_CACHE": str(tmp_path / "cache")})
    assert counts["failed"] == 0 and counts["built"] == 2, counts


# ---- the restatement on transposed arrays ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["far_comb", "far_two_in", "far_mixed"])
def test_the_restatement_on_transposed_arrays_is_its_own_answer(name):
    """stream-major buffers are the time-major frames transposed: far_grad_ref.grad of the window, transposed back, is far_grad_ref.grad
    -- the layout map the GPU file relies on; the state rows are [row][n_streams] in both layouts"""
    p = FS.prog(name)
    D = FS.DEEPEST[name]
    ns, T, row0 = 5, D + 3, 4
    x, s0, par, yb, sb, ap, ac = FS.FG.inputs(p, ns, T, 17, p0=D - 3)
    want = FR.grad(p, x, yb, s0, par, sb, ap, ac)
    xs, ys = FS.to_sm(x, None, row0, 7.0), FS.to_sm(yb, None, row0, 7.0)
    assert xs.shape == (ns, FS.up4(row0 + T), p.n_in)
    got = FR.grad(p, FS.from_sm(xs, T, row0), FS.from_sm(ys, T, row0), s0, par, sb, ap, ac)
    for k in want:
        assert np.array_equal(np.asarray(got[k]).view(np.uint32), np.asarray(want[k]).view(np.uint32)), k
    gx = FS.to_sm(got["x"], xs.shape[1], row0, fill=-1234.5)
    assert np.array_equal(FS.from_sm(gx, T, row0), want["x"]) and np.all(gx[:, :row0] == F32(-1234.5))
