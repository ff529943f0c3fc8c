"""The ring backward on stream-major buffers without a GPU (fz_run_block_ring_grad_stream_major,
fz_run_block_ring_loss_grad_stream_major): its scope and the refusals that stay, the calls it IS for a graph without a deep line, the
rule that chooses the workgroup and the patch length together (restated in tests/ring_sm_graphs.py), the refusal when rings plus the
shortest patch fit no workgroup, the argument checks of the stream-major siblings, the kernels' resources and instructions (JIT for
gfx950), the code pins' names for every other kernel, the kernel manifest of the GPU tests, and the restatement on transposed arrays."""
import ctypes
import os
import re

import numpy as np
import pytest

import adjoint_ref as A
import grad_graphs as GG
import ring_grad_graphs as RG
import ring_loss_graphs as RL
import ring_sm_graphs as RS
from grad_host_harness import (ADJOINT, ADJOINT_LOSS, ADJOINT_RING, ADJOINT_SM, LDS_BYTES, STATES, FakeCall, assert_no_contraction, code_pins, empty_args,
                               invalid, kernel_ops, recorded_recipe, replay, write_manifest)
from zignal_amd import _capi as C
from zignal_amd import flowz as F

F32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
RING_SM = ADJOINT | ADJOINT_RING | ADJOINT_SM
RING_LOSS_SM = RING_SM | ADJOINT_LOSS
NEW_EXPORTS = ("fz_run_block_ring_grad_stream_major", "fz_run_block_ring_loss_grad_stream_major", "fz_program_ring_grad_resources_for",
               "fz_program_ring_grad_kernel_symbol_for", "fz_program_ring_grad_source_for", "fz_program_ring_loss_grad_resources_for",
               "fz_program_ring_loss_grad_kernel_symbol_for", "fz_program_ring_loss_grad_source_for")


def run_sm(p, a, loss, ns, rows, row0, T):
    fn = C.lib.fz_run_block_ring_loss_grad_stream_major if loss else C.lib.fz_run_block_ring_grad_stream_major
    return fn(p._h, ctypes.byref(a) if a is not None else None, ns, rows, row0, T, None)


def test_the_new_entry_points_are_declared_and_exported():
    header = open(os.path.join(HERE, "..", "include", "flowz_hip.h")).read()
    for name in NEW_EXPORTS:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in C.EXPORTS and getattr(C.lib, name)
    p = RS.prog("fb9")
    with pytest.raises(F.FlowzError) as ei:                       # the layout is FZ_GRAD_TIME_MAJOR or FZ_GRAD_STREAM_MAJOR
        C.check(C.lib.fz_program_ring_grad_kernel_symbol_for(p._h, 0, 2, None, 0))
    assert ei.value.code == C.FZ_E_INVALID and "layout" in str(ei.value)
    for c in RS.STRIDES:                                          # time-major through the _for calls: the calls without a layout
        assert p.ring_grad_kernel_symbol(c, stream_major=False) == p.ring_grad_kernel_symbol(c)


# ---- scope -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(RS.GRAPHS))
def test_the_graphs_are_taken(name):
    p = RS.prog(name)
    tag = p.ring_grad_kernel_symbol().split("_g")[1]
    for loss in ((False, True) if name in RS.RINGS else (True,)):
        symbol = p.ring_loss_grad_kernel_symbol if loss else p.ring_grad_kernel_symbol
        sym = symbol(0, stream_major=True)
        assert re.fullmatch(r"fz_adjoint_ring_%ssm_kernel_c(1|2|4|8|16)r(4|8|16|32|64)b(256|128|64)_g%s" % ("loss_" if loss else "", tag), sym), sym
        src = (p.ring_loss_grad_source if loss else p.ring_grad_source)(0, stream_major=True)
        assert "fz_adj_ring_sm_args" in src and "#define FZ_LOSS %d " % loss in src and "#define FZ_R " in src and "#define FZ_RING_SLOTS " in src
        assert "__syncthreads" not in src and "atomic" not in src.split("extern \"C\"")[1]
        assert ("static void out(" in src) == loss
        for ns, T in ((0, 100), (100, 0), (0, 0)):                # an empty block is FZ_OK with nothing touched
            assert run_sm(p, empty_args(loss), loss, ns, 100, 0, T) == C.FZ_OK, C.last_error()
    # the plain and the loss kernel share C, R and the lanes
    assert RS.symbol_geometry(p.ring_grad_kernel_symbol(0, True)) == RS.symbol_geometry(p.ring_loss_grad_kernel_symbol(0, True))
    assert p.ring_grad_workspace_bytes(1000, 40) > 0


def test_rings_that_fit_no_workgroup_keep_the_refusal_of_the_ring_check():
    p = F.compile(F.from_sexpr(RG.six_lines_256()))
    assert C.lib.fz_program_ring_grad_check(p._h) == C.FZ_E_UNSUPPORTED
    why = C.last_error()
    for loss in (False, True):
        for ns, T in ((64, 16), (0, 0)):
            assert run_sm(p, empty_args(loss), loss, ns, 16, 0, T) == C.FZ_E_UNSUPPORTED and C.last_error() == why and "393216 bytes" in why
    for call in (p.ring_grad_kernel_symbol, p.ring_grad_source, p.ring_grad_resources, p.ring_loss_grad_kernel_symbol, p.ring_loss_grad_source,
                 p.ring_loss_grad_resources):
        with pytest.raises(F.FlowzError) as ei:
            call(0, stream_major=True)
        assert ei.value.code == C.FZ_E_UNSUPPORTED and "393216" in str(ei.value)


@pytest.mark.parametrize("name", sorted(n for n in GG.REFUSED if n != "lds_ring_comb"))
def test_refusals_keep_their_reasons(name):
    build, typed, word = GG.REFUSED[name]
    p = F.compile(F.from_sexpr(build()), typed=typed)
    assert C.lib.fz_program_grad_check(p._h) == C.FZ_E_UNSUPPORTED
    why = C.last_error()
    assert word.lower() in why.lower()
    for loss in (False, True):
        assert run_sm(p, empty_args(loss), loss, 64, 16, 0, 16) == C.FZ_E_UNSUPPORTED and C.last_error() == why


@pytest.mark.parametrize("name", sorted(GG.SUPPORTED))
def test_for_a_graph_without_a_ring_the_calls_are_the_stream_major_calls(name):
    p = F.compile(F.from_sexpr(GG.SUPPORTED[name]()))
    for c in RS.STRIDES:
        assert p.ring_grad_kernel_symbol(c, stream_major=True) == p.grad_kernel_symbol(c, stream_major=True)
        assert p.ring_grad_source(c, stream_major=True) == p.grad_source(c, stream_major=True)
        assert p.ring_loss_grad_kernel_symbol(c, stream_major=True) == p.loss_grad_kernel_symbol(c, stream_major=True)
        assert p.ring_loss_grad_source(c, stream_major=True) == p.loss_grad_source(c, stream_major=True)
    assert p.ring_grad_workspace_bytes(1000, 40) == p.grad_workspace_bytes(1000, 40)
    if name in ("integrator", "moog_ladder"):
        assert p.ring_grad_resources(0, stream_major=True) == p.grad_resources(0, stream_major=True)
        assert p.ring_loss_grad_resources(0, stream_major=True) == p.loss_grad_resources(0, stream_major=True)


def test_every_existing_stream_major_and_recording_call_still_refuses_the_ring_comb():
    p = RS.prog("lds_ring_comb")
    g, l = empty_args(False), empty_args(True)
    calls = (lambda: C.lib.fz_run_block_grad_stream_major(p._h, ctypes.byref(g), 64, 16, 0, 16, None),
             lambda: C.lib.fz_run_block_loss_grad_stream_major(p._h, ctypes.byref(l), 64, 16, 0, 16, None),
             lambda: C.lib.fz_run_block_grad(p._h, ctypes.byref(g), 64, 16, None),
             lambda: C.lib.fz_run_block_loss_grad(p._h, ctypes.byref(l), 64, 16, None),
             lambda: C.lib.fz_run_recording_grad(p._h, ctypes.byref(g), 0, 64, 0, 0, 16, 0, None, None),
             lambda: C.lib.fz_run_recording_grad(p._h, ctypes.byref(g), 1, 64, 16, 0, 16, 0, None, None),
             lambda: C.lib.fz_run_recording_loss_grad(p._h, ctypes.byref(l), 0, 64, 0, 0, 16, 0, None, None),
             lambda: C.lib.fz_run_recording_loss_grad(p._h, ctypes.byref(l), 1, 64, 16, 0, 16, 0, None, None))
    for i, call in enumerate(calls):
        assert call() == C.FZ_E_UNSUPPORTED and "LDS" in C.last_error(), (i, C.last_error())
    for sm in (False, True):
        for call in (p.grad_kernel_symbol, p.grad_resources, p.grad_source, p.loss_grad_kernel_symbol, p.loss_grad_resources, p.loss_grad_source):
            with pytest.raises(F.FlowzError) as ei:
                call(stream_major=sm)
            assert ei.value.code == C.FZ_E_UNSUPPORTED and "LDS" in str(ei.value)
        for call in (p.states_kernel_symbol, p.states_source):
            with pytest.raises(F.FlowzError) as ei:
                call(sm)
            assert ei.value.code == C.FZ_E_UNSUPPORTED and "LDS" in str(ei.value)
    from zignal_amd import autograd as AG
    for fn in (lambda: AG.run(p, None, stream_major=True), lambda: AG.mse(p, None, None, stream_major=True),
               lambda: AG.mse_recording(p, None, None, stream_major=True)):
        with pytest.raises(F.FlowzError) as ei:
            fn()
        assert ei.value.code == C.FZ_E_UNSUPPORTED and "LDS" in str(ei.value)


def test_a_forward_variant_naming_the_bits_is_refused_as_reserved():
    p = RS.prog("fb9")
    for flags in (ADJOINT_RING | ADJOINT_SM, RING_SM, RING_LOSS_SM):
        with pytest.raises(F.FlowzError) as ei:
            p.kernel_name(F.make_variant(1, 8, 256, flags), 4096, 64)
        assert ei.value.code == C.FZ_E_INVALID and "reserved" in str(ei.value)
        with pytest.raises(F.FlowzError):
            p.build(F.make_variant(1, 8, 256, flags))


# ---- the geometry rule ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(RS.GRAPHS))
def test_the_geometry_is_the_restated_rule(name):
    p = RS.prog(name)
    for c in RS.STRIDES:
        C_, R, block = RS.geometry(p, c)
        assert block and R >= max(4, C_) and R % 4 == 0 and R % C_ == 0 and R & (R - 1) == 0
        for loss in (False, True):
            sym = (p.ring_loss_grad_kernel_symbol if loss else p.ring_grad_kernel_symbol)(c, stream_major=True)
            assert RS.symbol_geometry(sym) == (C_, R, block), (c, sym)
        for res in (p.ring_grad_resources(c, stream_major=True), p.ring_loss_grad_resources(c, stream_major=True)):
            assert res["lds_bytes"] == RS.lds_bytes(p, block, R) <= LDS_BYTES and res["unroll"] == C_, (c, res)


def test_the_table_of_the_geometry_rule():
    """| graph | rings | C | block | R | LDS bytes |: lds_ring_comb 63 slots, 16, 128, 32, 67 072; the 256-slot graphs 16, 64, 16, 74 752
    (R = 32 would be 82 944 bytes per 64 lanes, and two of those do not fit 163 840)"""
    comb = RS.prog("lds_ring_comb")
    assert (RS.ring_slots(comb), comb.n_in, comb.n_out) == (63, 1, 1)
    assert RS.symbol_geometry(comb.ring_grad_kernel_symbol(0, stream_major=True)) == (16, 32, 128)
    assert comb.ring_grad_resources(0, stream_major=True)["lds_bytes"] == 67072
    deep = F.compile(F.from_sexpr(RG.fb(RG.add(RG.mul(RG.lit(0.5), RG.DEL(1, 256)), RG.IN(2)))))      # ~(0.5 _1[_256] + _2)
    for p in (deep, RS.prog("tap256")):
        assert RS.ring_slots(p) == 256
        assert RS.symbol_geometry(p.ring_grad_kernel_symbol(0, stream_major=True)) == (16, 16, 64)
        assert RS.symbol_geometry(p.ring_loss_grad_kernel_symbol(0, stream_major=True)) == (16, 16, 64)
        assert p.ring_grad_resources(0, stream_major=True)["lds_bytes"] == 74752
        assert RS.lds_bytes(p, 64, 32) == 82944 and 2 * 82944 > LDS_BYTES


def test_rings_plus_the_shortest_patch_that_fit_no_workgroup_are_refused_with_the_bytes():
    p = F.compile(F.from_sexpr(RS.three_wires_612()))
    assert (p.n_in, p.n_out, RS.ring_slots(p)) == (3, 1, 612)
    assert C.lib.fz_program_ring_grad_check(p._h) == C.FZ_OK, C.last_error()      # the time-major ring backward takes it
    assert re.match(r"fz_adjoint_ring_kernel_c8b64_g", p.ring_grad_kernel_symbol())
    assert RS.geometry(p) == (8, 8, 0) and RS.lds_bytes(p, 64, 8) == 165888 > LDS_BYTES
    for loss in (False, True):
        for ns, T in ((64, 16), (0, 0)):
            assert run_sm(p, empty_args(loss), loss, ns, 16, 0, T) == C.FZ_E_UNSUPPORTED
            why = C.last_error()
            assert "165888 bytes" in why and str(LDS_BYTES) in why and "LDS" in why and "checkpoint_rows" in why, why
    for call in (p.ring_grad_kernel_symbol, p.ring_loss_grad_source):
        with pytest.raises(F.FlowzError) as ei:
            call(0, stream_major=True)
        assert ei.value.code == C.FZ_E_UNSUPPORTED and "165888" in str(ei.value)
    # a smaller checkpoint_rows shortens the patch: 161 792 bytes, taken
    assert RS.geometry(p, 4) == (4, 4, 64) and RS.lds_bytes(p, 64, 4) == 161792
    assert RS.symbol_geometry(p.ring_grad_kernel_symbol(4, stream_major=True)) == (4, 4, 64)
    r = p.ring_grad_resources(4, stream_major=True)
    assert r["lds_bytes"] == 161792 and r["scratch_bytes"] == 0 and r["vgpr_spills"] == 0


# ---- argument checks: those of the stream-major siblings, before a device is needed ------------------------------------------------
@pytest.mark.parametrize("loss", [False, True])
@pytest.mark.parametrize("name", ["lds_ring_comb", "two_out_fb"])
def test_argument_checks_fail_one_by_one_with_their_reason(name, loss):
    p = RS.prog(name)
    b = FakeCall(p, 1000, 40, ring=True, loss=loss, window=(48, 0))
    second = "target" if loss else "out_grad"
    assert b.ws == p.ring_grad_workspace_bytes(1000, 40) > 0
    size = ctypes.sizeof(C.LossGradArgs if loss else C.GradArgs)
    for bad in (size - 8, size + 8, 0, ctypes.sizeof(C.GradArgs if loss else C.LossGradArgs)):
        assert invalid(b.run(b.args(struct_size=bad)), "struct_size")
    assert invalid(b.run(b.args(checkpoint_rows=3)), "checkpoint_rows") and invalid(b.run(b.args(checkpoint_rows=64)), "checkpoint_rows")
    # windows and alignment: fz_run_block_grad_stream_major's
    assert invalid(b.run(b.args(), row0=12), "beyond rows_total") and invalid(b.run(b.args(), rows=39), "beyond rows_total")
    if p.n_in % 4 or p.n_out % 4:
        odd = next(r for r in (41, 42, 43) if (r * p.n_in) % 4 or (r * p.n_out) % 4)
        assert invalid(b.run(b.args(), rows=odd), "rows_total * n_in and rows_total * n_out")
        odd0 = next(r for r in (1, 2, 3) if (r * p.n_in) % 4 or (r * p.n_out) % 4)
        assert invalid(b.run(b.args(), row0=odd0, T=8), "row0 * n_in and row0 * n_out")
    assert invalid(b.run(b.args(**{second: None})), "target" if loss else "out_grad")
    assert invalid(b.run(b.args(in_=None)), "in is null") and invalid(b.run(b.args(state=None)), "state")
    if p.n_param:
        assert invalid(b.run(b.args(params=None)), "params")
    assert invalid(b.run(b.args(workspace=None)), "fz_program_ring_grad_workspace")
    assert invalid(b.run(b.args(workspace_bytes=b.ws - 4)), "fz_program_ring_grad_workspace")
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
@pytest.mark.parametrize("name", sorted(RS.GRAPHS))
def test_the_kernels_jit_compile_without_scratch_within_the_lds(name, capsys):
    p = RS.prog(name)
    lines = []
    for c in (0, 1):
        for loss in (False, True):
            r = (p.ring_loss_grad_resources if loss else p.ring_grad_resources)(c, stream_major=True)
            sym = (p.ring_loss_grad_kernel_symbol if loss else p.ring_grad_kernel_symbol)(c, stream_major=True)
            assert r["scratch_bytes"] == 0 and r["vgpr_spills"] == 0, (sym, r)
            assert 0 < r["lds_bytes"] <= LDS_BYTES and r["vgprs"] + r["agprs"] <= 256, (sym, r)
            lines.append(f"{sym}: {r['vgprs']} VGPRs, {r['sgprs']} SGPRs, {r['sgpr_spills']} SGPR spills, {r['lds_bytes']} B LDS")
    with capsys.disabled():                                       # (SGPR spills are reported, not asserted: correct, slower)
        print("\n" + "\n".join(lines))


@pytest.mark.parametrize("c", [0, 1])
@pytest.mark.parametrize("name,loss", [(n, ls) for n in sorted(RS.GRAPHS) for ls in ((False, True) if n in RS.RINGS else (True,))])
def test_the_kernels_have_no_fma_no_barrier_and_no_atomic(name, loss, c, tmp_path, monkeypatch):
    """the method of test_ring_grad_host.py: test_ring_kernel_has_no_fma -- on every graph, at the default C and at C = 1 (the two graphs
    with two outputs have the loss kernel only, as everywhere in this file)"""
    _, _, _, every = kernel_ops(monkeypatch, tmp_path, RS.GRAPHS[name](), "ring_loss_grad_resources" if loss else "ring_grad_resources", c, stream_major=True)
    assert_no_contraction(every, divides=name == "ks_tanh11", lds=True)


# ---- every existing kernel's code is the parent's: tests/golden/adjoint_code_pins.json, held by test_adjoint_code_pins_host.py -------------
PINS = code_pins()


def test_the_pins_cover_every_graph():
    for kind in ("ring", "ring_loss"):
        for layout in ("tm", "sm"):
            for c in RS.STRIDES:
                assert sorted(k.split("/")[3] for k in PINS if k.startswith(f"{kind}/{layout}/c{c}/")) == sorted(RS.GRAPHS), (kind, layout, c)
    assert sorted(k.split("/")[2] for k in PINS if k.startswith("ring_states/tm/")) == sorted(RS.GRAPHS)
    for kind in ("adjoint", "loss", "states"):
        for layout in ("tm", "sm"):
            assert sorted(k.split("/")[2] for k in PINS if k.startswith(f"{kind}/{layout}/")) == sorted(GG.SUPPORTED), (kind, layout)


def test_every_other_kernel_has_the_parents_text():
    """the pins name the kernels the library makes in both layouts, and the stream-major ring kernels' instructions are none of the
    time-major ones' (that all of them are the parent's code: test_adjoint_code_pins_host.py)"""
    pinned = {v[".text"] for k, v in PINS.items() if k.startswith(("ring/tm/", "ring_loss/tm/"))}
    for name in sorted(RS.GRAPHS):
        p = RS.prog(name)
        for c in RS.STRIDES:
            for kind, symbol in (("ring", p.ring_grad_kernel_symbol), ("ring_loss", p.ring_loss_grad_kernel_symbol)):
                assert PINS[f"{kind}/tm/c{c}/{name}"]["symbol"] == symbol(c) and PINS[f"{kind}/sm/c{c}/{name}"]["symbol"] == symbol(c, stream_major=True)
                assert PINS[f"{kind}/sm/c{c}/{name}"][".text"] not in pinned


# ---- the kernel manifest of the GPU tests ------------------------------------------------------------------------------------------
def test_the_committed_manifest_holds_exactly_the_kernels_the_gpu_tests_launch():
    recs = RS.manifest_variants(RS.MANIFEST)
    for bits, loss in ((RING_SM, False), (RING_LOSS_SM, True)):
        got = sorted(v[:4] for v in recs if v[3] == bits)
        want = []
        for p, c, ls in RS.kernel_requests():
            if ls == loss:
                C_, R, block = RS.geometry(p, c)
                want.append((R, C_, block, bits))
        assert got == sorted(want) and len(got) == len({v for v in recs if v[3] == bits}), (loss, got, want)
    # nothing else but the time-major ring kernels compared with and the stream-major forward kernels of the chained windows and autograd
    others = [v for v in recs if v[3] not in (RING_SM, RING_LOSS_SM)]
    assert all(v[3] in (ADJOINT | ADJOINT_RING, ADJOINT | ADJOINT_RING | ADJOINT_LOSS) and v[0] == 1 for v in others if v[3] & ADJOINT)
    assert all(not (v[3] & (ADJOINT_LOSS | ADJOINT_RING | STATES)) for v in others if not v[3] & ADJOINT) and len(set(recs)) <= 64
    counts = replay(RS.MANIFEST)
    assert counts["failed"] == 0 and counts["records"] == len(set(recs)), counts


def test_a_manifest_cannot_ask_for_a_kernel_the_backward_would_not_make(tmp_path):
    """a wrong block, a wrong R (R / 2, 2 R, 1), a C that is no power of two <= 32, STATES next to the bits, a graph without a ring, a
    graph the call refuses: counted as failed, nothing built"""
    p = RS.prog("lds_ring_comb")
    C_, R, block = RS.geometry(p)
    ring_recipe = next(v[4] for v in RS.manifest_variants(RS.MANIFEST) if v[:4] == (R, C_, block, RING_SM))
    plain_recipe = recorded_recipe(tmp_path, "grad_graphs", "SUPPORTED['integrator']()", "grad_resources")
    refused_recipe = recorded_recipe(tmp_path, "ring_sm_graphs", "three_wires_612()", "ring_grad_resources")
    bad = []
    for bits in (RING_SM, RING_LOSS_SM):
        bad += [(R, C_, 256 if block != 256 else 128, bits, ring_recipe), (R, C_, 512, bits, ring_recipe), (R // 2, C_, block, bits, ring_recipe),
                (2 * R, C_, block, bits, ring_recipe), (1, C_, block, bits, ring_recipe), (R, 3, block, bits, ring_recipe), (R, 64, block, bits, ring_recipe),
                (R, 0, block, bits, ring_recipe), (R, C_, block, bits | STATES, ring_recipe), (R, C_, block, bits, plain_recipe),
                (8, 8, 64, bits, refused_recipe)]
    bad.append((R, 8, block, ADJOINT | STATES | ADJOINT_RING | ADJOINT_SM, ring_recipe))     # (stream-major ring recordings are not built)
    write_manifest(tmp_path / "bad.fzm", bad)
    counts = replay(tmp_path / "bad.fzm", {"FLOWZ_HIP_CACHE": str(tmp_path / "cache")})
    assert counts["failed"] == len(bad) and counts["built"] == 0 and counts["at_hand"] == 0, counts
    # and the same record with the right numbers is built
    write_manifest(tmp_path / "good.fzm", [(R, C_, block, RING_SM, ring_recipe), (4, 4, 64, RING_LOSS_SM, refused_recipe)])   # (checkpoint_rows = 4: taken)
    counts = replay(tmp_path / "good.fzm", {"FLOWZ_HIP_CACHE": str(tmp_path / "cache")})
    assert counts["failed"] == 0 and counts["built"] == 2, counts


# ---- the restatement on transposed arrays ------------------------------------------------------------------------------------------------
def test_the_transposition_helpers_round_trip():
    rng = np.random.default_rng(3)
    a = rng.standard_normal((13, 5, 2)).astype(F32)
    for rows, row0 in ((None, 0), (24, 4), (16, 3)):
        sm = RS.to_sm(a, rows, row0, fill=7.0)
        assert sm.shape == (5, RS.up4(row0 + 13) if rows is None else rows, 2) and np.array_equal(RS.from_sm(sm, 13, row0), a)
        keep = np.ones(sm.shape[1], bool)
        keep[row0:row0 + 13] = False
        assert np.all(sm[:, keep] == 7.0)
    assert [RS.up4(n) for n in (0, 1, 4, 5)] == [0, 4, 4, 8]


@pytest.mark.parametrize("name", ["lds_ring_comb", "two_in"])
def test_the_restatement_on_transposed_arrays_is_its_own_answer(name):
    """stream-major buffers are the time-major frames transposed: the restatement of the window, transposed back, is the restatement"""
    p = RS.prog(name)
    ns, T, row0 = 5, RS.DEEPEST[name] + 3, 4
    x, s0, par, yb, sb, ap, ac = RG.inputs(p, ns, T, 17)
    want = A.grad(p, x, yb, s0, par, sb, ap, ac)
    xs, ys = RS.to_sm(x, None, row0, 7.0), RS.to_sm(yb, None, row0, 7.0)
    got = A.grad(p, RS.from_sm(xs, T, row0), RS.from_sm(ys, T, row0), s0, par, sb, ap, ac)
    for k in want:
        assert np.array_equal(np.asarray(got[k]).view(np.uint32), np.asarray(want[k]).view(np.uint32)), k
    gx = RS.to_sm(got["x"], xs.shape[1], row0, fill=-1234.5)
    assert np.array_equal(RS.from_sm(gx, T, row0), want["x"])
