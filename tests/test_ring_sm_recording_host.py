"""The backward of a whole recording with deep delay lines on stream-major buffers, without a GPU
(fz_run_recording_ring_grad_stream_major, fz_run_recording_ring_loss_grad_stream_major): the exports, the scope and the refusals that
stay, the calls they ARE for a graph without a deep line, the rule that chooses the states kernel's workgroup and patch length together
(restated in tests/ring_sm_recording.py) with the figures derived by hand, the kernel's resources and instructions (JIT for gfx950: no
scratch, no VGPR spill, no FMA, no barrier, no atomic), every argument check with its reason, the kernel manifest of the GPU tests,
the code pins' names for every kernel, and the restatement on transposed arrays."""
import ctypes
import os
import re

import numpy as np
import pytest

import grad_graphs as GG
import grad_harness as H
import recording_ref as RR
import adjoint_ref as A
import ring_grad_graphs as RG
import ring_recording_graphs as R
import ring_sm_graphs as RS
import ring_sm_recording as S
from grad_harness import same
from grad_host_harness import (ADJOINT, ADJOINT_LOSS, ADJOINT_RING, ADJOINT_SM, LDS_BYTES, STATES, FakeCall, assert_no_contraction, code_objects, code_pins,
                               empty_args, invalid, kernel_ops, recipe_of, replay, write_manifest)
from zignal_amd import _capi as C
from zignal_amd import flowz as F

F32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
BITS = ADJOINT | STATES | ADJOINT_RING | ADJOINT_SM
NEW_EXPORTS = ("fz_run_recording_ring_grad_stream_major", "fz_run_recording_ring_loss_grad_stream_major", "fz_program_ring_states_resources_for",
               "fz_program_ring_states_kernel_symbol_for", "fz_program_ring_states_source_for")
NAMES = sorted(S.GRAPHS)


def run_fn(loss):
    return getattr(C.lib, H.ENTRY[(True, loss, True, True)])


def three_wires():
    return F.compile(F.from_sexpr(RS.three_wires_612()))


def test_the_new_entry_points_are_declared_and_exported():
    header = open(os.path.join(HERE, "..", "include", "flowz_hip.h")).read()
    for name in NEW_EXPORTS:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in C.EXPORTS and getattr(C.lib, name)
    for name in ("run_recording_ring_grad_stream_major", "run_recording_ring_loss_grad_stream_major"):
        assert callable(getattr(F.Program, name)), name
    p = S.prog("fb9")
    with pytest.raises(F.FlowzError) as ei:                       # the layout is FZ_GRAD_TIME_MAJOR or FZ_GRAD_STREAM_MAJOR
        C.check(C.lib.fz_program_ring_states_kernel_symbol_for(p._h, 2, None, 0))
    assert ei.value.code == C.FZ_E_INVALID and "layout" in str(ei.value)
    # time-major through the _for calls: the calls without a layout
    assert p.ring_states_kernel_symbol(stream_major=False) == F._name(C.lib.fz_program_ring_states_kernel_symbol, p._h)
    assert p.ring_states_source(False) == F._text(C.lib.fz_program_ring_states_source, p._h)
    assert p.ring_states_resources(False) == F._resources(C.lib.fz_program_ring_states_resources, p._h)
    import inspect
    from zignal_amd import autograd as AG
    assert inspect.signature(AG.mse_recording_rings).parameters["stream_major"].default is False


# ---- scope -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_the_ten_graphs_are_taken(name):
    p = S.prog(name)
    sym = p.ring_states_kernel_symbol(stream_major=True)
    U, R_, block = S.symbol_geometry(sym)
    assert sym.split("_g")[1] == p.ring_grad_kernel_symbol().split("_g")[1]          # the ring adjoint kernel's graph tag
    src = p.ring_states_source(stream_major=True)
    text = S.compiled_text(src)                                   # (the ring side of the one stream-major states text)
    assert sym in src and "#define FZ_RING 1 " in src and "fz_states_sm_args" in text
    assert "fz_adj::fwd(x[j], c, p, st, rv, sn, u)" in text and "fz_adj::fwd(x[j], c, p, st, sn)" not in text and "fz_apatch" not in text
    assert "if (active) fz_dump_state(sk, ns, st, ring, pos);" in text and "float fz_ring[FZ_RING_SLOTS * FZ_BLOCK" in text
    assert f"#define FZ_U {U} " in src and f"#define FZ_R {R_} " in src and f"#define FZ_BLOCK {block}\n" in src and "#define FZ_RING_SLOTS " in src
    assert "fz_patch_fetch<FZ_API>(patch, " in src and "\n//@splice" not in src
    assert "__syncthreads" not in src and "atomic" not in src.split("extern \"C\"")[1] and "xb[" not in src.split("extern \"C\"")[1]
    for loss in (False, True):
        for ns, T in ((0, 100), (100, 0), (0, 0)):                # an empty recording is FZ_OK with nothing touched
            assert run_fn(loss)(p._h, ctypes.byref(empty_args(loss)), ns, 100, 0, T, 0, None, None) == C.FZ_OK, C.last_error()


@pytest.mark.parametrize("sm", (False, True))
def test_each_layout_has_one_states_text_and_the_ring_is_a_switch(sm):
    """the hand-written part of a plain graph's states source and of a ring graph's ring states source is the same string, every
    `//@splice` line replaced; FZ_RING of the configuration chooses: the plain kernel compiles nothing of the rings"""
    plain = F.compile(F.from_sexpr(GG.SUPPORTED["df1_cascade6"]())).states_source(sm)
    ring = S.prog("biquad_comb17").ring_states_source(stream_major=sm)
    assert plain.count(S.HAND_WRITTEN) == 1 and ring.count(S.HAND_WRITTEN) == 1
    assert S.hand_written(plain) == S.hand_written(ring) and not re.search(r"(?m)^//@splice", S.hand_written(plain))
    assert "#define FZ_RING 0 " in plain and "#define FZ_RING 1 " in ring
    assert plain.split(S.HAND_WRITTEN)[0] != ring.split(S.HAND_WRITTEN)[0]
    text = S.compiled_text(plain)
    for word in ("fz_ring", "FZ_RING_SLOTS", "fz_dump_state(", "fz_reg_row", "pos[", "rv["):
        assert word not in text, word
    assert f"fz_adj::fwd({'x' if sm else 'xa'}[j], c, p, st, sn)" in text and "#define FZ_NREG FZ_NSTATE" in text
    assert "fz_ring" in S.compiled_text(ring) and "#define FZ_NREG FZ_NSTATE" not in S.compiled_text(ring)
    # a graph without a ring line asked through the ring calls IS the plain kernel: the same source, switch and all
    assert F.compile(F.from_sexpr(GG.SUPPORTED["df1_cascade6"]())).ring_states_source(stream_major=sm) == plain


def test_rings_that_fit_no_workgroup_keep_the_refusal_of_the_ring_check():
    p = F.compile(F.from_sexpr(RG.six_lines_256()))
    assert C.lib.fz_program_ring_grad_check(p._h) == C.FZ_E_UNSUPPORTED
    why = C.last_error()
    assert "393216 bytes" in why
    for loss in (False, True):
        for ns, T in ((64, 16), (0, 0)):
            assert run_fn(loss)(p._h, ctypes.byref(empty_args(loss)), ns, 16, 0, T, 0, None, None) == C.FZ_E_UNSUPPORTED and C.last_error() == why
    for call in (p.ring_states_kernel_symbol, p.ring_states_source, p.ring_states_resources):
        with pytest.raises(F.FlowzError) as ei:
            call(stream_major=True)
        assert ei.value.code == C.FZ_E_UNSUPPORTED and why in str(ei.value)
    from zignal_amd import autograd as AG
    with pytest.raises(F.FlowzError) as ei:
        AG.mse_recording_rings(p, None, None, stream_major=True)
    assert ei.value.code == C.FZ_E_UNSUPPORTED and "393216" in str(ei.value)


@pytest.mark.parametrize("name", sorted(n for n in GG.REFUSED if n != "lds_ring_comb"))
def test_refusals_keep_their_reasons(name):
    build, typed, word = GG.REFUSED[name]
    p = F.compile(F.from_sexpr(build()), typed=typed)
    assert C.lib.fz_program_ring_grad_check(p._h) == C.FZ_E_UNSUPPORTED
    why = C.last_error()
    assert word.lower() in why.lower()
    for loss in (False, True):
        assert run_fn(loss)(p._h, ctypes.byref(empty_args(loss)), 64, 16, 0, 16, 0, None, None) == C.FZ_E_UNSUPPORTED and C.last_error() == why
    with pytest.raises(F.FlowzError) as ei:
        p.ring_states_kernel_symbol(stream_major=True)
    assert ei.value.code == C.FZ_E_UNSUPPORTED and why in str(ei.value)


def test_three_wires_612_is_refused_at_the_default_stride_and_taken_at_four():
    """its states kernel fits once (R = 8 at 64 lanes: exactly 163 840 bytes); its block kernel at the default stride C = 8 does not
    (165 888 bytes per 64 lanes) and at checkpoint_rows = 4 does: the recording is refused with the block kernel's reason, and taken"""
    p = three_wires()
    assert S.geometry(p) == (4, 8, 64)
    r = p.ring_states_resources(stream_major=True)
    assert r["lds_bytes"] == 163840 and r["scratch_bytes"] == 0 and r["vgpr_spills"] == 0
    for loss in (False, True):
        a = empty_args(loss)
        for ns, T in ((64, 16), (0, 0)):
            assert run_fn(loss)(p._h, ctypes.byref(a), ns, 16, 0, T, 0, None, None) == C.FZ_E_UNSUPPORTED
            why = C.last_error()
            assert "165888 bytes per 64 lanes" in why and "checkpoint_rows" in why, why
        run_sm = C.lib.fz_run_block_ring_loss_grad_stream_major if loss else C.lib.fz_run_block_ring_grad_stream_major
        assert run_sm(p._h, ctypes.byref(a), 64, 16, 0, 16, None) == C.FZ_E_UNSUPPORTED and C.last_error() == why     # (the block call's reason)
        a.checkpoint_rows = 4
        assert run_fn(loss)(p._h, ctypes.byref(a), 0, 16, 0, 16, 0, None, None) == C.FZ_OK, C.last_error()
        b = FakeCall(p, 100, 16, ring=True, loss=loss, window=(None, 0), recording=4, c=4)
        if C.lib.fz_device_count() == 0:
            assert b.run(b.args(checkpoint_rows=4)) == C.FZ_E_NO_DEVICE, C.last_error()


@pytest.mark.parametrize("name", sorted(GG.SUPPORTED))
def test_for_a_graph_without_a_ring_the_calls_are_the_stream_major_recording_calls(name):
    p = F.compile(F.from_sexpr(GG.SUPPORTED[name]()))
    assert p.ring_states_kernel_symbol(stream_major=True) == p.states_kernel_symbol(True)
    assert p.ring_states_source(stream_major=True) == p.states_source(True)
    for c in (0, 1, 8):
        for T in (1, 37, 4096):
            for B in (0, 4, 40):
                assert p.ring_recording_workspace_bytes(1000, T, B, c) == p.recording_workspace_bytes(1000, T, B, c, stream_major=True)
                assert p.ring_recording_block_rows(T, B, c) == p.recording_block_rows(T, B, c)
    if name in ("integrator", "moog_ladder"):
        assert p.ring_states_resources(stream_major=True) == p.states_resources(True)


def test_every_existing_stream_major_and_recording_call_still_refuses_the_ring_comb():
    p = S.prog("lds_ring_comb")
    g, l = empty_args(False), empty_args(True)
    calls = (lambda: C.lib.fz_run_block_grad_stream_major(p._h, ctypes.byref(g), 64, 16, 0, 16, None),
             lambda: C.lib.fz_run_block_loss_grad_stream_major(p._h, ctypes.byref(l), 64, 16, 0, 16, None),
             lambda: C.lib.fz_run_block_grad(p._h, ctypes.byref(g), 64, 16, None),
             lambda: C.lib.fz_run_block_loss_grad(p._h, ctypes.byref(l), 64, 16, None),
             lambda: C.lib.fz_run_recording_grad(p._h, ctypes.byref(g), 0, 64, 0, 0, 16, 0, None, None),
             lambda: C.lib.fz_run_recording_grad(p._h, ctypes.byref(g), 1, 64, 16, 0, 16, 0, None, None),
             lambda: C.lib.fz_run_recording_loss_grad(p._h, ctypes.byref(l), 0, 64, 0, 0, 16, 0, None, None),
             lambda: C.lib.fz_run_recording_loss_grad(p._h, ctypes.byref(l), 1, 64, 16, 0, 16, 0, None, None))
    for call in calls:
        assert call() == C.FZ_E_UNSUPPORTED and "LDS" in C.last_error()
    for call in (p.states_kernel_symbol, p.states_resources, p.states_source, lambda sm: p.recording_workspace_bytes(64, 16, stream_major=sm)):
        for sm in (False, True):
            with pytest.raises(F.FlowzError) as ei:
                call(sm)
            assert ei.value.code == C.FZ_E_UNSUPPORTED and "LDS" in str(ei.value)
    # the time-major ring recordings have no window: through Python a window is refused before the library is asked
    with pytest.raises(F.FlowzError, match="no window"):
        p.run_recording_ring_grad(np.zeros((16, 64, 1), F32), None, row0=4)
    with pytest.raises(F.FlowzError, match="no window"):
        p.run_recording_ring_loss_grad(np.zeros((16, 64, 1), F32), None, n_samples=8)


def test_a_forward_variant_naming_the_bits_is_refused_as_reserved():
    p = S.prog("fb9")
    for flags in (STATES | ADJOINT_RING | ADJOINT_SM, BITS):
        with pytest.raises(F.FlowzError) as ei:
            p.kernel_name(F.make_variant(1, 8, 256, flags), 4096, 64)
        assert ei.value.code == C.FZ_E_INVALID and "reserved" in str(ei.value)
        with pytest.raises(F.FlowzError):
            p.build(F.make_variant(1, 8, 256, flags))


# ---- the geometry rule -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_the_geometry_rule_is_its_restatement(name):
    p = S.prog(name)
    U, R_, block = S.geometry(p)
    assert block and S.symbol_geometry(p.ring_states_kernel_symbol(stream_major=True)) == (U, R_, block)
    r = p.ring_states_resources(stream_major=True)
    assert r["lds_bytes"] == S.lds_bytes(p, block, R_) <= LDS_BYTES and r["unroll"] == U
    assert R_ % 4 == 0 and R_ % U == 0 and max(4, U) <= R_ <= 2 * S.states_patch_rows(p)
    # the plain states kernel's U, twice its R at the most; the time-major ring states kernel's U
    plain = re.fullmatch(r"fz_states_ring_kernel_u(\d+)b(\d+)_g[0-9a-f]{8}", p.ring_states_kernel_symbol())
    assert int(plain.group(1)) == U


def test_the_stated_figures():
    """derived by hand from 4 * block * (slots + R * n_in + 4) and the order of the rule: R from R0 down, per R the block from 256 down,
    twice before once"""
    table = {"lds_ring_comb": (63, 1, 8, 64, 128, 67072), "tap256": (256, 1, 8, 32, 64, 74752), "fb9": (9, 1, 8, 64, 256, 78848)}
    for name, (slots, n_in, U, R_, block, lds) in table.items():
        p = S.prog(name)
        assert (RS.ring_slots(p), p.n_in) == (slots, n_in)
        assert S.symbol_geometry(p.ring_states_kernel_symbol(stream_major=True)) == (U, R_, block), name
        assert p.ring_states_resources(stream_major=True)["lds_bytes"] == lds == 4 * block * (slots + R_ * n_in + 4), name
    assert 2 * 67072 == 134144 <= LDS_BYTES < 2 * 4 * 256 * (63 + 64 + 4)            # lds_ring_comb: twice at 128 lanes, not at 256
    assert 4 * 64 * (256 + 64 + 4) == 82944 and 2 * 82944 == 165888 > LDS_BYTES      # tap256: R = 64 does not fit twice at 64 lanes
    assert 2 * 78848 <= LDS_BYTES                                                    # fb9: twice at 256 lanes
    t = three_wires()
    assert (RS.ring_slots(t), t.n_in) == (612, 3)
    assert S.symbol_geometry(t.ring_states_kernel_symbol(stream_major=True)) == (4, 8, 64)
    assert t.ring_states_resources(stream_major=True)["lds_bytes"] == 163840 == 4 * 64 * (612 + 8 * 3 + 4)
    assert 2 * 4 * 64 * (612 + 4 * 3 + 4) > LDS_BYTES and 4 * 64 * (612 + 16 * 3 + 4) > LDS_BYTES    # never twice; R = 16 not even once
    # the records test_ring_sm_host.py pins as records no maker makes stay unmade
    assert S.geometry(S.prog("lds_ring_comb")) not in ((16, 32, 128), (8, 32, 128))


def test_a_states_kernel_that_fits_no_workgroup_is_refused_with_the_bytes():
    """two wires read 256 samples back and a third 120: 632 samples of ring fit a workgroup of 64 lanes (161 792 bytes: the ring check
    takes it), but not with a patch of Rmin = 4 rows of 3 wires + 4 floats: 4 * 64 * (632 + 12 + 4) = 165 888 bytes"""
    from graphs import DEL, add
    p = F.compile(F.from_sexpr(add(add(DEL(1, 256), DEL(2, 256)), DEL(3, 120))))
    assert C.lib.fz_program_ring_grad_check(p._h) == C.FZ_OK and S.geometry(p) == (4, 4, 0)
    for call in (p.ring_states_kernel_symbol, p.ring_states_source, p.ring_states_resources):
        with pytest.raises(F.FlowzError) as ei:
            call(stream_major=True)
        assert ei.value.code == C.FZ_E_UNSUPPORTED and "165888 bytes per 64 lanes" in str(ei.value) and str(LDS_BYTES) in str(ei.value)
    for loss in (False, True):
        assert run_fn(loss)(p._h, ctypes.byref(empty_args(loss)), 0, 16, 0, 0, 0, None, None) == C.FZ_E_UNSUPPORTED and "165888" in C.last_error()
    assert p.ring_states_resources()["lds_bytes"] == 632 * 64 * 4                    # the time-major recording takes it


# ---- the kernel for gfx950 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_the_kernel_compiles_without_scratch_or_spill_and_has_no_fma_no_barrier_no_atomic(name, tmp_path, monkeypatch, capsys):
    """the method of test_ring_recording_host.py: the only fused operations are those of the correctly rounded division (five each) and
    square root (two each) expansions"""
    p, r, _, every = kernel_ops(monkeypatch, tmp_path, S.GRAPHS[name](), "ring_states_resources", least=10, stream_major=True)
    assert r["scratch_bytes"] == 0 and r["vgpr_spills"] == 0 and r["vgprs"] + r["agprs"] <= 256, r
    assert_no_contraction(every, divides=name == "ks_tanh11", lds=True)
    sym = p.ring_states_kernel_symbol(stream_major=True)
    with capsys.disabled():                                       # (SGPR spills are reported, not asserted: correct, slower)
        print(f"\n{sym}: {r['vgprs']} VGPRs, {r['sgprs']} SGPRs, {r['sgpr_spills']} SGPR spills, {r['lds_bytes']} B LDS")


# ---- argument checks: every one fails before the device is needed --------------------------------------------------------------------
@pytest.mark.parametrize("loss", [False, True])
@pytest.mark.parametrize("name", ["biquad_comb17", "two_out_fb"])
def test_argument_checks_fail_one_by_one_with_their_reason(name, loss):
    p = S.prog(name)                                              # inputs, outputs, a deep line, a per-stream coefficient
    assert p.n_in and p.n_out and p.n_param
    b = FakeCall(p, 1000, 36, ring=True, loss=loss, window=(48, 4), recording=8)
    assert b.ws == (5 * p.n_state) * 4000 + p.ring_grad_workspace_bytes(1000, 8)
    ybar = "target" if loss else "out_grad"
    a0 = b.args()
    size = ctypes.sizeof(a0)
    for bad in (size - 8, size + 8, 0, ctypes.sizeof(C.GradArgs if loss else C.LossGradArgs)):
        assert invalid(b.run(b.args(struct_size=bad)), "struct_size")
    assert invalid(b.run(b.args(checkpoint_rows=3)), "checkpoint_rows") and invalid(b.run(b.args(checkpoint_rows=64)), "checkpoint_rows")
    # the window: inside the buffers, and on the 4-float grid
    assert b.run(b.args(), rows=36, row0=4) == C.FZ_E_INVALID and b.run(b.args(), rows=32, row0=0) == C.FZ_E_INVALID
    odd = 1                                                       # (one or two floats per row: an odd row count is off the grid)
    assert p.n_in in (1, 2) and p.n_out in (1, 2)
    assert invalid(b.run(b.args(), rows=48 + odd), "rows_total * n_in") and "multiples of 4" in C.last_error()
    assert invalid(b.run(b.args(), row0=4 + odd, rows=48), "row0 * n_in") and "multiples of 4" in C.last_error()
    # a block_rows whose block windows break the rule: the second block's window starts at row0 + B
    assert invalid(b.run(b.args(workspace_bytes=1 << 40), B=4 + odd), "row0 * n_in"), C.last_error()
    assert invalid(b.run(b.args(**{ybar: None})), ybar)
    assert invalid(b.run(b.args(in_=None)), "in is null") and invalid(b.run(b.args(state=None)), "state") and invalid(b.run(b.args(params=None)), "params")
    assert invalid(b.run(b.args(workspace=None)), "fz_program_ring_recording_workspace")
    assert invalid(b.run(b.args(workspace_bytes=b.ws - 4)), "fz_program_ring_recording_workspace")
    # (a workspace that would do for the one launch over the T rows is short for blocks of 4)
    assert p.ring_grad_workspace_bytes(1000, 36) < p.ring_recording_workspace_bytes(1000, 36, 4)
    assert invalid(b.run(b.args(workspace_bytes=p.ring_grad_workspace_bytes(1000, 36)), B=4), "fz_program_ring_recording_workspace")
    outs = ["in_grad", "workspace", "state0_grad", "param_grad"] + (["loss", "out"] if loss else [])
    for k in ["in_", ybar, "state", "params", "state_grad"] + outs:
        assert invalid(b.run(b.args(**{k: b.addr[k] + 4})), "aligned") and k.rstrip("_") in C.last_error(), k
    assert invalid(b.run(b.args(), state_out=b.addr["state_out"] + 4), "state_out")
    pairs = [("in_grad", ybar), ("state0_grad", ybar), ("in_grad", "in_"), ("param_grad", "workspace"), ("state0_grad", "state"), ("workspace", "in_")]
    pairs += [("loss", "target"), ("out", "in_"), ("out", "in_grad"), ("out", "target"), ("workspace", "out")] if loss else []
    for k, other in pairs:
        assert invalid(b.run(b.args(**{k: b.addr[other]})), "overlap"), (k, other)
        assert k in C.last_error() and other.rstrip("_") in C.last_error()
    # (a stream-major buffer counts over its whole extent, the rows outside the window too)
    assert invalid(b.run(b.args(), state_out=b.addr["in_"] + b.size["in_"] - 16), "overlap")
    assert invalid(b.run(b.args(state0_grad=b.addr["state_grad"] + 16)), "overlap")      # (only the exact alias of state_grad is allowed)
    for other in ("state", "in_", "workspace", "state0_grad", "param_grad"):             # state_out is an output: it overlaps nothing
        assert invalid(b.run(b.args(), state_out=b.addr[other]), "overlap") and "state_out" in C.last_error(), other
    assert invalid(b.run(b.args(), state_out=b.addr["workspace"] + b.ws - 16), "overlap")
    assert invalid(b.run(b.args(state0_grad=None)), "state0_grad")      # more than one block: they chain through it
    fn = run_fn(loss)
    assert fn(p._h, None, 10, 12, 0, 10, 0, None, None) == C.FZ_E_INVALID and "null arguments" in C.last_error()
    assert fn(None, ctypes.byref(a0), 10, 12, 0, 10, 0, None, None) == C.FZ_E_INVALID
    assert invalid(b.run(b.args(), T=1 << 31, rows=0, row0=0), "2^31")
    # the order of run_recording: the scope, the length, then the arguments
    assert invalid(b.run(b.args(in_=None), T=1 << 31), "2^31")
    big = FakeCall(p, 1, 4, ring=True, loss=loss, window=(None, 0), recording=0)
    assert big.run(big.args(), ns=1 << 30) == C.FZ_E_UNSUPPORTED and "2^30" in C.last_error()
    # an empty recording is FZ_OK and needs no buffer, but a bad struct_size is refused even then
    empty = empty_args(loss)
    for ns, T in ((0, 36), (1000, 0), (0, 0)):
        assert b.run(empty, ns=ns, T=T, state_out=None) == C.FZ_OK, C.last_error()
    empty.struct_size = 8
    assert b.run(empty, ns=0, T=0) == C.FZ_E_INVALID
    # what passes every check stops at the missing device (with one, fake addresses are not launched on)
    if C.lib.fz_device_count() == 0:
        assert b.run(b.args()) == C.FZ_E_NO_DEVICE, C.last_error()
        assert b.run(b.args(state0_grad=b.addr["state_grad"])) == C.FZ_E_NO_DEVICE, C.last_error()
        assert b.run(b.args(), state_out=None) == C.FZ_E_NO_DEVICE, C.last_error()
        assert b.run(b.args(), B=0) == C.FZ_E_NO_DEVICE and b.run(b.args(), B=40) == C.FZ_E_NO_DEVICE, C.last_error()
        assert b.run(b.args(workspace_bytes=2 * b.ws), B=4) == C.FZ_E_NO_DEVICE, C.last_error()
        optional = dict(in_grad=None, param_grad=None, const_grad=None, state_grad=None, **(dict(loss=None, out=None) if loss else {}))
        assert b.run(b.args(**optional), state_out=None) == C.FZ_E_NO_DEVICE, C.last_error()
        assert b.run(b.args(state0_grad=None, **optional), B=40, state_out=None) == C.FZ_E_NO_DEVICE, C.last_error()   # one block: no chain
        # one block: block_rows is on no grid of its own
        assert b.run(b.args(), B=37) == C.FZ_E_NO_DEVICE, C.last_error()


# ---- every kernel's name is the pinned one: tests/golden/adjoint_code_pins.json, held by test_adjoint_code_pins_host.py -----------------
PINS = code_pins()


def test_the_pinned_names_are_still_produced():
    pinned = {v[".text"] for v in PINS.values()}
    for name in NAMES:
        p = S.prog(name)
        assert PINS[f"ring_states/tm/{name}"]["symbol"] == p.ring_states_kernel_symbol() == p.ring_states_kernel_symbol(stream_major=False)
        for c in (0, 1, 4):
            for kind, symbol in (("ring", p.ring_grad_kernel_symbol), ("ring_loss", p.ring_loss_grad_kernel_symbol)):
                assert PINS[f"{kind}/tm/c{c}/{name}"]["symbol"] == symbol(c) and PINS[f"{kind}/sm/c{c}/{name}"]["symbol"] == symbol(c, stream_major=True)
        assert PINS[f"ring_states/sm/{name}"]["symbol"] == p.ring_states_kernel_symbol(stream_major=True)
    for name in sorted(GG.SUPPORTED):
        p = F.compile(F.from_sexpr(GG.SUPPORTED[name]()))
        for key, sm in (("tm", False), ("sm", True)):
            assert PINS[f"states/{key}/{name}"]["symbol"] == p.states_kernel_symbol(sm) == p.ring_states_kernel_symbol(stream_major=sm)
    assert len(pinned) > 1


# ---- the kernel manifest of the GPU tests ----------------------------------------------------------------------------------------------
def test_the_committed_manifest_holds_exactly_the_kernels_the_gpu_tests_launch():
    recs = S.manifest_variants(S.MANIFEST)
    progs = [S.prog(n) for n in NAMES]
    new = [v for v in recs if v[3] == BITS]
    assert sorted(v[:3] for v in new) == sorted((S.geometry(p)[1], S.geometry(p)[0], S.geometry(p)[2]) for p in progs)
    assert len({v[4] for v in new}) == len(NAMES)                 # one recipe per graph
    ring = ADJOINT | ADJOINT_RING
    for bits, loss in ((ring | ADJOINT_SM, False), (ring | ADJOINT_SM | ADJOINT_LOSS, True)):
        want = sorted((RS.geometry(p, c)[1], RS.geometry(p, c)[0], RS.geometry(p, c)[2], bits) for p in progs for c in S.STRIDES)
        assert sorted(v[:4] for v in recs if v[3] == bits) == want, loss
    # nothing else but the time-major kernels compared with and the stream-major forward kernels of the state comparison
    others = [v for v in recs if v[3] & ADJOINT and not v[3] & ADJOINT_SM]
    assert sorted({v[3] for v in others}) == sorted({ring, ring | ADJOINT_LOSS, ring | STATES}) and all(v[0] == 1 for v in others)
    forward = [v for v in recs if not v[3] & ADJOINT]
    assert all(not (v[3] & (ADJOINT_LOSS | ADJOINT_RING | STATES)) for v in forward)
    assert len(recs) == len(set(recs)) == 10 * len(NAMES) + len(forward) <= 120
    counts = replay(S.MANIFEST)
    assert counts["failed"] == 0 and counts["records"] == len(recs), counts


def test_a_manifest_cannot_ask_for_a_states_kernel_the_recording_would_not_make(tmp_path):
    """a wrong block, R / 2, 2 R, a U that is not the rule's, the loss next to the bits, a graph without a ring line, a graph the call
    refuses: counted as failed, nothing built; the right record is built"""
    p = S.prog("lds_ring_comb")
    U, R_, block = S.geometry(p)
    recipe = next(v[4] for v in S.manifest_variants(S.MANIFEST) if v[:4] == (R_, U, block, BITS))

    plain, refused = recipe_of(GG.SUPPORTED["integrator"]()), recipe_of(RG.six_lines_256())
    bad = [(R_, U, 256 if block != 256 else 128, BITS, recipe), (R_, U, 64 if block != 64 else 128, BITS, recipe), (R_, U, 512, BITS, recipe),
           (R_ // 2, U, block, BITS, recipe), (2 * R_, U, block, BITS, recipe), (1, U, block, BITS, recipe),
           (R_, U // 2, block, BITS, recipe), (R_, 2 * U, block, BITS, recipe), (R_, 0, block, BITS, recipe),
           (R_, U, block, BITS | ADJOINT_LOSS, recipe), (R_, U, block, BITS | 256, recipe),
           (32, 8, 256, BITS, plain), (4, 4, 64, BITS | ADJOINT_LOSS, plain), (8, 8, 64, BITS, refused)]
    write_manifest(tmp_path / "bad.fzm", bad)
    counts = replay(tmp_path / "bad.fzm", {"FLOWZ_HIP_CACHE": str(tmp_path / "cache")})
    assert counts["failed"] == len(bad) and counts["built"] == 0 and counts["at_hand"] == 0, counts
    write_manifest(tmp_path / "good.fzm", [(R_, U, block, BITS, recipe)])
    counts = replay(tmp_path / "good.fzm", {"FLOWZ_HIP_CACHE": str(tmp_path / "cache")})
    assert counts["failed"] == 0 and counts["built"] == 1, counts
    assert len(code_objects(tmp_path / "cache")) == 1


# ---- the restatement on transposed arrays ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_the_restatement_on_transposed_arrays_is_its_own_answer(name):
    """stream-major buffers are the time-major frames transposed: recording_ref.grad on the window's rows, transposed back, is
    recording_ref.grad on the time-major arrays, at every case and both windows"""
    p = S.prog(name)
    for (ns, T, B), c in S.cases(name):
        d = R.case(name, ns, T)
        x, s0, par, yb, tg, sb, ap, ac, al = d
        Be = p.ring_recording_block_rows(T, B, c)
        assert Be == R.block_rows(T, c or R.stride(p), p.n_state, *R.COUNTS[name], B)
        for rows, row0 in S.windows(T):
            assert rows % 4 == 0 and row0 % 4 == 0 and row0 + T <= rows and (row0 == 0 or rows > row0 + T)
            xs, ts, ys = (H.to_sm(a, rows, row0, H.FILL) for a in (x, tg, yb))
            assert same(H.from_sm(xs, T, row0), x) and same(H.from_sm(ts, T, row0), tg) and same(H.from_sm(ys, T, row0), yb)
        rows, row0 = S.windows(T)[1]
        kw = dict(state=s0, params=par, state_grad=sb, accum_params=ap, accum_consts=ac, ref=A)
        xs = H.from_sm(H.to_sm(x, rows, row0, H.FILL), T, row0)
        for loss in (False, True):
            if loss:
                got = RR.grad(p, xs, Be, target=H.from_sm(H.to_sm(tg, rows, row0, H.FILL), T, row0), k=S.K, accum_loss=al, **kw)
            else:
                got = RR.grad(p, xs, Be, out_grad=H.from_sm(H.to_sm(yb, rows, row0, H.FILL), T, row0), **kw)
            want = R.want(name, ns, T, B, loss, c)
            assert set(got) == set(want)
            for k in want:
                assert same(got[k], want[k]), (name, ns, T, B, k)
