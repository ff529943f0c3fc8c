"""The far recording calls with the layout as an argument, without a GPU (fz_run_recording_far_grad_for,
fz_run_recording_far_loss_grad_for: with FZ_GRAD_STREAM_MAJOR the backward of a whole recording whose graph has delay lines deeper
than 256 samples on a [batch, time] tensor as it lies): the exports and the three names that stay absent; layout 0 against the calls
without a layout; the scope and the refusals every other call keeps; the far-free and ring-free identities; the geometry rule against
its restatement and the figures stated by hand, and its LDS refusal; every argument check; workspace and block rows against the
time-major queries; the eight new kernels' resources, instructions and prefetch table (JIT for gfx950); the kernel manifest of the GPU
tests; and tests/far_recording_ref.py on transposed arrays."""
import ctypes
import re

import numpy as np
import pytest

import far_recording_graphs as FRG
import far_recording_ref as RR
import far_sm_recording as S
import grad_graphs as GG
import grad_harness as H
import ring_grad_graphs as RG
from grad_harness import same
from grad_host_harness import (ADJOINT, ADJOINT_FAR, ADJOINT_LOSS, ADJOINT_RING, ADJOINT_SM, LDS_BYTES, STATES, FakeCall, assert_no_contraction, code_objects,
                               empty_args, invalid, kernel_ops, recipe_of, replay, symbol_shape, write_manifest)
from zignal_amd import _capi as C
from zignal_amd import flowz as F

F32 = np.float32
NAMES = S.NAMES
FAR_BITS = ADJOINT | ADJOINT_RING | ADJOINT_FAR
BITS = FAR_BITS | STATES | ADJOINT_SM                              # the new kernel's
K = S.K
prog = S.prog


def run_fn(loss):
    return getattr(C.lib, S.ENTRY[loss])


def fake_call(p, ns, T, loss, B, window, c=0):
    """grad_host_harness.FakeCall at this corner: window None -- layout 0 --, or (rows, row0)"""
    b = FakeCall(S.AsPlainFamily(p), ns, T, loss=loss, window=window, recording=B, c=c)
    b.fn = run_fn(loss)
    return b


# ---- the surface ---------------------------------------------------------------------------------------------------------------------------
NEW = ("fz_run_recording_far_grad_for", "fz_run_recording_far_loss_grad_for", "fz_program_far_states_resources_for",
       "fz_program_far_states_kernel_symbol_for", "fz_program_far_states_source_for")


def test_the_new_entry_points_are_declared_and_exported_and_the_pinned_names_stay_absent():
    header = open(F.__file__.replace("zignal_amd/flowz.py", "include/flowz_hip.h")).read()
    for fn in NEW:
        assert re.search(r"\b(int|long) %s\(" % fn, header), fn
        assert getattr(C.lib, fn)
    for absent in ("fz_run_recording_far_grad_stream_major", "fz_run_recording_far_loss_grad_stream_major"):
        assert not hasattr(C.lib, absent) and not re.search(r"\b%s\(" % absent, header)
    assert not hasattr(F.Program, "run_recording_far_grad_stream_major") and not hasattr(F.Program, "run_recording_far_loss_grad_stream_major")
    import inspect
    from zignal_amd import autograd as AG
    assert inspect.signature(AG.mse_recording_far).parameters["stream_major"].default is False
    for fn in (F.Program.run_recording_far_grad, F.Program.run_recording_far_loss_grad):
        par = inspect.signature(fn).parameters
        assert (par["stream_major"].default, par["row0"].default, par["n_samples"].default, par["in_grad"].default) == (False, 0, None, None)
    for fn in (F.Program.far_states_resources, F.Program.far_states_kernel_symbol, F.Program.far_states_source):
        assert inspect.signature(fn).parameters["stream_major"].default is False


# ---- layout 0 IS the call without a layout ---------------------------------------------------------------------------------------------------
def text(fn, p, *args):
    buf = ctypes.create_string_buffer(1 << 20)
    n = fn(p._h, *args, buf, 1 << 20)
    assert 0 < n < 1 << 20, C.last_error()
    return buf.raw[:n]


@pytest.mark.parametrize("name", NAMES)
def test_layout_zero_of_the_inspectors_answers_what_the_calls_without_a_layout_answer(name):
    p = prog(name)
    assert text(C.lib.fz_program_far_states_kernel_symbol_for, p, 0) == text(C.lib.fz_program_far_states_kernel_symbol, p)
    assert text(C.lib.fz_program_far_states_source_for, p, 0) == text(C.lib.fz_program_far_states_source, p)
    a, b = C.KernelResources(), C.KernelResources()
    assert C.lib.fz_program_far_states_resources_for(p._h, 0, ctypes.byref(a)) == C.FZ_OK == C.lib.fz_program_far_states_resources(p._h, ctypes.byref(b))
    assert bytes(a) == bytes(b)
    assert p.far_states_kernel_symbol() == p.far_states_kernel_symbol(stream_major=False) and p.far_states_resources() == p.far_states_resources(False)
    buf = ctypes.create_string_buffer(64)
    assert C.lib.fz_program_far_states_kernel_symbol_for(p._h, 2, buf, 64) < 0 and "layout" in C.last_error()


@pytest.mark.parametrize("loss", [False, True])
def test_layout_zero_of_the_run_calls_is_the_time_major_call(loss):
    """the same answers to the same fake calls: what passes stops at the missing device, what fails fails with the same words"""
    p = prog("far_mixed")
    old = C.lib.fz_run_recording_far_loss_grad if loss else C.lib.fz_run_recording_far_grad
    b = fake_call(p, 1000, 700, loss, 64, None)
    assert b.ws == p.far_recording_workspace_bytes(1000, 700, 64)

    def both(a, T=700, B=64, so="given"):
        so = b.addr["state_out"] if so == "given" else so
        new = b.run(a, T=T, B=B, state_out=so), C.last_error()
        ref = old(p._h, ctypes.byref(a), 1000, T, B, so, None), C.last_error()
        assert new[0] == ref[0] and (new[0] in (C.FZ_OK, C.FZ_E_NO_DEVICE) or new[1] == ref[1]), (new, ref)
        return new[0]
    if C.lib.fz_device_count() == 0:
        assert both(b.args()) == C.FZ_E_NO_DEVICE and both(b.args(), B=0, so=None) == C.FZ_E_NO_DEVICE
    assert both(b.args(in_=None)) == C.FZ_E_INVALID and both(b.args(workspace_bytes=b.ws - 4)) == C.FZ_E_INVALID
    assert both(b.args(), B=6) == C.FZ_E_INVALID and "multiple of 4" in C.last_error()
    assert both(b.args(state0_grad=None)) == C.FZ_E_INVALID and both(b.args(), T=1 << 31) == C.FZ_E_INVALID
    assert both(empty_args(loss), T=0) == C.FZ_OK
    # no window: run_recording's rule for time-major frames
    assert invalid(b.run(b.args(), rows=704, row0=0), "no window") and invalid(b.run(b.args(), rows=700, row0=4), "no window")
    if C.lib.fz_device_count() == 0:
        assert b.run(b.args(), rows=700) == C.FZ_E_NO_DEVICE
    assert invalid(run_fn(loss)(p._h, ctypes.byref(b.args()), 2, 1000, 0, 0, 700, 64, None, None), "layout")


# ---- scope ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_the_eight_graphs_are_taken_and_every_existing_stream_major_and_recording_call_keeps_refusing_them(name):
    p = prog(name)
    sym = p.far_states_kernel_symbol(stream_major=True)
    assert S.SYMBOL.fullmatch(sym), sym
    assert sym.split("_g")[1] == p.kernel_symbol().split("_g")[-1]
    assert "fz_states_sm_args" in p.far_states_source(stream_major=True) and "fz_states_sm_args" not in p.far_states_source()
    g, a = empty_args(False), empty_args(True)
    hbm = lambda rc: rc == C.FZ_E_UNSUPPORTED and "HBM" in C.last_error()     # noqa: E731
    assert hbm(C.lib.fz_run_recording_ring_grad_stream_major(p._h, ctypes.byref(g), 64, 16, 0, 16, 0, None, None))
    assert hbm(C.lib.fz_run_recording_ring_loss_grad_stream_major(p._h, ctypes.byref(a), 64, 16, 0, 16, 0, None, None))
    assert hbm(C.lib.fz_run_recording_ring_grad(p._h, ctypes.byref(g), 64, 16, 0, None, None))
    assert hbm(C.lib.fz_run_block_ring_grad_stream_major(p._h, ctypes.byref(g), 64, 16, 0, 16, None))
    deep = lambda rc: rc == C.FZ_E_UNSUPPORTED and ("HBM" in C.last_error() or (name == "far_mixed" and "LDS" in C.last_error()))     # noqa: E731
    assert deep(C.lib.fz_run_recording_grad(p._h, ctypes.byref(g), 1, 64, 16, 0, 16, 0, None, None))
    assert deep(C.lib.fz_run_recording_loss_grad(p._h, ctypes.byref(a), 1, 64, 16, 0, 16, 0, None, None))
    for call in (lambda: p.ring_states_resources(True), lambda: p.ring_states_kernel_symbol(True), lambda: p.ring_states_source(True)):
        with pytest.raises(F.FlowzError) as ei:
            call()
        assert ei.value.code == C.FZ_E_UNSUPPORTED and "HBM" in str(ei.value)
    with pytest.raises(F.FlowzError) as ei:
        p.states_resources(True)
    assert ei.value.code == C.FZ_E_UNSUPPORTED
    with pytest.raises(F.FlowzError):                              # the forward stream-major plan: no body for rings in HBM
        p.kernel_name(F.make_variant(0, 0, 0, F.C.FZ_VF_STREAM_MAJOR), 4096, 64)


@pytest.mark.parametrize("name", sorted(n for n in GG.REFUSED if n not in ("lds_ring_comb", "far_comb")))
def test_refusals_of_the_far_check_keep_their_words(name):
    """double and complex far lines among them"""
    build, typed, word = GG.REFUSED[name]
    p = F.compile(F.from_sexpr(build()), typed=typed)
    assert C.lib.fz_program_far_grad_check(p._h) == C.FZ_E_UNSUPPORTED
    why = C.last_error()
    assert word.lower() in why.lower()
    for call in (p.far_states_resources, p.far_states_kernel_symbol, p.far_states_source):
        with pytest.raises(F.FlowzError) as ei:
            call(stream_major=True)
        assert ei.value.code == C.FZ_E_UNSUPPORTED and str(ei.value).endswith(why)
    for loss in (False, True):
        a = empty_args(loss)
        assert run_fn(loss)(p._h, ctypes.byref(a), 1, 64, 16, 0, 16, 0, None, None) == C.FZ_E_UNSUPPORTED and C.last_error() == why
        assert run_fn(loss)(p._h, ctypes.byref(a), 1, 0, 0, 0, 0, 6, None, None) == C.FZ_E_UNSUPPORTED         # (the scope comes first)


def test_rings_that_fit_no_workgroup_keep_the_refusal_of_the_ring_check():
    p = F.compile(F.from_sexpr(RG.six_lines_256()))
    with pytest.raises(F.FlowzError) as ei:
        p.far_states_kernel_symbol(stream_major=True)
    assert ei.value.code == C.FZ_E_UNSUPPORTED and "393216" in str(ei.value) and str(LDS_BYTES) in str(ei.value)
    assert run_fn(False)(p._h, ctypes.byref(empty_args()), 1, 64, 16, 0, 16, 0, None, None) == C.FZ_E_UNSUPPORTED and "393216" in C.last_error()


# ---- the identities ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(RG.RINGS) + ["integrator", "df1_cascade6", "moog_ladder"])
def test_for_a_graph_without_a_far_line_the_calls_are_the_stream_major_ring_recording_calls(name):
    """and without a ring line the plain stream-major recording: the same states Variant (symbol, source), B and workspace; the same
    answers to the same fake calls"""
    ring = name in RG.RINGS
    p = F.compile(F.from_sexpr((RG.RINGS.get(name) or GG.SUPPORTED[name])()))
    try:
        want = p.ring_states_kernel_symbol(stream_major=True)
    except F.FlowzError as er:                                      # (a ring graph whose states kernel fits no workgroup: the same refusal)
        with pytest.raises(F.FlowzError) as ei:
            p.far_states_kernel_symbol(stream_major=True)
        assert str(ei.value) == str(er)
        return
    assert p.far_states_kernel_symbol(stream_major=True) == want and p.far_states_source(stream_major=True) == p.ring_states_source(stream_major=True)
    assert p.far_states_resources(stream_major=True) == p.ring_states_resources(stream_major=True)
    if not ring:
        assert want == p.states_kernel_symbol(True)
    for T in (1, 36, 1000, 4096):
        for B in (0, 4, 40):
            assert p.far_recording_block_rows(T, B) == p.ring_recording_block_rows(T, B)
            assert p.far_recording_workspace_bytes(1000, T, B) == p.ring_recording_workspace_bytes(1000, T, B)
            if not ring:
                assert p.far_recording_workspace_bytes(1000, T, B) == p.recording_workspace_bytes(1000, T, B, 0, True)
    for loss in (False, True):
        if loss and not p.n_out:
            continue
        b = FakeCall(p, 1000, 36, ring=True, loss=loss, window=(48, 4), recording=8)
        for over, kw in ((dict(), dict()), (dict(in_=None), dict()), (dict(workspace_bytes=8), dict()), (dict(), dict(row0=5)), (dict(state0_grad=None), dict())):
            ref = b.run(b.args(**over), **kw), C.last_error()
            new = run_fn(loss)(p._h, ctypes.byref(b.args(**over)), 1, 1000, 48, kw.get("row0", 4), 36, 8, b.addr["state_out"] if p.n_state else None, None), C.last_error()
            assert new[0] == ref[0] and (new[0] in (C.FZ_OK, C.FZ_E_NO_DEVICE) or new[1] == ref[1].replace("fz_program_ring_recording_workspace", "fz_program_far_recording_workspace")), (new, ref)


# ---- the geometry rule ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_the_geometry_rule_is_its_restatement(name):
    p = prog(name)
    U, R, block = S.geometry(p)
    assert block and S.symbol_geometry(p.far_states_kernel_symbol(stream_major=True)) == (U, R, block)
    r = p.far_states_resources(stream_major=True)
    assert r["lds_bytes"] == S.lds_bytes(p, block, R) <= LDS_BYTES and r["unroll"] == U
    assert R % U == 0 and R % 4 == 0 and R >= max(4, U)
    assert U == symbol_shape(p.far_states_kernel_symbol(), "u")[0]                            # the time-major far states kernel's U
    cfg = p.far_states_source(stream_major=True).split("// ==== fz_graph_body.h ====")[0]
    assert f"#define FZ_R {R} " in cfg and f"#define FZ_U {U} " in cfg and f"#define FZ_BLOCK {block}\n" in cfg
    assert "#define FZ_FAR 1 " in cfg and "#define FZ_RING 1 " in cfg and f"#define FZ_RING_SLOTS {S.lds_ring_slots(p)} " in cfg


def test_the_geometry_stated_by_hand():
    for name, (slots, n_in, U, R, block, lds) in S.TABLE.items():
        p = prog(name)
        assert (S.lds_ring_slots(p), p.n_in) == (slots, n_in), name
        assert S.symbol_geometry(p.far_states_kernel_symbol(stream_major=True)) == (U, R, block), name
        assert p.far_states_resources(stream_major=True)["lds_bytes"] == lds == 4 * block * (slots + R * n_in + 4), name
    assert 2 * 54272 == 108544 <= LDS_BYTES
    # half the ring states kernel's R0: the records test_far_sm_host.py and test_far_recording_host.py pin as ones no maker makes stay unmade
    assert S.geometry(prog("far_comb")) == (8, 32, 256) != (8, 16, 256)
    import ring_sm_recording as RS
    assert S.geometry(prog("far_comb"))[1] * 2 == 2 * RS.states_patch_rows(prog("far_comb"))   # (the ring rule's R0 is twice it)


def test_a_states_kernel_that_fits_no_workgroup_is_refused_with_the_bytes():
    """the refusal of the stream-major ring recording, in its words: 632 samples of LDS rings next to a far line on a fourth wire fit a
    workgroup of 64 lanes alone (161 792 bytes), but not with a patch of Rmin = 4 rows of 4 wires + 4 floats:
    4 * 64 * (632 + 16 + 4) = 166 912 bytes"""
    from graphs import DEL, add
    p = F.compile(F.from_sexpr(add(add(add(DEL(1, 256), DEL(2, 256)), DEL(3, 120)), DEL(4, 300))))
    assert C.lib.fz_program_far_grad_check(p._h) == C.FZ_OK and S.lds_ring_slots(p) == 632 and S.geometry(p) == (4, 4, 0)
    for call in (p.far_states_kernel_symbol, p.far_states_source, p.far_states_resources):
        with pytest.raises(F.FlowzError) as ei:
            call(stream_major=True)
        msg = str(ei.value)
        assert ei.value.code == C.FZ_E_UNSUPPORTED and "stream-major ring recording" in msg and "166912 bytes per 64 lanes" in msg and str(LDS_BYTES) in msg
    for loss in (False, True):
        assert run_fn(loss)(p._h, ctypes.byref(empty_args(loss)), 1, 0, 16, 0, 0, 0, None, None) == C.FZ_E_UNSUPPORTED and "166912" in C.last_error()
    assert p.far_states_resources()["lds_bytes"] == 632 * 64 * 4                     # the time-major far recording takes it


# ---- argument checks: every one fails before the device is needed ---------------------------------------------------------------------------
@pytest.mark.parametrize("loss", [False, True])
@pytest.mark.parametrize("name", ["far_comb", "far_mixed", "far_two_in"])
def test_argument_checks_fail_one_by_one_with_their_reason(name, loss):
    p = prog(name)
    b = fake_call(p, 1000, 700, loss, 64, (712, 4))
    assert b.ws == 11 * p.n_state * 4000 + p.far_grad_workspace_bytes(1000, 64) == p.far_recording_workspace_bytes(1000, 700, 64)
    ybar = "target" if loss else "out_grad"
    a0 = b.args()
    size = ctypes.sizeof(a0)
    for bad in (size - 8, size + 8, 0, ctypes.sizeof(C.GradArgs if loss else C.LossGradArgs)):
        assert invalid(b.run(b.args(struct_size=bad)), "struct_size")
    assert invalid(b.run(b.args(checkpoint_rows=3)), "checkpoint_rows") and invalid(b.run(b.args(checkpoint_rows=64)), "checkpoint_rows")
    # the window: inside the buffers, and on the 4-float grid
    assert b.run(b.args(), rows=700, row0=4) == C.FZ_E_INVALID and b.run(b.args(), rows=696, row0=0) == C.FZ_E_INVALID
    odd = 1                                                       # (one or two floats per row: an odd row count is off the grid)
    assert p.n_in in (1, 2) and p.n_out == 1
    assert invalid(b.run(b.args(), rows=712 + odd), "rows_total * n_in") and "multiples of 4" in C.last_error()
    assert invalid(b.run(b.args(), row0=4 + odd, rows=712), "row0 * n_in") and "multiples of 4" in C.last_error()
    # a block_rows whose block windows break the rule: the second block's window starts at row0 + B
    # (block_rows that keep the workspace within the room the fake addresses leave behind it)
    for B in (37, 50, 62):
        assert invalid(b.run(b.args(workspace_bytes=2 * b.ws), B=B), "row0 * n_in"), C.last_error()
    assert invalid(b.run(b.args(**{ybar: None})), ybar)
    assert invalid(b.run(b.args(in_=None)), "in is null") and invalid(b.run(b.args(state=None)), "state")
    if p.n_param:
        assert invalid(b.run(b.args(params=None)), "params")
    assert invalid(b.run(b.args(workspace=None)), "fz_program_far_recording_workspace")
    assert invalid(b.run(b.args(workspace_bytes=b.ws - 4)), "fz_program_far_recording_workspace")
    assert b.ws < p.far_recording_workspace_bytes(1000, 700, 4)
    assert invalid(b.run(b.args(), B=4), "fz_program_far_recording_workspace")
    outs = ["in_grad", "workspace", "state0_grad"] + (["param_grad"] if p.n_param else []) + (["loss", "out"] if loss else [])
    for k in ["in_", ybar, "state", "state_grad"] + (["params"] if p.n_param else []) + outs:
        assert invalid(b.run(b.args(**{k: b.addr[k] + 4})), "aligned") and k.rstrip("_") in C.last_error(), k
    assert invalid(b.run(b.args(), state_out=b.addr["state_out"] + 4), "state_out")
    pairs = [("in_grad", ybar), ("state0_grad", ybar), ("in_grad", "in_"), ("in_grad", "workspace"), ("state0_grad", "state"), ("workspace", "in_")]
    pairs += [("loss", "target"), ("out", "in_"), ("out", "in_grad"), ("out", "target"), ("workspace", "out")] if loss else []
    for k, other in pairs:
        assert invalid(b.run(b.args(**{k: b.addr[other]})), "overlap"), (k, other)
        assert k in C.last_error() and other.rstrip("_") in C.last_error()
    # (a stream-major buffer counts over its whole extent, the rows outside the window too)
    assert invalid(b.run(b.args(), state_out=b.addr["in_"] + b.size["in_"] - 16), "overlap")
    assert invalid(b.run(b.args(state0_grad=b.addr["state_grad"] + 16)), "overlap")      # (only the exact alias of state_grad is allowed)
    for other in ("state", "in_", "workspace", "state0_grad", "in_grad"):                  # state_out is an output: it overlaps nothing
        assert invalid(b.run(b.args(), state_out=b.addr[other]), "overlap") and "state_out" in C.last_error(), other
    # (the tail of the whole workspace counts -- also the rows behind `starts` the far states kernel keeps its working rings in)
    assert invalid(b.run(b.args(), state_out=b.addr["workspace"] + b.ws - 16), "overlap")
    assert invalid(b.run(b.args(), state_out=b.addr["workspace"] + 11 * p.n_state * 4000), "overlap")
    assert invalid(b.run(b.args(state0_grad=None)), "state0_grad is null")      # more than one block: they chain through it
    fn = run_fn(loss)
    assert fn(p._h, None, 1, 10, 12, 0, 10, 0, None, None) == C.FZ_E_INVALID and "null arguments" in C.last_error()
    assert fn(None, ctypes.byref(a0), 1, 10, 12, 0, 10, 0, None, None) == C.FZ_E_INVALID
    assert invalid(b.run(b.args(), T=1 << 31, rows=0, row0=0), "2^31")
    # the order of run_recording: the scope, the length, then the arguments
    assert invalid(b.run(b.args(in_=None), T=1 << 31), "2^31")
    big = fake_call(p, 1, 4, loss, 0, (None, 0))
    assert big.run(big.args(), ns=1 << 30) == C.FZ_E_UNSUPPORTED and "2^30" in C.last_error()
    # an empty recording is FZ_OK and needs no buffer, but a bad struct_size is refused even then
    empty = empty_args(loss)
    for ns, T in ((0, 700), (1000, 0), (0, 0)):
        assert b.run(empty, ns=ns, T=T, state_out=None) == C.FZ_OK, C.last_error()
    empty.struct_size = 8
    assert b.run(empty, ns=0, T=0) == C.FZ_E_INVALID
    # what passes every check stops at the missing device (with one, fake addresses are not launched on)
    if C.lib.fz_device_count() == 0:
        assert b.run(b.args()) == C.FZ_E_NO_DEVICE, C.last_error()
        assert b.run(b.args(state0_grad=b.addr["state_grad"])) == C.FZ_E_NO_DEVICE, C.last_error()
        assert b.run(b.args(), state_out=None) == C.FZ_E_NO_DEVICE, C.last_error()
        assert b.run(b.args(), B=0) == C.FZ_E_NO_DEVICE and b.run(b.args(), B=400) == C.FZ_E_NO_DEVICE, C.last_error()
        assert b.run(b.args(workspace_bytes=2 * b.ws), B=32) == C.FZ_E_NO_DEVICE, C.last_error()
        optional = dict(in_grad=None, param_grad=None, const_grad=None, state_grad=None, **(dict(loss=None, out=None) if loss else {}))
        assert b.run(b.args(**optional), state_out=None) == C.FZ_E_NO_DEVICE, C.last_error()
        assert b.run(b.args(state0_grad=None, **optional), B=700, state_out=None) == C.FZ_E_NO_DEVICE, C.last_error()   # one block: no chain
        assert b.run(b.args(), B=701) == C.FZ_E_NO_DEVICE, C.last_error()                    # one block: block_rows is on no grid of its own


# ---- B and the workspace do not depend on the layout -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_workspace_and_block_rows_are_the_time_major_queries(name):
    """one pair of queries answers both layouts: a call with exactly the queried bytes passes every check in either layout, four
    bytes less fail in both, over a grid"""
    if C.lib.fz_device_count():
        pytest.skip("fake addresses are not launched on")
    p = prog(name)
    for c in (0, 1):
        for T in (4, 36, 700, 4096):
            for B in (0, 4, 64, 4096):
                Be = p.far_recording_block_rows(T, B, c)
                assert Be == S.block_rows(name, T, B, c)
                ws = p.far_recording_workspace_bytes(1000, T, B, c)
                assert ws == FRG.workspace_bytes(name, 1000, T, c or symbol_shape(p.far_grad_kernel_symbol(), "c")[0], B)
                for window in (None, (H.up4(T) + 8, 4)):
                    b = fake_call(p, 1000, T, False, B, window, c)
                    assert b.ws == ws
                    assert b.run(b.args(checkpoint_rows=c)) == C.FZ_E_NO_DEVICE, (C.last_error(), c, T, B, window)
                    assert invalid(b.run(b.args(checkpoint_rows=c, workspace_bytes=ws - 4)), "fz_program_far_recording_workspace")


# ---- the eight kernels for gfx950 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_the_kernel_compiles_without_scratch_or_spill_and_has_no_fma_no_barrier_no_atomic(name, tmp_path, monkeypatch, capsys):
    p, r, _, every = kernel_ops(monkeypatch, tmp_path, S.FARS[name](), "far_states_resources", least=10, stream_major=True)
    U, R, block = S.geometry(p)
    assert r["scratch_bytes"] == 0 and r["vgpr_spills"] == 0 and r["vgprs"] + r["agprs"] <= 256, r
    assert r["lds_bytes"] == S.lds_bytes(p, block, R)
    assert_no_contraction(every, divides=name == "far_adjacent", lds=True)          # (the patch: every graph here has an input wire)
    assert "s_barrier" not in every and not [o for o in every if "atomic" in o]
    assert "v_readfirstlane_b32" in every                           # the phase: one per wave and far line
    sym = p.far_states_kernel_symbol(stream_major=True)
    with capsys.disabled():                                       # (SGPR spills are reported, not asserted: correct, slower)
        print(f"\n{sym}: {r['vgprs']} VGPRs, {r['sgprs']} SGPRs, {r['sgpr_spills']} SGPR spills, {r['lds_bytes']} B LDS")


def ahead(p):
    src = p.far_states_source(stream_major=True)
    m, d = re.search(r"fz_fr_ahead\[\d+\] = \{([^}]*)\}", src), re.search(r"fz_fr_delay\[\d+\] = \{([^}]*)\}", src)
    return [int(x.strip().rstrip("u")) for x in d.group(1).split(",")], [int(x.strip().rstrip("u")) for x in m.group(1).split(",")]


def test_the_prefetch_table_at_this_u():
    """a far read at a delay of at least 2 U travels a group ahead: far_tap1 at U = 8 has both kinds, 300 and 20 against 1"""
    assert ahead(prog("far_tap1")) == ([300, 1, 20], [1, 0, 1])
    for name in NAMES:
        U = S.geometry(prog(name))[0]
        delays, table = ahead(prog(name))
        assert table == [int(d >= 2 * U) for d in delays], name
        assert "fz_fr_chunked" not in prog(name).far_states_source(stream_major=True).split("// ==== fz_graph_body.h ====")[0]


# ---- the kernel manifest of the GPU tests ---------------------------------------------------------------------------------------------------
def test_the_committed_manifest_holds_exactly_the_kernels_the_gpu_tests_launch():
    recs = S.manifest_variants(S.MANIFEST)
    progs = [prog(n) for n in NAMES]
    new = [v for v in recs if v[3] == BITS]
    assert sorted(v[:3] for v in new) == sorted((S.geometry(p)[1], S.geometry(p)[0], S.geometry(p)[2]) for p in progs)
    assert len({v[4] for v in new}) == len(NAMES)                 # one recipe per graph
    for loss, sym in ((0, F.Program.far_grad_kernel_symbol), (ADJOINT_LOSS, F.Program.far_loss_grad_kernel_symbol)):
        bits = FAR_BITS | ADJOINT_SM | loss
        want = sorted((shape[1], shape[0], shape[2], bits) for shape in (symbol_shape(sym(p, c, stream_major=True), "c") for p in progs for c in S.STRIDES))
        assert sorted(v[:4] for v in recs if v[3] == bits) == want, loss
        assert sorted(v[:4] for v in recs if v[3] == FAR_BITS | loss) == sorted((1, *symbol_shape(sym(p, c), "c"), FAR_BITS | loss) for p in progs for c in S.STRIDES)
    assert sorted(v[:4] for v in recs if v[3] == FAR_BITS | STATES) == sorted((1, *symbol_shape(p.far_states_kernel_symbol(), "u"), FAR_BITS | STATES) for p in progs)
    # nothing else but the time-major forward kernels starts and state_out are compared with
    forward = [v for v in recs if not v[3] & ADJOINT]
    assert all(not (v[3] & (ADJOINT_LOSS | ADJOINT_RING | STATES)) for v in forward)
    assert len(recs) == len(set(recs)) == 10 * len(NAMES) + len(forward) <= 120
    counts = replay(S.MANIFEST)
    assert counts["failed"] == 0 and counts["records"] == len(recs), counts


def test_a_manifest_cannot_ask_for_a_states_kernel_the_recording_would_not_make(tmp_path):
    """a wrong block, R / 2, 2 R, P = 1, a wrong U, the loss beside STATES, a far-free recipe, a graph the check refuses: counted as
    failed, nothing built; the right record is built"""
    p = prog("far_comb")
    U, R, block = S.geometry(p)
    assert (U, R, block) == (8, 32, 256)
    recipe = next(v[4] for v in S.manifest_variants(S.MANIFEST) if v[:4] == (R, U, block, BITS) and v[4] == recipe_of(S.FARS["far_comb"]()))
    ring, plain, refused = recipe_of(RG.RINGS["fb9"]()), recipe_of(GG.SUPPORTED["integrator"]()), recipe_of(RG.six_lines_256())
    bad = [(R, U, 128, BITS, recipe), (R, U, 64, BITS, recipe), (R, U, 512, BITS, recipe),
           (R // 2, U, block, BITS, recipe), (2 * R, U, block, BITS, recipe), (1, U, block, BITS, recipe),
           (R, U // 2, block, BITS, recipe), (R, 2 * U, block, BITS, recipe), (R, 0, block, BITS, recipe),
           (R, U, block, BITS | ADJOINT_LOSS, recipe), (R, U, block, BITS | 256, recipe), (R, U, block, BITS & ~ADJOINT_RING, recipe),
           (R, U, block, BITS, ring), (R, U, block, BITS, plain), (R, U, 64, BITS, refused)]
    write_manifest(tmp_path / "bad.fzm", bad)
    counts = replay(tmp_path / "bad.fzm", {"FLOWZ_HIP_CACHE": str(tmp_path / "cache")})
    assert counts["failed"] == len(bad) and counts["built"] == 0 and counts["at_hand"] == 0, counts
    write_manifest(tmp_path / "good.fzm", [(R, U, block, BITS, recipe)])
    counts = replay(tmp_path / "good.fzm", {"FLOWZ_HIP_CACHE": str(tmp_path / "cache")})
    assert counts["failed"] == 0 and counts["built"] == 1, counts
    assert len(code_objects(tmp_path / "cache")) == 1


# ---- the restatement on transposed arrays ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_the_restatement_on_transposed_arrays_is_its_own_answer(name):
    """stream-major buffers are the time-major frames transposed: far_recording_ref.grad on the window's rows of the buffers, transposed
    back, is far_recording_ref.grad on the time-major arrays, at every case (both windows hold the same rows)"""
    p = prog(name)
    for ns, T, B, c in S.cases(name):
        Be = S.block_rows(name, T, B, c)
        assert Be == p.far_recording_block_rows(T, B, c) and (Be % 4 == 0 or Be == T)
        for loss in (False, True):
            d = S.inputs(name, ns, T, loss)
            x, s0, par, yt, sb, ap, ac = d[:7]
            back = []
            for rows, row0 in S.windows(T):
                assert rows % 4 == 0 and row0 % 4 == 0 and row0 + T <= rows and (row0 == 0 or rows > row0 + T)
                xs, ys = H.to_sm(x, rows, row0, H.FILL), H.to_sm(yt, rows, row0, H.FILL)
                assert xs.shape == (ns, rows, p.n_in)
                back.append((H.from_sm(xs, T, row0), H.from_sm(ys, T, row0)))
                assert same(back[-1][0], x) and same(back[-1][1], yt)
            kw = dict(state=s0, params=par, state_grad=sb, accum_params=ap, accum_consts=ac)
            if loss:
                got = RR.grad(p, back[1][0], Be, target=back[1][1], k=K, accum_loss=d[7], **kw)
                want = RR.grad(p, x, Be, target=yt, k=K, accum_loss=d[7], **kw)
            else:
                got, want = RR.grad(p, back[1][0], Be, out_grad=back[1][1], **kw), RR.grad(p, x, Be, out_grad=yt, **kw)
            assert set(got) == set(want)
            for key in want:
                assert want[key] is None and got[key] is None or same(got[key], want[key]), (name, ns, T, B, key)
