"""The backward of a whole recording without a GPU (fz_run_recording_grad, fz_run_recording_loss_grad): the workspace formula and the
block rule, the argument checks and refusals (all before a device is needed), the two block-start-states kernels' JIT for gfx950 (symbols
of their own, no scratch, no VGPR spills, the stated LDS), manifests, and tests/recording_ref.py -- the block-by-block restatement the
GPU test holds the calls to -- against the single-call restatements, bit for bit."""
import ctypes
import gzip
import os
import re

import numpy as np
import pytest

import adjoint_ref as A
import grad_fuzz_cells as GC
import grad_graphs as GG
import loss_grad_ref as LR
import recording_ref as RR
from grad_harness import make_inputs, same
from grad_host_harness import (ADJOINT, ADJOINT_LOSS, ADJOINT_SM, STATES, FakeCall, code_objects, empty_args, invalid, recipe_of, replay, symbol_shape,
                               write_manifest)
from zignal_amd import _capi as C
from zignal_amd import flowz as F

F32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
NEW_EXPORTS = ("fz_run_recording_grad", "fz_run_recording_loss_grad", "fz_program_recording_workspace", "fz_program_recording_block_rows",
               "fz_program_states_resources", "fz_program_states_kernel_symbol", "fz_program_states_source")
MANIFEST = os.path.join(HERE, "golden", "recording_kernels.fzm.gz")
TM, SM = 0, 1                                                     # FZ_GRAD_TIME_MAJOR, FZ_GRAD_STREAM_MAJOR
FIVE = ("integrator", "df1_cascade_params6", "moog_ladder", "par4_sum", "rules")


def prog_of(name):
    return F.compile(F.from_sexpr(GG.SUPPORTED[name]())) if name in GG.SUPPORTED else GC.prog(name)


def stride_of(p):
    return int(re.match(r"fz_adjoint_kernel_c(\d+)b", p.grad_kernel_symbol()).group(1))


def test_the_new_entry_points_are_declared_and_exported():
    header = open(os.path.join(HERE, "..", "include", "flowz_hip.h")).read()
    for name in NEW_EXPORTS:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in C.EXPORTS and getattr(C.lib, name)


# ---- workspace and the block rule ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIVE)
def test_workspace_is_the_stated_formula(name):
    p = prog_of(name)
    ceil = lambda a, b: (a + b - 1) // b                          # noqa: E731
    for c in (0, 1, 8):
        Cc = c or stride_of(p)
        for ns, T, B in ((1000, 37, 8), (1000, 37, 12), (65, 37, 40), (1, 8, 8), (4096, 4096, 0), (3, 48000, 0), (77, 100, 64), (5, 1, 0)):
            Be = RR.block_rows(T, Cc, B)
            assert p.recording_block_rows(T, B, c) == Be
            want = (ceil(T, Be) + ceil(Be, Cc)) * p.n_state * ns * 4
            for sm in (False, True):
                assert p.recording_workspace_bytes(ns, T, B, c, stream_major=sm) == want, (c, ns, T, B, sm)
    assert p.recording_workspace_bytes(100, 0) == 0 and p.recording_workspace_bytes(0, 100) == 0


def test_the_default_block_rule():
    """block_rows = 0: sqrt(T C) rounded up to a multiple of lcm(4, C), and T when that is not smaller -- worked out by hand here for
    C = 4 (df1_cascade_params6), C = 8 (moog_ladder) and C = 16 (integrator)"""
    by_hand = {4: {1: 1, 7: 7, 1024: 64, 48000: 440},               # sqrt(4096) = 64;  sqrt(192000) = 438.2 -> 440
               8: {1: 1, 7: 7, 1024: 96, 48000: 624},                # sqrt(8192) = 90.5 -> 96;  sqrt(384000) = 619.7 -> 624
               16: {1: 1, 7: 7, 1024: 128, 48000: 880}}              # sqrt(16384) = 128;  sqrt(768000) = 876.4 -> 880
    for name in ("df1_cascade_params6", "moog_ladder", "integrator"):
        p = prog_of(name)
        Cc = stride_of(p)
        for T, B in by_hand[Cc].items():
            assert p.recording_block_rows(T) == B == RR.block_rows(T, Cc), (name, T)
            assert p.recording_block_rows(T, 4 * T + 4) == T      # (a block_rows beyond T: one block)
    # the rule's B is what minimises the row sets kept among the multiples of lcm(4, C) below T and T itself
    for Cc, name in ((4, "df1_cascade_params6"), (16, "integrator")):
        p = prog_of(name)
        sets = lambda T, B: -(-B // Cc) - (-T // B)               # noqa: E731
        for T in (64, 100, 1000, 1024, 5000, 48000):
            B = p.recording_block_rows(T)
            assert sets(T, B) == min(sets(T, b) for b in list(range(max(4, Cc), T, max(4, Cc))) + [T]), (name, T)


@pytest.mark.parametrize("name", FIVE)
def test_the_workspace_is_smaller_than_the_one_launch_calls_from_64_rows_on(name):
    """Strictly smaller for every T >= 64 -- but for the checkpoint stride C = 16 (integrator) at 64 <= T <= 80.  There the one-launch
    call keeps ceil(T / 16) = 4 (T = 64) or 5 row sets, and no B keeps fewer: min over B of ceil(B / 16) + ceil(T / B) is 4 at T = 64
    (B = 32: 2 + 2) and 5 for 65 .. 80 (B = 32 or 48: 2 + 3, 3 + 2).  For those the two are EQUAL, which is what is asserted; from
    T = 81 on (6 against 3 + 2) and for every C <= 8 from T = 64 on it is strictly smaller."""
    p = prog_of(name)
    Cc = stride_of(p)
    for T in list(range(64, 2200)) + [4096, 16384, 48000, 1 << 20]:
        rec, one = p.recording_workspace_bytes(1000, T), p.grad_workspace_bytes(1000, T)
        if Cc == 16 and T <= 80:
            assert rec == one, (T, rec, one)
        else:
            assert rec < one, (T, rec, one)


# ---- argument checks: every one fails before the device is needed ------------------------------------------------------------------
@pytest.mark.parametrize("loss", [False, True])
@pytest.mark.parametrize("rows", [None, 48])
def test_argument_checks_fail_one_by_one_with_their_reason(rows, loss):
    p = prog_of("moog_ladder")                                    # 1 in, 1 out, state, a parameter and coefficients
    b = FakeCall(p, 1000, 37, loss=loss, window=rows and (rows, 0), recording=8)
    ybar = "target" if loss else "out_grad"
    a0 = b.args()
    size = ctypes.sizeof(a0)
    for bad in (size - 8, size + 8, 0):
        assert invalid(b.run(b.args(struct_size=bad)), "struct_size")
    assert invalid(b.run(b.args(checkpoint_rows=3)), "checkpoint_rows")
    assert invalid(b.run(b.args(**{ybar: None})), ybar)
    assert invalid(b.run(b.args(in_=None)), "in is null") and invalid(b.run(b.args(state=None)), "state") and invalid(b.run(b.args(params=None)), "params")
    assert invalid(b.run(b.args(workspace=None)), "fz_program_recording_workspace")
    assert invalid(b.run(b.args(workspace_bytes=b.ws - 4)), "fz_program_recording_workspace")
    outs = ["in_grad", "workspace"] + (["loss", "out"] if loss else [])
    for k in ["in_", ybar] + outs:
        assert invalid(b.run(b.args(**{k: b.addr[k] + 4})), "aligned"), k
    assert invalid(b.run(b.args(), state_out=b.addr["state_out"] + 4), "state_out")
    pairs = [("in_grad", ybar), ("state0_grad", ybar), ("in_grad", "in_"), ("param_grad", "workspace"), ("const_grad", "state")]
    pairs += [("loss", "target"), ("out", "in_"), ("out", "in_grad")] if loss else []
    for k, other in pairs:
        assert invalid(b.run(b.args(**{k: b.addr[other]})), "overlap"), (k, other)
        assert k in C.last_error() and other.rstrip("_") in C.last_error()
    for other in ("state", "in_", "workspace", "state0_grad", "param_grad"):      # state_out is an output: it overlaps nothing
        assert invalid(b.run(b.args(), state_out=b.addr[other]), "overlap") and "state_out" in C.last_error(), other
    # (the tail of the whole workspace counts, not only the block launches' share of it)
    assert invalid(b.run(b.args(), state_out=b.addr["workspace"] + b.ws - 16), "overlap")
    assert invalid(b.run(b.args(state0_grad=None)), "state0_grad")      # more than one block: they chain through it
    fn = b.fn
    assert fn(p._h, None, TM, 10, 0, 0, 10, 0, None, None) == C.FZ_E_INVALID and "null arguments" in C.last_error()
    assert fn(None, ctypes.byref(a0), TM, 10, 0, 0, 10, 0, None, None) == C.FZ_E_INVALID
    assert fn(p._h, ctypes.byref(a0), 2, 10, 0, 0, 10, 0, None, None) == C.FZ_E_INVALID and "layout" in C.last_error()
    assert invalid(b.run(b.args(), T=1 << 31), "2^31")
    if rows is None:
        for B in (1, 2, 6, 37):
            assert invalid(b.run(b.args(), B=B), "multiple of 4") and "16-byte" in C.last_error()
        assert fn(p._h, ctypes.byref(a0), TM, 1000, 37, 4, 37, 8, None, None) == C.FZ_E_INVALID and "row0" in C.last_error()
        assert fn(p._h, ctypes.byref(a0), TM, 1000, 40, 0, 37, 8, None, None) == C.FZ_E_INVALID and "rows_total" in C.last_error()
        with pytest.raises(F.FlowzError, match="multiple of 4"):
            p.recording_workspace_bytes(1000, 37, 6)
    else:                                                         # windows and alignment: every block's are fz_run_block_grad_stream_major's
        assert invalid(b.run(b.args(), rows=47), "rows_total") and invalid(b.run(b.args(), row0=2, T=8), "row0")
        assert invalid(b.run(b.args(), row0=12), "beyond rows_total")
        assert invalid(b.run(b.args(), rows=46, row0=5), "rows_total")      # T + 9 rows with the window at row 5: off the float4 grid for one wire
        assert invalid(b.run(b.args(workspace_bytes=2 * b.ws), B=6), "row0")              # the second block's window would start at row 6
    big = FakeCall(p, 1, 1, loss=loss, window=rows and (rows, 0), recording=0)
    assert big.run(big.args(), ns=1 << 30) == C.FZ_E_UNSUPPORTED and "2^30" in C.last_error()
    # what passes every check stops at the missing device (with one, fake addresses are not launched on)
    if C.lib.fz_device_count() == 0:
        assert b.run(b.args()) == C.FZ_E_NO_DEVICE, C.last_error()
        assert b.run(b.args(state0_grad=b.addr["state_grad"])) == C.FZ_E_NO_DEVICE, C.last_error()
        assert b.run(b.args(), state_out=None) == C.FZ_E_NO_DEVICE, C.last_error()
        assert b.run(b.args(), B=0) == C.FZ_E_NO_DEVICE and b.run(b.args(), B=40) == C.FZ_E_NO_DEVICE, C.last_error()
        if rows is not None:
            assert b.run(b.args(workspace_bytes=2 * b.ws), B=6, T=6) == C.FZ_E_NO_DEVICE, C.last_error()      # (one block: any block_rows)
        optional = dict(in_grad=None, param_grad=None, const_grad=None, state_grad=None, **(dict(loss=None, out=None) if loss else {}))
        assert b.run(b.args(**optional), state_out=None) == C.FZ_E_NO_DEVICE, C.last_error()
        assert b.run(b.args(state0_grad=None, **optional), B=40, state_out=None) == C.FZ_E_NO_DEVICE, C.last_error()   # one block: no chain


def test_an_empty_recording_is_ok_and_needs_no_buffer():
    p = prog_of("df1_cascade_params6")
    for args, fn in ((empty_args(), C.lib.fz_run_recording_grad), (empty_args(True), C.lib.fz_run_recording_loss_grad)):
        for ns, T in ((0, 100), (100, 0), (0, 0)):
            assert fn(p._h, ctypes.byref(args), TM, ns, 0, 0, T, 0, None, None) == C.FZ_OK, C.last_error()
            assert fn(p._h, ctypes.byref(args), SM, ns, 100, 0, T, 0, None, None) == C.FZ_OK, C.last_error()


@pytest.mark.parametrize("name", sorted(GG.REFUSED))
def test_refusals_are_the_backwards(name):
    build, typed, word = GG.REFUSED[name]
    p = F.compile(F.from_sexpr(build()), typed=typed)
    assert C.lib.fz_program_grad_check(p._h) == C.FZ_E_UNSUPPORTED
    why = C.last_error()
    assert word.lower() in why.lower()
    g, a = empty_args(), empty_args(True)
    for layout in (TM, SM):
        assert C.lib.fz_run_recording_grad(p._h, ctypes.byref(g), layout, 64, 16 * layout, 0, 16, 0, None, None) == C.FZ_E_UNSUPPORTED and C.last_error() == why
        assert C.lib.fz_run_recording_loss_grad(p._h, ctypes.byref(a), layout, 64, 16 * layout, 0, 16, 0, None, None) == C.FZ_E_UNSUPPORTED and C.last_error() == why
        for call in (p.states_kernel_symbol, p.states_resources, p.states_source, lambda sm: p.recording_workspace_bytes(64, 16, stream_major=sm)):
            with pytest.raises(F.FlowzError) as ei:
                call(bool(layout))
            assert ei.value.code == C.FZ_E_UNSUPPORTED and why in str(ei.value)
    with pytest.raises(F.FlowzError):
        p.recording_block_rows(16)


# ---- the block-start-states kernels for gfx950 -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(GG.SUPPORTED) + GC.CELLS)
def test_states_kernels_jit_compile_without_scratch_or_vgpr_spills(name, capsys):
    p = prog_of(name)
    lines = []
    for sm in (False, True):
        r, sym = p.states_resources(sm), p.states_kernel_symbol(sm)
        m = re.fullmatch(r"fz_states_sm_kernel_u(\d+)r(\d+)b256_g[0-9a-f]{8}" if sm else r"fz_states_kernel_u(\d+)b256_g[0-9a-f]{8}", sym)
        assert m, sym
        U, R = int(m.group(1)), int(m.group(2)) if sm else 0
        assert sym.endswith(p.grad_kernel_symbol()[-10:]) and r["unroll"] == U and U in (1, 2, 4, 8) and U * p.n_in <= max(16, p.n_in)
        if sm:
            assert R % 4 == 0 and R % U == 0 and (R * p.n_in >= 32 or not p.n_in)
        assert r["scratch_bytes"] == 0 and r["vgpr_spills"] == 0, r
        # the stated LDS: four waves' patches of x alone; nothing for a kernel that fetches no x or has no state to store
        assert r["lds_bytes"] == (4 * 64 * (R * p.n_in + 4) * 4 if sm and p.n_in and p.n_state else 0), r
        assert r["vgprs"] + r["agprs"] <= 256
        src = p.states_source(sm)
        assert sym in src and "fz_adj::fwd" in src and f"#define FZ_U {U} " in src
        lines.append(f"{sym}: {r['vgprs']} VGPRs, {r['sgpr_spills']} SGPR spills, {r['lds_bytes']} B LDS")
    with capsys.disabled():                                       # (SGPR spills are reported, not asserted: correct, slower)
        print("\n" + "\n".join(lines))


def test_a_manifest_with_a_sound_and_impossible_states_variants_builds_one_and_refuses_the_rest(tmp_path):
    recipe = recipe_of(GG.SUPPORTED["integrator"]())
    p = F.compile(F.from_sexpr(GG.SUPPORTED["integrator"]()))
    u = symbol_shape(p.states_kernel_symbol(), "u")[0]
    usm, r, _ = symbol_shape(p.states_kernel_symbol(True), "u")
    path = tmp_path / "m.fzm"
    write_manifest(path, [(1, u, 256, ADJOINT | STATES, recipe),                              # sound
                          (1, 2 * u, 256, ADJOINT | STATES, recipe),                          # an unroll the host does not make for this graph
                          (2, u, 256, ADJOINT | STATES, recipe),                              # streams per lane: always 1
                          (1, u, 128, ADJOINT | STATES, recipe),                              # another workgroup
                          (2 * r, usm, 256, ADJOINT | STATES | ADJOINT_SM, recipe),           # another patch
                          (1, u, 256, ADJOINT | STATES | ADJOINT_LOSS, recipe),               # the loss bit next to it: no kernel of anything
                          (1, u, 256, ADJOINT | STATES | 256, recipe)])                       # a forward flag next to it
    res = replay(path, {"FLOWZ_HIP_CACHE": str(tmp_path / "cache")}, jobs=2)
    assert res["records"] == 7 and res["built"] == 1 and res["failed"] == 6 and res["at_hand"] == 0, res
    assert len(code_objects(tmp_path / "cache")) == 1
    # the states bit without the adjoint bit is no variant of anything: a caller's forward variant with it is refused as reserved
    with pytest.raises(F.FlowzError):
        p.build(F.make_variant(1, 8, 256, STATES))


def test_the_recorded_manifest_holds_the_kernels_of_the_gpu_tests():
    """tests/golden/recording_kernels.fzm.gz: states kernels in both layouts, the adjoint and loss kernels they are followed by, and the
    forward kernels the GPU test takes its states from; none refused"""
    flags = [int(m.group(1)) for m in re.finditer(rb"FZM1 \d+ \d+ \d+ (\d+) \d+\n", gzip.open(MANIFEST, "rb").read())]
    states = [f for f in flags if f & ADJOINT and f & STATES]
    assert states and any(f & ADJOINT_SM for f in states) and any(not f & ADJOINT_SM for f in states)
    assert any(f & ADJOINT and f & ADJOINT_LOSS for f in flags) and any(f & ADJOINT and not f & (STATES | ADJOINT_LOSS) for f in flags)
    r = F.manifest_build(MANIFEST)
    assert r["failed"] == 0 and r["at_hand"] + r["built"] == r["records"] == len(flags), r


# ---- the restatement: block by block in reverse is the single call, bit for bit -----------------------------------------------------
@pytest.mark.parametrize("name", ["df1_cascade_params6", "moog_ladder", "rules", "make11", "generator_without_input", "no_delay_line"])
def test_the_block_by_block_restatement_is_the_single_call_bitwise(name):
    p = prog_of(name)
    ns, T = 9, 37
    kw = dict(draw_params=GC.draw_params, ties=GC.has_ties(p), special_every=GC.SPECIAL_EVERY) if name in GC.CELLS else {}
    x, s0, par, yb, sb, ap, ac = make_inputs(p, name, ns, T, 41, **kw)
    al = np.random.default_rng(42).standard_normal(ns).astype(F32)
    one = A.grad(p, x, yb, s0, par, sb, ap, ac)
    y, s_T = A.forward(p, x, s0, par)
    one_loss = LR.loss_grad(p, x, yb, 0.37, s0, par, sb, ap, ac, al) if p.n_out else None
    for B in (4, 8, 12, T, 4 * T):
        got = RR.grad(p, x, B, out_grad=yb, state=s0, params=par, state_grad=sb, accum_params=ap, accum_consts=ac)
        for k in ("x", "state", "params", "consts"):
            assert same(got[k], one[k]), (name, B, k)
        assert same(got["state_out"], s_T) and same(got["starts"][0], s0)
        assert got["starts"].shape[0] == -(-T // min(B, T))
        for kb in range(1, got["starts"].shape[0]):               # the state before block kb is the forward's after kb * B rows
            assert same(got["starts"][kb], A.forward(p, x[:kb * min(B, T)], s0, par)[1]), (name, B, kb)
        if one_loss is not None:
            got = RR.grad(p, x, B, target=yb, k=0.37, state=s0, params=par, state_grad=sb, accum_params=ap, accum_consts=ac, accum_loss=al)
            for k in ("x", "state", "params", "consts", "loss", "out"):
                assert same(got[k], one_loss[k]), (name, B, k, "loss")
            assert same(got["out"], y)
