"""The backward of a whole recording with deep delay lines without a GPU (fz_run_recording_ring_grad, fz_run_recording_ring_loss_grad):
the scope and the refusals that stay, the calls they ARE for a graph without a deep line, the block rule and the workspace formula
against their restatements, every argument check with its reason, the ring states kernel's JIT for gfx950 (a symbol of its own, no
scratch, no VGPR spills, the ring adjoint kernel's LDS, no FMA, no barrier, no atomic), the code pins' names for every other kernel, the kernel
manifest of the GPU tests, and tests/recording_ref.py on the ring graphs -- the block-by-block restatement the GPU test holds the calls
to -- against the single restated call, bit for bit, with inputs that tell a wrong chain from the right one."""
import ctypes
import os
import re

import numpy as np
import pytest

import adjoint_ref as A
import grad_graphs as GG
import loss_grad_ref as LR
import recording_ref as RR
import ring_grad_graphs as RG
import ring_recording_graphs as R
import ring_sm_recording as S
from grad_harness import same
from grad_host_harness import (ADJOINT, ADJOINT_LOSS, ADJOINT_RING, ADJOINT_SM, LDS_BYTES, STATES, FakeCall, assert_no_contraction, code_objects, code_pins,
                               empty_args, invalid, kernel_ops, recipe_of, replay, symbol_shape, write_manifest)
from zignal_amd import _capi as C
from zignal_amd import flowz as F

F32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
RING_STATES_BITS = ADJOINT | STATES | ADJOINT_RING
NEW_EXPORTS = ("fz_program_ring_recording_block_rows", "fz_program_ring_recording_workspace", "fz_run_recording_ring_grad",
               "fz_run_recording_ring_loss_grad", "fz_program_ring_states_resources", "fz_program_ring_states_kernel_symbol",
               "fz_program_ring_states_source")
NAMES = sorted(R.GRAPHS)


def run_fn(loss):
    return C.lib.fz_run_recording_ring_loss_grad if loss else C.lib.fz_run_recording_ring_grad


def test_the_new_entry_points_are_declared_and_exported():
    header = open(os.path.join(HERE, "..", "include", "flowz_hip.h")).read()
    for name in NEW_EXPORTS:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in C.EXPORTS and getattr(C.lib, name)
    for name in ("ring_recording_block_rows", "ring_recording_workspace_bytes", "ring_states_resources", "ring_states_kernel_symbol",
                 "ring_states_source", "run_recording_ring_grad", "run_recording_ring_loss_grad"):
        assert callable(getattr(F.Program, name)), name
    from zignal_amd import autograd as AG
    assert callable(AG.mse_recording_rings)


# ---- scope ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_the_ten_graphs_are_taken(name):
    p = R.prog(name)
    sym = p.ring_states_kernel_symbol()
    m = re.fullmatch(r"fz_states_ring_kernel_u(1|2|4|8)b(256|128|64)_g([0-9a-f]{8})", sym)
    assert m, sym
    ring = re.fullmatch(r"fz_adjoint_ring_kernel_c\d+b(\d+)_g([0-9a-f]{8})", p.ring_grad_kernel_symbol())
    assert (m.group(2), m.group(3)) == (ring.group(1), ring.group(2))     # the ring adjoint kernel's lanes and graph tag
    src = p.ring_states_source()
    text = S.compiled_text(src)                                   # (the ring side of the one time-major states text)
    assert sym in src and "#define FZ_RING 1 " in src and "fz_states_args" in text and f"#define FZ_U {m.group(1)} " in src
    assert "fz_adj::fwd(xa[j], c, p, st, rv, sn, u)" in text and "fz_adj::fwd(xa[j], c, p, st, sn)" not in text
    assert "fz_dump_state(sk, ns, st, ring, pos)" in text and "__shared__ float fz_ring[FZ_RING_SLOTS * FZ_BLOCK];" in text
    assert "__syncthreads" not in src and "atomic" not in src.split("// ==== fz_block_kernel.hip.inc ====")[1].split("#include")[1]
    for loss in (False, True):
        for ns, T in ((0, 100), (100, 0), (0, 0)):                # an empty recording is FZ_OK with nothing touched
            assert run_fn(loss)(p._h, ctypes.byref(empty_args(loss)), ns, T, 0, None, None) == C.FZ_OK, C.last_error()
    assert p.ring_recording_block_rows(0) == 0 and p.ring_recording_workspace_bytes(100, 0) == 0 and p.ring_recording_workspace_bytes(0, 100) == 0


@pytest.mark.parametrize("name", sorted(n for n in GG.REFUSED if n != "lds_ring_comb"))
def test_refusals_keep_their_reasons(name):
    build, typed, word = GG.REFUSED[name]
    p = F.compile(F.from_sexpr(build()), typed=typed)
    assert C.lib.fz_program_ring_grad_check(p._h) == C.FZ_E_UNSUPPORTED
    why = C.last_error()
    assert word.lower() in why.lower()
    for loss in (False, True):
        for ns, T in ((64, 16), (0, 0)):
            assert run_fn(loss)(p._h, ctypes.byref(empty_args(loss)), ns, T, 0, None, None) == C.FZ_E_UNSUPPORTED and C.last_error() == why
    for call in (p.ring_states_kernel_symbol, p.ring_states_source, p.ring_states_resources, lambda: p.ring_recording_block_rows(16),
                 lambda: p.ring_recording_workspace_bytes(64, 16)):
        with pytest.raises(F.FlowzError) as ei:
            call()
        assert ei.value.code == C.FZ_E_UNSUPPORTED and why in str(ei.value)


def test_rings_that_fit_no_workgroup_are_refused_with_the_bytes():
    p = F.compile(F.from_sexpr(RG.six_lines_256()))
    for loss in (False, True):
        for ns, T in ((64, 16), (0, 0)):
            assert run_fn(loss)(p._h, ctypes.byref(empty_args(loss)), ns, T, 0, None, None) == C.FZ_E_UNSUPPORTED
            why = C.last_error()
            assert "393216 bytes" in why and str(LDS_BYTES) in why and "LDS" in why, why
    for call in (p.ring_states_kernel_symbol, p.ring_states_source, p.ring_states_resources, lambda: p.ring_recording_block_rows(16),
                 lambda: p.ring_recording_workspace_bytes(64, 16)):
        with pytest.raises(F.FlowzError) as ei:
            call()
        assert ei.value.code == C.FZ_E_UNSUPPORTED and "393216" in str(ei.value)
    from zignal_amd import autograd as AG
    with pytest.raises(F.FlowzError) as ei:
        AG.mse_recording_rings(p, None, None)
    assert ei.value.code == C.FZ_E_UNSUPPORTED and "393216" in str(ei.value)


def test_the_recording_calls_without_rings_still_refuse_the_ring_comb():
    p = R.prog("lds_ring_comb")
    g, a = empty_args(False), empty_args(True)
    for layout in (0, 1):
        assert C.lib.fz_run_recording_grad(p._h, ctypes.byref(g), layout, 64, 16 * layout, 0, 16, 0, None, None) == C.FZ_E_UNSUPPORTED and "LDS" in C.last_error()
        assert C.lib.fz_run_recording_loss_grad(p._h, ctypes.byref(a), layout, 64, 16 * layout, 0, 16, 0, None, None) == C.FZ_E_UNSUPPORTED and "LDS" in C.last_error()
        for call in (p.states_kernel_symbol, p.states_resources, p.states_source, lambda sm: p.recording_workspace_bytes(64, 16, stream_major=sm)):
            with pytest.raises(F.FlowzError) as ei:
                call(bool(layout))
            assert ei.value.code == C.FZ_E_UNSUPPORTED and "LDS" in str(ei.value)
    with pytest.raises(F.FlowzError) as ei:
        p.recording_block_rows(16)
    assert ei.value.code == C.FZ_E_UNSUPPORTED and "LDS" in str(ei.value)
    from zignal_amd import autograd as AG
    with pytest.raises(F.FlowzError) as ei:
        AG.mse_recording(p, None, None)
    assert ei.value.code == C.FZ_E_UNSUPPORTED and "LDS" in str(ei.value)


def test_a_forward_variant_naming_states_and_ring_is_refused_as_reserved():
    p = R.prog("fb9")
    for flags in (STATES | ADJOINT_RING, RING_STATES_BITS):
        with pytest.raises(F.FlowzError) as ei:
            p.kernel_name(F.make_variant(1, 8, 256, flags), 4096, 64)
        assert ei.value.code == C.FZ_E_INVALID and "reserved" in str(ei.value)
        with pytest.raises(F.FlowzError):
            p.build(F.make_variant(1, 8, 256, flags))


# ---- a graph without a deep line: the calls ARE the time-major recording calls ---------------------------------------------------------
GRID_T = (1, 3, 4, 7, 37, 64, 100, 1000, 1024, 4096, 48000, (1 << 31) - 1)
GRID_B = (0, 4, 8, 12, 40, 64, 4096)


@pytest.mark.parametrize("name", sorted(GG.SUPPORTED))
def test_for_a_graph_without_a_ring_the_calls_are_the_recording_calls(name):
    p = F.compile(F.from_sexpr(GG.SUPPORTED[name]()))
    assert p.ring_states_kernel_symbol() == p.states_kernel_symbol(False)
    assert p.ring_states_source() == p.states_source(False)
    for c in (0, 1, 8):
        for T in GRID_T:
            for B in GRID_B:
                assert p.ring_recording_block_rows(T, B, c) == p.recording_block_rows(T, B, c), (c, T, B)
                assert p.ring_recording_workspace_bytes(1000, T, B, c) == p.recording_workspace_bytes(1000, T, B, c), (c, T, B)


# ---- the block rule and the workspace formula ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_the_counts_of_each_graph_are_what_the_ring_workspace_says(name):
    """n_register_state and n_ring_lines from fz_program_ring_grad_workspace at T = 1 (one checkpoint, one tape row) and T = C (one
    checkpoint, C tape rows); and from the lines themselves"""
    p = R.prog(name)
    n_reg, n_rl = R.COUNTS[name]
    Cc = R.stride(p)
    assert Cc > 1 and p.ring_grad_workspace_bytes(7, 1) == (n_reg + n_rl) * 7 * 4 and p.ring_grad_workspace_bytes(7, Cc) == (n_reg + Cc * n_rl) * 7 * 4
    depths = [d for _, d in p.lines()]
    assert n_reg == sum(d for d in depths if d <= 8) and n_rl == len([d for d in depths if d > 8]) and p.n_state == sum(depths)
    assert max(depths) == R.DEEPEST[name] and [d for _, d in R.ring_rows(p)] == [d for d in depths if d > 8]


@pytest.mark.parametrize("name", NAMES)
def test_both_rules_are_their_restatements(name):
    p = R.prog(name)
    n_reg, n_rl = R.COUNTS[name]
    for c in (0, 1, 4):
        Cc = c or R.stride(p)
        for T in GRID_T:
            for B in GRID_B:
                Be = R.block_rows(T, Cc, p.n_state, n_reg, n_rl, B)
                assert p.ring_recording_block_rows(T, B, c) == Be, (c, T, B)
                rec = p.ring_recording_workspace_bytes(1000, T, B, c)
                assert rec == R.workspace_bytes(1000, T, Be, Cc, p.n_state, n_reg, n_rl), (c, T, B)
                # ... which is the block starts in front of the one-launch workspace of a block
                assert rec == -(-T // Be) * p.n_state * 1000 * 4 + p.ring_grad_workspace_bytes(1000, Be, c)
                # smaller than the one-launch workspace wherever the formulas say so
                one, one_rows = p.ring_grad_workspace_bytes(1000, T, c), -(-T // Cc) * n_reg + T * n_rl
                assert one == one_rows * 1000 * 4 and (rec < one) == (R.rows_kept(T, Be, Cc, p.n_state, n_reg, n_rl) < one_rows)
            assert p.ring_recording_block_rows(T, 4 * (T // 4) + 4, c) == T      # (a block_rows beyond T: one block)
            if T >= 8:                                            # the default B is a multiple of max(4, C) below T, or T
                B0 = p.ring_recording_block_rows(T, 0, c)
                assert B0 == T or (B0 < T and B0 % max(4, Cc) == 0)


def test_the_stated_figures():
    """derived by hand from the formulas (lds_ring_comb: n_state 63, two ring lines, no register rows, C 16; tap256: n_state 256, one ring
    line, C 16): B^2 * 32 >= 4096 * 63 * 16 gives 360, rounded to 368; 12 blocks; 12 * 63 + 368 * 2 = 1492 rows per stream"""
    p = R.prog("lds_ring_comb")
    assert R.stride(p) == 16 and p.n_state == 63
    for T, B, nb, rows, one in ((4096, 368, 12, 1492, 8192), (1024, 192, 6, 762, 2048)):
        assert p.ring_recording_block_rows(T) == B and -(-T // B) == nb
        assert p.ring_recording_workspace_bytes(1, T) == rows * 4 and p.ring_grad_workspace_bytes(1, T) == one * 4
    t = R.prog("tap256")
    assert t.ring_recording_block_rows(16384) == 2048 and t.ring_recording_workspace_bytes(1, 16384) == 4096 * 4 and t.ring_grad_workspace_bytes(1, 16384) == 16384 * 4
    # 1 048 576 streams x 4096 rows of the comb: 32 GiB in one launch
    assert p.ring_grad_workspace_bytes(1 << 20, 4096) == 32 << 30 and p.ring_recording_workspace_bytes(1 << 20, 4096) == 1492 * 4 << 20
    for name in NAMES:                                            # from 4096 rows on the recording is the smaller one for every graph
        q = R.prog(name)
        for T in (4096, 16384, 1 << 20):
            assert q.ring_recording_workspace_bytes(1000, T) < q.ring_grad_workspace_bytes(1000, T), (name, T)


# ---- argument checks: every one fails before the device is needed --------------------------------------------------------------------
@pytest.mark.parametrize("loss", [False, True])
@pytest.mark.parametrize("name", ["biquad_comb17", "two_out_fb"])
def test_argument_checks_fail_one_by_one_with_their_reason(name, loss):
    p = R.prog(name)                                              # inputs, outputs, a deep line, a per-stream coefficient
    assert p.n_in and p.n_out and p.n_param
    b = FakeCall(p, 1000, 37, ring=True, loss=loss, recording=8)
    assert b.ws == (5 * p.n_state) * 4000 + p.ring_grad_workspace_bytes(1000, 8)
    ybar = "target" if loss else "out_grad"
    a0 = b.args()
    size = ctypes.sizeof(a0)
    for bad in (size - 8, size + 8, 0, ctypes.sizeof(C.GradArgs if loss else C.LossGradArgs)):
        assert invalid(b.run(b.args(struct_size=bad)), "struct_size")
    assert invalid(b.run(b.args(checkpoint_rows=3)), "checkpoint_rows") and invalid(b.run(b.args(checkpoint_rows=64)), "checkpoint_rows")
    assert invalid(b.run(b.args(**{ybar: None})), ybar)
    assert invalid(b.run(b.args(in_=None)), "in is null") and invalid(b.run(b.args(state=None)), "state") and invalid(b.run(b.args(params=None)), "params")
    assert invalid(b.run(b.args(workspace=None)), "fz_program_ring_recording_workspace")
    assert invalid(b.run(b.args(workspace_bytes=b.ws - 4)), "fz_program_ring_recording_workspace")
    # (a workspace that would do for the one launch over the T rows is short for blocks of 4)
    assert p.ring_grad_workspace_bytes(1000, 37) < p.ring_recording_workspace_bytes(1000, 37, 4)
    assert invalid(b.run(b.args(workspace_bytes=p.ring_grad_workspace_bytes(1000, 37)), B=4), "fz_program_ring_recording_workspace")
    outs = ["in_grad", "workspace", "state0_grad", "param_grad"] + (["loss", "out"] if loss else [])
    for k in ["in_", ybar, "state", "params", "state_grad"] + outs:
        assert invalid(b.run(b.args(**{k: b.addr[k] + 4})), "aligned") and k.rstrip("_") in C.last_error(), k
    assert invalid(b.run(b.args(), state_out=b.addr["state_out"] + 4), "state_out")
    pairs = [("in_grad", ybar), ("state0_grad", ybar), ("in_grad", "in_"), ("param_grad", "workspace"), ("state0_grad", "state"), ("workspace", "in_")]
    pairs += [("loss", "target"), ("out", "in_"), ("out", "in_grad"), ("out", "target"), ("workspace", "out")] if loss else []
    for k, other in pairs:
        assert invalid(b.run(b.args(**{k: b.addr[other]})), "overlap"), (k, other)
        assert k in C.last_error() and other.rstrip("_") in C.last_error()
    assert invalid(b.run(b.args(state0_grad=b.addr["state_grad"] + 16)), "overlap")      # (only the exact alias of state_grad is allowed)
    for other in ("state", "in_", "workspace", "state0_grad", "param_grad"):             # state_out is an output: it overlaps nothing
        assert invalid(b.run(b.args(), state_out=b.addr[other]), "overlap") and "state_out" in C.last_error(), other
    # (the tail of the whole workspace counts, not only the block launches' share of it)
    assert invalid(b.run(b.args(), state_out=b.addr["workspace"] + b.ws - 16), "overlap")
    assert invalid(b.run(b.args(state0_grad=None)), "state0_grad")      # more than one block: they chain through it
    fn = run_fn(loss)
    assert fn(p._h, None, 10, 10, 0, None, None) == C.FZ_E_INVALID and "null arguments" in C.last_error()
    assert fn(None, ctypes.byref(a0), 10, 10, 0, None, None) == C.FZ_E_INVALID
    assert invalid(b.run(b.args(), T=1 << 31), "2^31")
    for B in (1, 2, 6, 37):
        assert invalid(b.run(b.args(), B=B), "multiple of 4") and "16-byte" in C.last_error()
    with pytest.raises(F.FlowzError, match="multiple of 4"):
        p.ring_recording_workspace_bytes(1000, 37, 6)
    with pytest.raises(F.FlowzError, match="2\\^31"):
        p.ring_recording_workspace_bytes(1000, 1 << 31)
    with pytest.raises(F.FlowzError, match="2\\^31"):
        p.ring_recording_block_rows(1 << 31)
    with pytest.raises(F.FlowzError, match="checkpoint_rows"):
        p.ring_recording_block_rows(100, 0, 3)
    # the order of run_recording: the scope, block_rows, the length, then the arguments
    assert invalid(b.run(b.args(in_=None), T=1 << 31, B=6), "multiple of 4") and invalid(b.run(b.args(in_=None), T=1 << 31), "2^31")
    big = FakeCall(p, 1, 1, ring=True, loss=loss, recording=0)
    assert big.run(big.args(), ns=1 << 30) == C.FZ_E_UNSUPPORTED and "2^30" in C.last_error()
    # an empty recording is FZ_OK and needs no buffer, but a bad struct_size is refused even then
    empty = empty_args(loss)
    for ns, T in ((0, 100), (100, 0), (0, 0)):
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


# ---- the ring states kernel for gfx950 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_ring_states_kernel_jit_compiles_without_scratch_with_the_ring_kernels_lds(name, capsys):
    p = R.prog(name)
    r, ring = p.ring_states_resources(), p.ring_grad_resources()
    sym = p.ring_states_kernel_symbol()
    U, block = symbol_shape(sym, "u")
    assert r["scratch_bytes"] == 0 and r["vgpr_spills"] == 0, r
    assert r["unroll"] == U and U in (1, 2, 4, 8) and U * p.n_in <= max(16, p.n_in)
    depths = [d for _, d in p.lines() if d > 8]
    assert r["lds_bytes"] == ring["lds_bytes"] == sum(depths) * block * 4 <= LDS_BYTES, (r, ring)
    # it holds two groups of frame registers (the group the recursion runs, the one requested for the next trip) next to the state
    assert 2 * U * p.n_in <= r["vgprs"] and r["vgprs"] + r["agprs"] <= 256
    with capsys.disabled():                                       # (SGPR spills are reported, not asserted: correct, slower)
        print(f"\n{sym}: {r['vgprs']} VGPRs ({ring['vgprs']} ring adjoint), {r['sgprs']} SGPRs, {r['sgpr_spills']} SGPR spills, {r['lds_bytes']} B LDS")


@pytest.mark.parametrize("name", NAMES)
def test_ring_states_kernel_has_no_fma_no_barrier_no_atomic(name, tmp_path, monkeypatch):
    """the method of test_ring_grad_host.py: test_ring_kernel_has_no_fma -- the only fused operations are those of the correctly rounded
    division (five each) and square root (two each) expansions"""
    _, _, _, every = kernel_ops(monkeypatch, tmp_path, R.GRAPHS[name](), "ring_states_resources", least=10)
    assert_no_contraction(every, divides=name == "ks_tanh11", lds=True)


# ---- every other kernel's code is the parent's: tests/golden/adjoint_code_pins.json, held by test_adjoint_code_pins_host.py ---------------
PINS = code_pins()


def test_the_pins_cover_every_graph():
    for kind in ("ring/tm/c0/", "ring/tm/c1/", "ring_loss/tm/c0/", "ring_loss/tm/c1/", "ring_states/tm/"):
        assert sorted(k[len(kind):] for k in PINS if k.startswith(kind)) == NAMES, kind
    assert sorted(k.split("/")[2] for k in PINS if k.startswith("states/tm/")) == sorted(GG.SUPPORTED)


def test_every_other_kernel_has_the_parents_text():
    """the pins name the kernels the library makes, and the ring states kernel's instructions are none of the ring adjoint kernels' (that
    all of them are the parent's code: test_adjoint_code_pins_host.py)"""
    pinned = {PINS[f"{kind}/tm/c{c}/{name}"][".text"] for kind in ("ring", "ring_loss") for c in (0, 1) for name in NAMES}
    for name in NAMES:
        p = R.prog(name)
        assert PINS[f"ring_states/tm/{name}"]["symbol"] == p.ring_states_kernel_symbol() and PINS[f"ring_states/tm/{name}"][".text"] not in pinned
        for c in (0, 1):
            assert PINS[f"ring/tm/c{c}/{name}"]["symbol"] == p.ring_grad_kernel_symbol(c)
            assert PINS[f"ring_loss/tm/c{c}/{name}"]["symbol"] == p.ring_loss_grad_kernel_symbol(c)


# ---- the kernel manifest of the GPU tests ----------------------------------------------------------------------------------------------
def test_the_committed_manifest_holds_exactly_the_kernels_the_gpu_tests_launch():
    import ring_loss_graphs as RL
    recs = RL.manifest_variants(R.MANIFEST)
    progs = [R.prog(n) for n in NAMES]
    got = sorted(v[:4] for v in recs if v[3] == RING_STATES_BITS)
    assert got == sorted((1, *symbol_shape(p.ring_states_kernel_symbol(), "u"), RING_STATES_BITS) for p in progs)
    assert len({v[4] for v in recs if v[3] == RING_STATES_BITS}) == len(NAMES)               # one recipe per graph
    for bits, sym in ((ADJOINT | ADJOINT_RING, F.Program.ring_grad_kernel_symbol), (ADJOINT | ADJOINT_RING | ADJOINT_LOSS, F.Program.ring_loss_grad_kernel_symbol)):
        assert sorted(v[:4] for v in recs if v[3] == bits) == sorted((1, *symbol_shape(sym(p, c), "c"), bits) for p in progs for c in (0, 1))
    # nothing else but the forward kernels the state comparison launches
    others = [v for v in recs if not v[3] & ADJOINT]
    assert all(not (v[3] & (ADJOINT_LOSS | ADJOINT_RING | STATES)) for v in others) and len(recs) == len(set(recs)) == 5 * len(NAMES) + len(others) <= 70
    counts = replay(R.MANIFEST)
    assert counts["failed"] == 0 and counts["records"] == len(recs), counts


def test_a_manifest_cannot_ask_for_a_ring_states_kernel_the_recording_would_not_make(tmp_path):
    """a wrong block, a wrong U, streams per lane, bits next to the three, a graph without a ring line, a graph the check refuses: counted
    as failed, nothing built"""
    import ring_loss_graphs as RL
    U, block, ring_recipe = next((v[1], v[2], v[4]) for v in RL.manifest_variants(R.MANIFEST) if v[3] == RING_STATES_BITS)

    plain, refused = recipe_of(GG.SUPPORTED["integrator"]()), recipe_of(RG.six_lines_256())
    bad = [(1, U, 512, RING_STATES_BITS, ring_recipe), (1, U, block // 2 if block > 64 else 128, RING_STATES_BITS, ring_recipe),
           (1, 2 * U, block, RING_STATES_BITS, ring_recipe), (1, U // 2, block, RING_STATES_BITS, ring_recipe), (1, 0, block, RING_STATES_BITS, ring_recipe),
           (2, U, block, RING_STATES_BITS, ring_recipe), (1, U, block, RING_STATES_BITS | ADJOINT_LOSS, ring_recipe),
           (1, U, block, RING_STATES_BITS | ADJOINT_SM, ring_recipe), (1, U, block, RING_STATES_BITS | 256, ring_recipe),
           (1, U, 256, RING_STATES_BITS, plain), (1, 8, 64, RING_STATES_BITS, refused)]
    good = [(1, U, block, RING_STATES_BITS, ring_recipe)]
    write_manifest(tmp_path / "bad.fzm", bad + good)
    counts = replay(tmp_path / "bad.fzm", {"FLOWZ_HIP_CACHE": str(tmp_path / "cache")})
    assert counts["failed"] == len(bad) and counts["built"] == 1 and counts["at_hand"] == 0, counts
    assert len(code_objects(tmp_path / "cache")) == 1


# ---- the restatement: block by block in reverse is the single call, bit for bit --------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_the_block_by_block_restatement_is_the_single_call_bitwise(name):
    p = R.prog(name)
    D = R.DEEPEST[name]
    cases = [(t, 0) for t in R.triples(name)] + [(R.below_depth(name), 1)]
    assert max(T for (_, T, _), _ in cases) == 2 * D + 3 and {ns for (ns, _, _), _ in cases} == {1, 64, 65, 257}
    for (ns, T, B), c in cases:
        d = R.case(name, ns, T)
        x, s0, par = d[0], d[1], d[2]
        Be = R.block_rows(T, c or R.stride(p), p.n_state, *R.COUNTS[name], B)
        assert Be == p.ring_recording_block_rows(T, B, c) and (B == 0 or Be == min(B, T))
        _, s_T = A.forward(p, x, s0, par)
        for loss in (False, True):
            one, got = R.single(p, d, loss), R.want(name, ns, T, B, loss, c)
            for k in ("x", "state", "params", "consts") + (("loss", "out") if loss else ()):
                assert same(got[k], one[k]), (name, ns, T, B, k, loss)
            assert same(got["state_out"], s_T) and same(got["starts"][0], s0) and got["starts"].shape == (-(-T // Be), p.n_state, ns)
        st = R.want(name, ns, T, B, True, c)["starts"]
        for kb in (1, st.shape[0] - 1):                           # the state before block kb is the forward's after kb * B rows
            if 0 < kb < st.shape[0]:
                assert same(st[kb], A.forward(p, x[:kb * Be], s0, par)[1]), (name, ns, T, B, kb)


def wrong_chain(p, d, B, kind):
    """the loss backward block by block with one mistake: `caller_state_grad` hands every block the caller's state_grad; `rotated` hands
    the blocks behind the first the rows of every deep line rotated by one (a ring read out one slot off)"""
    x, s0, par, _, tg, sb, ap, ac, al = d
    T = x.shape[0]
    st, _ = RR.starts(p, x, B, s0, par, A)
    if kind == "rotated":
        st = st.copy()
        for r0, D in R.ring_rows(p):
            st[1:, r0:r0 + D] = np.roll(st[1:, r0:r0 + D], 1, axis=1)
    g, gx, ys, r = sb, [None] * len(st), [None] * len(st), None
    for kb in range(len(st) - 1, -1, -1):
        rows = slice(kb * B, min((kb + 1) * B, T))
        r = LR.loss_grad(p, x[rows], tg[rows], R.K, st[kb], par, sb if kind == "caller_state_grad" else g, ap, ac, al, ref=A)
        gx[kb], ys[kb], g, ap, ac, al = r["x"], r["out"], r["state"], r["params"], r["consts"], r["loss"]
    return dict(r, x=np.concatenate(gx), out=np.concatenate(ys))


@pytest.mark.parametrize("name", NAMES)
def test_the_inputs_tell_a_wrong_chain(name):
    p = R.prog(name)
    ns, T, B = 65, R.DEEPEST[name] + 5, 4
    d, right = R.case(name, ns, T), R.want(name, ns, T, B, True)
    for kind in ("caller_state_grad", "rotated"):
        wrong = wrong_chain(p, d, B, kind)
        differs = np.zeros(ns, bool)
        for k in ("x", "state", "params", "consts", "loss", "out"):
            a, b = np.asarray(wrong[k], F32), np.asarray(right[k], F32)
            if a.size:
                ne = a.view(np.uint32) != b.view(np.uint32)
                differs |= ne if a.ndim == 1 else ne.any(axis=0) if a.ndim == 2 else ne.any(axis=(0, 2))
        assert differs.all(), (name, kind, int((~differs).sum()))
