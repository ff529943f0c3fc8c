"""The far recording calls without a GPU (fz_run_recording_far_grad, fz_run_recording_far_loss_grad: the backward of a whole recording
whose graph has delay lines deeper than 256 samples): their scope and the refusals every other call keeps; the far-free identity; the
rule for the rows per block and the workspace formula against their restatements and the stated figures; every argument check; the far
states kernel's resources, instructions and prefetch table (JIT for gfx950); the kernel manifest of the GPU tests; the code pins; and
tests/far_recording_ref.py -- the chaining identity the driver rests on, and that it tells a wrong chain."""
import ctypes
import re

import numpy as np
import pytest

import far_grad_graphs as FG
import far_grad_ref as FR
import far_recording_graphs as FRG
import far_recording_ref as RR
import grad_graphs as GG
import ring_grad_graphs as RG
import ring_loss_graphs as RL
from grad_harness import same
from grad_host_harness import (ADJOINT, ADJOINT_LOSS, ADJOINT_RING, ADJOINT_SM, LDS_BYTES, STATES, FakeCall, assert_no_contraction, code_objects, empty_args,
                               invalid, kernel_ops, recipe_of, replay, symbol_shape, write_manifest)
from zignal_amd import _capi as C
from zignal_amd import flowz as F

F32 = np.float32
ADJOINT_FAR = 1                                                    # fz_internal.hpp: FZ_VF_ADJOINT_FAR
FAR_BITS = ADJOINT | ADJOINT_RING | ADJOINT_FAR
FAR_STATES_BITS = FAR_BITS | STATES
NAMES = sorted(FRG.FARS)
K = 0.37

prog = FRG.prog


def stride(p, c=0):
    return c or symbol_shape(p.far_grad_kernel_symbol(), "c")[0]


def run_fn(loss):
    return C.lib.fz_run_recording_far_loss_grad if loss else C.lib.fz_run_recording_far_grad


class AsRing:
    """a program whose ring workspace queries are the far ones: what FakeCall(ring=True) asks of it"""
    MAP = {"ring_grad_workspace_bytes": "far_grad_workspace_bytes", "ring_recording_workspace_bytes": "far_recording_workspace_bytes"}

    def __init__(self, p):
        self._p = p

    def __getattr__(self, k):
        return getattr(self._p, self.MAP.get(k, k))


def far_fake_call(p, ns, T, loss, B):
    b = FakeCall(AsRing(p), ns, T, ring=True, loss=loss, recording=B)
    b.fn = run_fn(loss)
    return b


# ---- the surface ---------------------------------------------------------------------------------------------------------------------------
def test_the_new_entry_points_are_declared_and_exported():
    header = open(F.__file__.replace("zignal_amd/flowz.py", "include/flowz_hip.h")).read()
    for fn in ("fz_run_recording_far_grad", "fz_run_recording_far_loss_grad", "fz_program_far_recording_block_rows", "fz_program_far_recording_workspace",
               "fz_program_far_states_resources", "fz_program_far_states_kernel_symbol", "fz_program_far_states_source"):
        assert re.search(r"\b(int|long) %s\(" % fn, header), fn
        assert getattr(C.lib, fn)
    from zignal_amd import autograd as AG
    assert callable(AG.mse_recording_far)


# ---- scope ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_the_eight_graphs_are_taken_and_every_other_recording_call_keeps_refusing_them(name):
    p = prog(name)
    sym = p.far_states_kernel_symbol()
    assert re.fullmatch(r"fz_states_far_kernel_u(1|2|4|8)b(256|128|64)_g[0-9a-f]{8}", sym), sym
    assert sym.split("_g")[1] == p.kernel_symbol().split("_g")[-1]
    assert symbol_shape(sym, "u")[1] == symbol_shape(p.far_grad_kernel_symbol(), "c")[1]      # the far adjoint kernel's workgroup
    assert p.far_recording_block_rows(1000) and p.far_recording_workspace_bytes(64, 1000)
    g, a = empty_args(False), empty_args(True)
    hbm = lambda rc: rc == C.FZ_E_UNSUPPORTED and "HBM" in C.last_error()     # noqa: E731
    assert hbm(C.lib.fz_run_recording_ring_grad(p._h, ctypes.byref(g), 64, 16, 0, None, None))
    assert hbm(C.lib.fz_run_recording_ring_loss_grad(p._h, ctypes.byref(a), 64, 16, 0, None, None))
    assert hbm(C.lib.fz_run_recording_ring_grad_stream_major(p._h, ctypes.byref(g), 64, 16, 0, 16, 0, None, None))
    assert hbm(C.lib.fz_run_recording_ring_loss_grad_stream_major(p._h, ctypes.byref(a), 64, 16, 0, 16, 0, None, None))
    # (the plain calls name the first line deeper than 8 samples they meet: far_mixed's 17-sample ring stands in front of its far line)
    deep = lambda rc: rc == C.FZ_E_UNSUPPORTED and ("HBM" in C.last_error() or (name == "far_mixed" and "LDS" in C.last_error()))     # noqa: E731
    for layout in (0, 1):
        assert deep(C.lib.fz_run_recording_grad(p._h, ctypes.byref(g), layout, 64, 16 * layout, 0, 16, 0, None, None))
        assert deep(C.lib.fz_run_recording_loss_grad(p._h, ctypes.byref(a), layout, 64, 16 * layout, 0, 16, 0, None, None))
    ring_calls = [lambda: p.ring_recording_block_rows(16), lambda: p.ring_recording_workspace_bytes(64, 16), p.ring_states_resources, p.ring_states_kernel_symbol,
                  p.ring_states_source, lambda: p.ring_states_resources(True), lambda: p.ring_states_kernel_symbol(True)]
    plain_calls = [lambda: p.recording_block_rows(16), lambda: p.recording_workspace_bytes(64, 16), lambda: p.states_kernel_symbol(False),
                   lambda: p.states_resources(True)]
    from zignal_amd import autograd as AG
    for call in ring_calls + [lambda: AG.mse_recording_rings(p, None, None)]:
        with pytest.raises(F.FlowzError) as ei:
            call()
        assert ei.value.code == C.FZ_E_UNSUPPORTED and "HBM" in str(ei.value)
    for call in plain_calls + [lambda: AG.mse_recording(p, None, None)]:
        with pytest.raises(F.FlowzError) as ei:
            call()
        assert ei.value.code == C.FZ_E_UNSUPPORTED and ("HBM" in str(ei.value) or (name == "far_mixed" and "LDS" in str(ei.value)))


@pytest.mark.parametrize("name", sorted(n for n in GG.REFUSED if n not in ("lds_ring_comb", "far_comb")))
def test_refusals_keep_their_reasons(name):
    build, typed, word = GG.REFUSED[name]
    p = F.compile(F.from_sexpr(build()), typed=typed)
    assert C.lib.fz_program_far_grad_check(p._h) == C.FZ_E_UNSUPPORTED
    why = C.last_error()
    assert word.lower() in why.lower()
    for call in (lambda: p.far_recording_block_rows(16), lambda: p.far_recording_workspace_bytes(64, 16), p.far_states_resources, p.far_states_kernel_symbol,
                 p.far_states_source):
        with pytest.raises(F.FlowzError) as ei:
            call()
        assert ei.value.code == C.FZ_E_UNSUPPORTED and word.lower() in str(ei.value).lower()
    for loss in (False, True):
        a = empty_args(loss)
        assert run_fn(loss)(p._h, ctypes.byref(a), 64, 16, 0, None, None) == C.FZ_E_UNSUPPORTED and C.last_error() == why
        assert run_fn(loss)(p._h, ctypes.byref(a), 0, 0, 6, None, None) == C.FZ_E_UNSUPPORTED         # (the scope comes first)
    from zignal_amd import autograd as AG
    with pytest.raises(F.FlowzError) as ei:
        AG.mse_recording_far(p, None, None)
    assert ei.value.code == C.FZ_E_UNSUPPORTED


def test_rings_that_fit_no_workgroup_are_refused_with_the_bytes():
    p = F.compile(F.from_sexpr(RG.six_lines_256()))
    for call in (lambda: p.far_recording_block_rows(16), lambda: p.far_recording_workspace_bytes(64, 16), p.far_states_resources, p.far_states_kernel_symbol):
        with pytest.raises(F.FlowzError) as ei:
            call()
        assert ei.value.code == C.FZ_E_UNSUPPORTED and "393216" in str(ei.value) and str(LDS_BYTES) in str(ei.value)
    a = empty_args(False)
    assert run_fn(False)(p._h, ctypes.byref(a), 64, 16, 0, None, None) == C.FZ_E_UNSUPPORTED and "393216" in C.last_error()


def test_stream_major_buffers_stay_refused_for_far_lines():
    """there is no stream-major far recording call; the stream-major ring recording calls refuse the graphs (above), and a manifest
    cannot ask for a far states kernel with the stream-major bit (below).  The reason block_variant gives is the one-launch stream-major
    ring call's at a far graph's scope: the far scope is not that call's, so it says HBM"""
    p = prog("far_comb")
    assert not hasattr(C.lib, "fz_run_recording_far_grad_stream_major") and not hasattr(F.Program, "run_recording_far_grad_stream_major")
    g = empty_args(False)
    assert C.lib.fz_run_block_ring_grad_stream_major(p._h, ctypes.byref(g), 64, 16, 0, 16, None) == C.FZ_E_UNSUPPORTED and "HBM" in C.last_error()


def test_a_forward_variant_naming_the_far_states_bits_is_refused_as_reserved():
    p = prog("far_comb")
    for flags in (STATES | ADJOINT_RING | ADJOINT_FAR, FAR_STATES_BITS):
        with pytest.raises(F.FlowzError) as ei:
            p.kernel_name(F.make_variant(1, 8, 256, flags), 4096, 64)
        assert ei.value.code == C.FZ_E_INVALID and "reserved" in str(ei.value)


# ---- a graph without a far line: the calls ARE the time-major ring recording calls ----------------------------------------------------------
GRID_T = (1, 3, 4, 7, 37, 64, 100, 1000, 1024, 4096, 16384, 48000, (1 << 31) - 1)
GRID_B = (0, 4, 8, 12, 40, 64, 4096)


@pytest.mark.parametrize("name", sorted(RG.RINGS) + ["integrator", "df1_cascade6", "moog_ladder"])
def test_for_a_graph_without_a_far_line_the_calls_are_the_ring_recording_calls(name):
    p = F.compile(F.from_sexpr((RG.RINGS.get(name) or GG.SUPPORTED[name])()))
    assert p.far_states_kernel_symbol() == p.ring_states_kernel_symbol()
    assert p.far_states_source() == p.ring_states_source()
    for c in (0, 1, 8):
        for T in GRID_T:
            for B in GRID_B:
                assert p.far_recording_block_rows(T, B, c) == p.ring_recording_block_rows(T, B, c), (c, T, B)
                assert p.far_recording_workspace_bytes(1000, T, B, c) == p.ring_recording_workspace_bytes(1000, T, B, c), (c, T, B)


# ---- the block rule and the workspace formula -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_the_counts_of_each_graph_are_its_lines(name):
    p = prog(name)
    d = [depth for _, depth in p.lines()]
    n_reg, n_rl, n_fl, depths = FRG.COUNTS[name]
    assert (sum(x for x in d if x <= 8), sum(1 for x in d if 8 < x <= 256), sum(1 for x in d if x > 256), tuple(x for x in d if x > 256)) == (n_reg, n_rl, n_fl, depths)
    assert p.n_state == FRG.n_state(name) == sum(d) + n_fl and max(d) == FRG.DEEPEST[name]
    assert [(dd, pr) for _, dd, pr in FG.far_rows(p)] == [(dd, sum(d) + i) for i, dd in enumerate(depths)]


@pytest.mark.parametrize("name", NAMES)
def test_both_rules_are_their_restatements(name):
    p = prog(name)
    for c in (0, 1, 32):
        C_ = stride(p, c)
        for T in GRID_T:
            if T > 1 << 24 and c != 0:
                continue
            for B in GRID_B:
                Be = FRG.block_rows(name, T, C_, B)
                assert p.far_recording_block_rows(T, B, c) == Be, (c, T, B)
                assert Be % 4 == 0 or Be == T
                for ns in (1, 1000):
                    assert p.far_recording_workspace_bytes(ns, T, B, c) == FRG.workspace_bytes(name, ns, T, C_, B), (c, T, B, ns)
                # the formula by reference: the block-start states plus one block's far workspace
                assert p.far_recording_workspace_bytes(1000, T, B, c) == -(-T // Be) * p.n_state * 4000 + p.far_grad_workspace_bytes(1000, Be, c)
    assert p.far_recording_block_rows(0) == 0 and p.far_recording_workspace_bytes(1000, 0) == 0
    # B = 0 is the least multiple of max(4, C) at or beyond the continuous minimiser of the rows kept: one multiple less keeps more
    C_ = stride(p)
    for T in (4096, 16384, 48000):
        B = p.far_recording_block_rows(T)
        n_reg, n_rl, n_fl, _ = FRG.COUNTS[name]
        assert B < T and (B - max(4, C_)) ** 2 * (n_reg + C_ * (n_rl + n_fl)) < T * p.n_state * C_ <= B * B * (n_reg + C_ * (n_rl + n_fl))


def test_the_stated_figures():
    """far_comb (n_state 301, one far line, no register rows, C 16): T -> (B, blocks, rows kept per stream, one-launch rows)"""
    p = prog("far_comb")
    assert p.n_state == 301 and stride(p) == 16 and FRG.COUNTS["far_comb"] == (0, 0, 1, (300,))
    for T, (B, nb, kept, one) in {4096: (1120, 4, 2624, 4396), 16384: (2224, 8, 4932, 16684)}.items():
        assert p.far_recording_block_rows(T) == B and -(-T // B) == nb
        assert p.far_recording_workspace_bytes(1, T) == kept * 4 == FRG.rows_kept("far_comb", T, B, 16) * 4
        assert p.far_grad_workspace_bytes(1, T) == one * 4
    # 1 048 576 streams x 4096 rows: 10.25 GiB against 17.2 GiB
    assert p.far_recording_workspace_bytes(1 << 20, 4096) == 2624 * 4 << 20 and 2624 * 4 / 1024 == 10.25
    assert round(p.far_grad_workspace_bytes(1 << 20, 4096) / 2**30, 1) == 17.2
    # the saving grows with T
    ratios = [p.far_recording_workspace_bytes(1000, T) / p.far_grad_workspace_bytes(1000, T) for T in (4096, 16384, 1 << 20)]
    assert ratios[0] > ratios[1] > ratios[2]


# ---- argument checks: every one fails before the device is needed ---------------------------------------------------------------------------
@pytest.mark.parametrize("loss", [False, True])
@pytest.mark.parametrize("name", ["far_comb", "far_mixed"])
def test_argument_checks_fail_one_by_one_with_their_reason(name, loss):
    p = prog(name)
    b = far_fake_call(p, 1000, 700, loss, 64)
    assert b.ws == 11 * p.n_state * 4000 + p.far_grad_workspace_bytes(1000, 64)
    ybar = "target" if loss else "out_grad"
    a0 = b.args()
    size = ctypes.sizeof(a0)
    for bad in (size - 8, size + 8, 0, ctypes.sizeof(C.GradArgs if loss else C.LossGradArgs)):
        assert invalid(b.run(b.args(struct_size=bad)), "struct_size")
    assert invalid(b.run(b.args(checkpoint_rows=3)), "checkpoint_rows") and invalid(b.run(b.args(checkpoint_rows=64)), "checkpoint_rows")
    assert invalid(b.run(b.args(**{ybar: None})), ybar)
    assert invalid(b.run(b.args(in_=None)), "in is null") and invalid(b.run(b.args(state=None)), "state")
    if p.n_param:
        assert invalid(b.run(b.args(params=None)), "params")
    assert invalid(b.run(b.args(workspace=None)), "fz_program_far_recording_workspace")
    assert invalid(b.run(b.args(workspace_bytes=b.ws - 4)), "fz_program_far_recording_workspace")
    # (a workspace that does for blocks of 64 rows is short for blocks of 4: more block starts of n_state rows each)
    assert b.ws < p.far_recording_workspace_bytes(1000, 700, 4)
    assert invalid(b.run(b.args(), B=4), "fz_program_far_recording_workspace")
    outs = ["in_grad", "workspace", "state0_grad"] + (["param_grad"] if p.n_param else []) + (["loss", "out"] if loss else [])
    for k in ["in_", ybar, "state", "state_grad"] + (["params"] if p.n_param else []) + outs:
        assert invalid(b.run(b.args(**{k: b.addr[k] + 4})), "aligned") and k.rstrip("_") in C.last_error(), k
    assert invalid(b.run(b.args(), state_out=b.addr["state_out"] + 4), "state_out")
    pairs = [("in_grad", ybar), ("state0_grad", ybar), ("in_grad", "in_"), ("const_grad", "workspace"), ("state0_grad", "state"), ("workspace", "in_")]
    pairs += [("loss", "target"), ("out", "in_"), ("out", "in_grad"), ("out", "target"), ("workspace", "out")] if loss else []
    for k, other in pairs:
        assert invalid(b.run(b.args(**{k: b.addr[other]})), "overlap"), (k, other)
        assert k in C.last_error() and other.rstrip("_") in C.last_error()
    assert invalid(b.run(b.args(state0_grad=b.addr["state_grad"] + 16)), "overlap")      # (only the exact alias of state_grad is allowed)
    for other in ("state", "in_", "workspace", "state0_grad", "const_grad"):               # state_out is an output: it overlaps nothing
        assert invalid(b.run(b.args(), state_out=b.addr[other]), "overlap") and "state_out" in C.last_error(), other
    # (the tail of the whole workspace counts -- also the rows behind `starts` the far states kernel keeps its working rings in)
    assert invalid(b.run(b.args(), state_out=b.addr["workspace"] + b.ws - 16), "overlap")
    assert invalid(b.run(b.args(), state_out=b.addr["workspace"] + 11 * p.n_state * 4000), "overlap")
    assert invalid(b.run(b.args(state0_grad=None)), "state0_grad")      # more than one block: they chain through it
    fn = run_fn(loss)
    assert fn(p._h, None, 10, 10, 0, None, None) == C.FZ_E_INVALID and "null arguments" in C.last_error()
    assert fn(None, ctypes.byref(a0), 10, 10, 0, None, None) == C.FZ_E_INVALID
    assert invalid(b.run(b.args(), T=1 << 31), "2^31")
    for B in (1, 2, 6, 37):
        assert invalid(b.run(b.args(), B=B), "multiple of 4") and "16-byte" in C.last_error()
    with pytest.raises(F.FlowzError, match="multiple of 4"):
        p.far_recording_workspace_bytes(1000, 37, 6)
    with pytest.raises(F.FlowzError, match="2\\^31"):
        p.far_recording_workspace_bytes(1000, 1 << 31)
    with pytest.raises(F.FlowzError, match="2\\^31"):
        p.far_recording_block_rows(1 << 31)
    with pytest.raises(F.FlowzError, match="checkpoint_rows"):
        p.far_recording_block_rows(100, 0, 3)
    # the order of run_recording: the scope, block_rows, the length, then the arguments
    assert invalid(b.run(b.args(in_=None), T=1 << 31, B=6), "multiple of 4") and invalid(b.run(b.args(in_=None), T=1 << 31), "2^31")
    big = far_fake_call(p, 1, 1, loss, 0)
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
        assert b.run(b.args(), B=0) == C.FZ_E_NO_DEVICE and b.run(b.args(), B=400) == C.FZ_E_NO_DEVICE, C.last_error()
        assert b.run(b.args(workspace_bytes=2 * b.ws), B=32) == C.FZ_E_NO_DEVICE, C.last_error()      # (twice the block starts: under twice the bytes)
        optional = dict(in_grad=None, param_grad=None, const_grad=None, state_grad=None, **(dict(loss=None, out=None) if loss else {}))
        assert b.run(b.args(**optional), state_out=None) == C.FZ_E_NO_DEVICE, C.last_error()
        assert b.run(b.args(state0_grad=None, **optional), B=700, state_out=None) == C.FZ_E_NO_DEVICE, C.last_error()   # one block: no chain


# ---- the far states kernel for gfx950 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_far_states_kernel_jit_compiles_without_scratch_with_the_lds_of_the_ring_lines_alone(name, capsys):
    p = prog(name)
    r, far = p.far_states_resources(), p.far_grad_resources()
    sym = p.far_states_kernel_symbol()
    U, block = symbol_shape(sym, "u")
    assert r["scratch_bytes"] == 0 and r["vgpr_spills"] == 0, r
    assert r["unroll"] == U and U in (1, 2, 4, 8) and U * p.n_in <= max(16, p.n_in)
    lds_slots = sum(d for _, d in p.lines() if 8 < d <= 256)
    assert r["lds_bytes"] == far["lds_bytes"] == lds_slots * block * 4 <= LDS_BYTES, (r, far)
    assert block == [b for b in (256, 128, 64) if 2 * lds_slots * b * 4 <= LDS_BYTES][0]
    if name == "far_comb":
        assert r["lds_bytes"] == 0 and block == 256
    if name == "far_mixed":
        assert r["lds_bytes"] == 17 * 256 * 4
    assert r["vgprs"] + r["agprs"] <= 256
    with capsys.disabled():                                       # (SGPR spills are reported, not asserted: correct, slower)
        print(f"\n{sym}: {r['vgprs']} VGPRs ({far['vgprs']} far adjoint), {r['sgprs']} SGPRs, {r['sgpr_spills']} SGPR spills, {r['lds_bytes']} B LDS")


@pytest.mark.parametrize("name", NAMES)
def test_far_states_kernel_has_no_fma_no_barrier_no_atomic(name, tmp_path, monkeypatch):
    """the no-contraction rule of grad_host_harness; the far lines use no LDS, so only far_mixed touches it"""
    _, r, _, every = kernel_ops(monkeypatch, tmp_path, FRG.FARS[name](), "far_states_resources", least=10)
    assert_no_contraction(every, divides=name == "far_adjacent", lds=name == "far_mixed")
    if name != "far_mixed":
        assert not [o for o in every if o.startswith("ds_")] and r["lds_bytes"] == 0
    assert "s_barrier" not in every and not [o for o in every if "atomic" in o]
    assert "v_readfirstlane_b32" in every                           # the phase: one per wave and far line


def test_the_far_states_kernel_has_a_text_of_its_own():
    p = prog("far_mixed")
    src = p.far_states_source()
    cfg = src.split("// ==== fz_graph_body.h ====")[0]
    assert "fz_states_args" in src and "#define FZ_FAR 1 " in cfg and "#define FZ_RING 1 " in cfg and "#define FZ_FAR_SLOTS " in cfg
    assert "__syncthreads" not in src and "atomicAdd" not in src and "__shared__" in src and "FZ_FAR_FAST" not in cfg
    ring = RG.prog("biquad_comb17").ring_states_source().split("// ==== fz_graph_body.h ====")[0]
    assert "#define FZ_FAR 0 " in ring and "FZ_NFL" not in ring and "fz_fr_ahead" not in p.far_grad_source().split("// ==== fz_graph_body.h ====")[0]


def ahead(p):
    m = re.search(r"fz_fr_ahead\[\d+\] = \{([^}]*)\}", p.far_states_source())
    d = re.search(r"fz_fr_delay\[\d+\] = \{([^}]*)\}", p.far_states_source())
    return [int(x.strip().rstrip("u")) for x in d.group(1).split(",")], [int(x.strip().rstrip("u")) for x in m.group(1).split(",")]


def test_the_prefetch_table():
    """a far read at a delay of at least 2 U travels with the next group's x rows: far_tap1 at U = 8 has both kinds, 300 and 20 against 1"""
    assert ahead(prog("far_tap1")) == ([300, 1, 20], [1, 0, 1])
    assert symbol_shape(prog("far_tap1").far_states_kernel_symbol(), "u")[0] == 8
    for name in NAMES:
        U = symbol_shape(prog(name).far_states_kernel_symbol(), "u")[0]
        delays, table = ahead(prog(name))
        assert table == [int(d >= 2 * U) for d in delays], name


# ---- the kernel manifest of the GPU tests ---------------------------------------------------------------------------------------------------
def test_the_committed_manifest_holds_exactly_the_kernels_the_gpu_tests_launch():
    recs = RL.manifest_variants(FRG.MANIFEST)
    progs = [prog(n) for n in NAMES]
    assert sorted(v[:4] for v in recs if v[3] == FAR_STATES_BITS) == sorted((1, *symbol_shape(p.far_states_kernel_symbol(), "u"), FAR_STATES_BITS) for p in progs)
    assert len({v[4] for v in recs if v[3] == FAR_STATES_BITS}) == len(NAMES)                 # one recipe per graph
    for bits, sym in ((FAR_BITS, F.Program.far_grad_kernel_symbol), (FAR_BITS | ADJOINT_LOSS, F.Program.far_loss_grad_kernel_symbol)):
        assert sorted(v[:4] for v in recs if v[3] == bits) == sorted((1, *symbol_shape(sym(p, c), "c"), bits) for p in progs for c in (0, 1))
    # nothing else but the forward kernels the state comparison launches
    others = [v for v in recs if not v[3] & ADJOINT]
    assert all(not (v[3] & (ADJOINT_LOSS | ADJOINT_RING | STATES)) for v in others) and len(recs) == len(set(recs)) == 5 * len(NAMES) + len(others) <= 70
    counts = replay(FRG.MANIFEST)
    assert counts["failed"] == 0 and counts["records"] == len(recs), counts


def test_a_manifest_cannot_ask_for_a_far_states_kernel_the_recording_would_not_make(tmp_path):
    """a wrong block, a wrong U (16 among them: no maker answers it), streams per lane, the loss or the stream-major bit beside the four,
    the far bit without the ring bit, a graph without a far line, a graph the check refuses: counted as failed, nothing built"""
    U, block, far_recipe = next((v[1], v[2], v[4]) for v in RL.manifest_variants(FRG.MANIFEST) if v[3] == FAR_STATES_BITS)
    ring, refused = recipe_of(RG.RINGS["fb9"]()), recipe_of(RG.six_lines_256())
    bad = [(1, U, 512, FAR_STATES_BITS, far_recipe), (1, U, 128, FAR_STATES_BITS, far_recipe), (1, 16, block, FAR_STATES_BITS, far_recipe),
           (1, U // 2, block, FAR_STATES_BITS, far_recipe), (1, 0, block, FAR_STATES_BITS, far_recipe), (2, U, block, FAR_STATES_BITS, far_recipe),
           (1, U, block, FAR_STATES_BITS | ADJOINT_LOSS, far_recipe), (1, U, block, FAR_STATES_BITS | ADJOINT_SM, far_recipe),
           (1, U, block, FAR_STATES_BITS | 256, far_recipe), (1, U, block, ADJOINT | STATES | ADJOINT_FAR, far_recipe),
           (1, U, block, ADJOINT | STATES | ADJOINT_RING, far_recipe), (1, U, block, ADJOINT | STATES, far_recipe),
           (1, 8, 256, FAR_STATES_BITS, ring), (1, 8, 64, FAR_STATES_BITS, refused)]
    good = [(1, U, block, FAR_STATES_BITS, far_recipe)]
    assert (U, block) == (8, 256)
    write_manifest(tmp_path / "bad.fzm", bad + good)
    counts = replay(tmp_path / "bad.fzm", {"FLOWZ_HIP_CACHE": str(tmp_path / "cache")})
    assert counts["failed"] == len(bad) and counts["built"] == 1 and counts["at_hand"] == 0, counts
    assert len(code_objects(tmp_path / "cache")) == 1


# ---- every other kernel's code is the parent's -----------------------------------------------------------------------------------------------
def test_the_code_pins_still_hold():
    """tests/golden/adjoint_code_pins.json pins the machine code of every adjoint and states kernel that existed before the far states
    kernel: test_adjoint_code_pins_host.py, run here unmodified, in a process of its own"""
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider", os.path.join(here, "test_adjoint_code_pins_host.py")],
                       cwd=os.path.dirname(here), capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    assert re.search(r"\b\d+ passed", r.stdout) and "failed" not in r.stdout and "skipped" not in r.stdout


# ---- the restatement: block by block in reverse is the single call, bit for bit --------------------------------------------------------------
_one = {}


def one_call(name, ns, T, loss):
    """far_grad_ref's single call over the T rows of a shape's draw, computed once"""
    key = (name, ns, T, loss)
    if key not in _one:
        p = prog(name)
        d = FRG.inputs(name, ns, T, loss)
        x, s0, par, yt, sb, ap, ac = d[:7]
        _one[key] = (d, FR.loss_grad(p, x, yt, K, s0, par, sb, ap, ac, d[7]) if loss else FR.grad(p, x, yt, s0, par, sb, ap, ac))
    return _one[key]


@pytest.mark.parametrize("loss", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_the_block_by_block_restatement_is_the_single_call_bitwise(name, loss):
    p = prog(name)
    for ns, T, B, c in FRG.shapes(name):
        if c:
            continue                                               # (the restatement knows no checkpoint stride: B is given)
        Be = FRG.block_rows(name, T, stride(p), B)
        d, whole = one_call(name, ns, T, loss)
        x, s0, par, yt, sb, ap, ac = d[:7]
        if loss:
            got = RR.grad(p, x, Be, target=yt, k=K, state=s0, params=par, state_grad=sb, accum_params=ap, accum_consts=ac, accum_loss=d[7])
        else:
            got = RR.grad(p, x, Be, out_grad=yt, state=s0, params=par, state_grad=sb, accum_params=ap, accum_consts=ac)
        for k in whole:
            assert same(got[k], whole[k]), (name, ns, T, B, k)
        # the block starts are the forward's: slots, and phase rows advanced by B modulo the depths
        _, s_end = FR.forward(p, x, s0, par)
        assert same(got["state_out"], s_end) and same(got["starts"][0], s0)
        for _, dd, pr in FG.far_rows(p):
            assert [int(got["starts"][k][pr, 0]) for k in range(len(got["starts"]))] == [(FRG.p0_of(name) + k * Be) % dd for k in range(len(got["starts"]))]
            assert int(s_end[pr, 0]) == (FRG.p0_of(name) + T) % dd


@pytest.mark.parametrize("wrong", ["rotated", "stale_phase"])
@pytest.mark.parametrize("name", NAMES)
def test_the_inputs_tell_a_wrong_chain(name, wrong):
    """the far slots of the block starts rotated by one, or a phase row not advanced between blocks: dL/dx differs from the right answer
    in every stream.  Under the loss: most of the graphs are linear, and a linear graph's dL/dx for a GIVEN dL/dy does not depend on the
    values its lines hold -- the error the loss forms does"""
    p = prog(name)
    ns, T, B, _ = FRG.shapes(name)[2]                             # two blocks and a tail, the blocks shorter than the line
    d, whole = one_call(name, ns, T, True)
    x, s0, par, yt, sb, ap, ac = d[:7]
    got = RR.grad(p, x, B, target=yt, k=K, state=s0, params=par, state_grad=sb, accum_params=ap, accum_consts=ac, accum_loss=d[7], wrong=wrong)
    assert same(got["starts"], RR.starts(p, x, B, s0, par)[0])     # (the forward's; the chain used the spoilt ones)
    differs = (np.asarray(got["x"], F32).view(np.uint32) != np.asarray(whole["x"], F32).view(np.uint32)).any(axis=(0, 2))
    assert differs.shape == (ns,) and differs.all(), (name, wrong, int(differs.sum()))
