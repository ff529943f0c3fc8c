"""The backward of a block without a GPU: the support matrix, the workspace size, argument checks, the adjoint kernel's resources and
instructions (JIT for gfx950), and tests/adjoint_ref.py -- the numpy statement of the documented order the GPU tests hold the kernel
to -- against float64 autograd and central finite differences."""
import ctypes

import numpy as np
import pytest

import adjoint_ref as A
import grad_graphs as GG
from grad_host_harness import FakeCall, assert_no_contraction, empty_args, fd_check, inputs, kernel_ops, params_for, symbol_shape
from zignal_amd import _capi as C
from zignal_amd import flowz as F

F32 = np.float32


def prog_of(name):
    return F.compile(F.from_sexpr(GG.SUPPORTED[name]()))


@pytest.mark.parametrize("name", sorted(GG.SUPPORTED))
def test_supported_graphs_pass_the_check(name):
    p = prog_of(name)
    assert C.lib.fz_program_grad_check(p._h) == C.FZ_OK, C.last_error()
    assert p.grad_supported() and p.grad_unsupported_reason() == ""


@pytest.mark.parametrize("name", sorted(GG.REFUSED))
def test_refusals_name_their_reason(name):
    build, typed, word = GG.REFUSED[name]
    p = F.compile(F.from_sexpr(build()), typed=typed)
    assert C.lib.fz_program_grad_check(p._h) == C.FZ_E_UNSUPPORTED
    assert word.lower() in C.last_error().lower(), C.last_error()
    assert not p.grad_supported()
    with pytest.raises(F.FlowzError) as ei:
        p.grad_workspace_bytes(64, 16)
    assert ei.value.code == C.FZ_E_UNSUPPORTED
    with pytest.raises(F.FlowzError) as ei:
        p.grad_kernel_symbol()
    assert ei.value.code == C.FZ_E_UNSUPPORTED


@pytest.mark.parametrize("name", ["integrator", "df1_cascade6", "osc_chain6", "moog_ladder", "rules"])
def test_workspace_size_formula(name):
    p = prog_of(name)
    for ns, T in ((1, 1), (63, 7), (1000, 1000), (65537, 33)):
        for c in (1, 2, 4, 8, 16, 32):
            assert p.grad_workspace_bytes(ns, T, c) == -(-T // c) * p.n_state * ns * 4
        cd = symbol_shape(p.grad_kernel_symbol(), "c")[0]
        assert cd & (cd - 1) == 0 and 1 <= cd <= 16
        assert p.grad_workspace_bytes(ns, T) == p.grad_workspace_bytes(ns, T, cd)
    for bad in (3, 6, 64, 1 << 20):
        with pytest.raises(F.FlowzError) as ei:
            p.grad_workspace_bytes(64, 64, bad)
        assert ei.value.code == C.FZ_E_INVALID


def test_kernel_symbol_names_stride_block_and_graph():
    p = prog_of("df1_cascade6")
    s1, s4 = p.grad_kernel_symbol(1), p.grad_kernel_symbol(4)
    assert s1.startswith("fz_adjoint_kernel_c1b256_g") and s4.startswith("fz_adjoint_kernel_c4b256_g")
    assert s1.split("_g")[1] == s4.split("_g")[1] == p.kernel_symbol().split("_g")[-1]


# ---- argument checks: every one fails before the device is needed ----------------------------------------------------------------
def test_argument_checks():
    p = prog_of("df1_cascade_params6")
    assert p.n_const == 0
    q = prog_of("moog_ladder")
    b = FakeCall(p, 1000, 40)
    bad = [
        b.args(struct_size=ctypes.sizeof(C.GradArgs) - 8),
        b.args(struct_size=ctypes.sizeof(C.GradArgs) + 8),
        b.args(struct_size=0),
        b.args(checkpoint_rows=3),
        b.args(checkpoint_rows=64),
        b.args(in_=b.addr["in_"] + 4),                          # misaligned
        b.args(param_grad=b.addr["param_grad"] + 8),
        b.args(workspace=b.addr["workspace"] + 4),
        b.args(in_=None),                                        # NULL where a size needs data
        b.args(state=None),
        b.args(params=None),
        b.args(out_grad=None),
        b.args(workspace=None),
        b.args(workspace_bytes=b.ws - 4),                        # smaller than the query's answer
        b.args(in_grad=b.addr["in_"]),                           # outputs overlapping inputs / each other / the workspace
        b.args(in_grad=b.addr["out_grad"] + 16),
        b.args(state0_grad=b.addr["state"]),
        b.args(param_grad=b.addr["params"]),
        b.args(param_grad=b.addr["state0_grad"]),
        b.args(state0_grad=b.addr["state_grad"] + 16),           # (only the exact alias of state_grad is allowed)
        b.args(workspace=b.addr["in_grad"]),
        b.args(workspace=b.addr["out_grad"]),
    ]
    for i, a in enumerate(bad):
        assert b.run(a) == C.FZ_E_INVALID, (i, C.last_error())
    assert C.lib.fz_run_block_grad(p._h, None, 10, 10, None) == C.FZ_E_INVALID
    # the exact alias state0_grad == state_grad passes every check, and so do NULL outputs: without a device the call then stops at
    # FZ_E_NO_DEVICE.  (Where a GPU is present these fake addresses would be LAUNCHED on: not there -- test_grad_gpu.py runs the
    # alias and the NULL outputs on real buffers.)
    if C.lib.fz_device_count() == 0:
        assert b.run(b.args(state0_grad=b.addr["state_grad"])) == C.FZ_E_NO_DEVICE, C.last_error()
        assert b.run(b.args(in_grad=None, state0_grad=None, param_grad=None, const_grad=None, state_grad=None)) == C.FZ_E_NO_DEVICE
    # an empty block is FZ_OK and touches nothing: no buffer is needed at all
    empty = empty_args()
    for ns, T in ((0, 100), (100, 0), (0, 0)):
        assert C.lib.fz_run_block_grad(p._h, ctypes.byref(empty), ns, T, None) == C.FZ_OK, C.last_error()
        assert C.lib.fz_run_block_grad(q._h, ctypes.byref(empty), ns, T, None) == C.FZ_OK, C.last_error()
    # ... but a bad struct_size or an unsupported graph is refused even then
    empty.struct_size = 8
    assert C.lib.fz_run_block_grad(p._h, ctypes.byref(empty), 0, 0, None) == C.FZ_E_INVALID
    r = F.compile(F.from_sexpr(GG.REFUSED["far_comb"][0]()))
    empty.struct_size = ctypes.sizeof(C.GradArgs)
    assert C.lib.fz_run_block_grad(r._h, ctypes.byref(empty), 0, 0, None) == C.FZ_E_UNSUPPORTED


# ---- the adjoint kernel for gfx950 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(GG.SUPPORTED))
def test_adjoint_kernel_jit_compiles_without_scratch(name):
    p = prog_of(name)
    r = p.grad_resources()
    assert r["scratch_bytes"] == 0 and r["vgpr_spills"] == 0, r
    assert r["unroll"] == symbol_shape(p.grad_kernel_symbol(), "c")[0]
    if name in ("df1_cascade6", "moog_ladder"):
        for c in (1, 4):
            assert p.grad_resources(c)["scratch_bytes"] == 0


@pytest.mark.parametrize("name", ["df1_cascade6", "osc_chain6", "envelope_follower", "moog_ladder", "div_sqrt_exp", "rules"])
def test_adjoint_kernel_has_no_fma(name, tmp_path, monkeypatch):
    p, _, _, every = kernel_ops(monkeypatch, tmp_path, GG.SUPPORTED[name](), "grad_resources")
    assert_no_contraction(every, divides=bool({k for k, *_ in p.ir()} & {"div", "tanh", "sqrt"}))


def test_forward_kernel_sources_unchanged_by_the_adjoint():
    """the adjoint kernel has a text of its own: the forward kernels' sources do not mention it"""
    p = prog_of("df1_cascade6")
    src = p.source()
    assert "fz_adj" not in src and "fz_adjoint_kernel" not in src


# ---- the numpy restatement against float64 autograd and finite differences --------------------------------------------------------
@pytest.mark.parametrize("name", sorted(GG.SUPPORTED))
def test_reference_matches_float64_autograd(name):
    p = prog_of(name)
    ns, T = 8, 256 if name not in ("osc_chain6", "df1_cascade_params6", "df1_cascade6", "soft_clip_cascade") else 96
    rng = np.random.default_rng(7)
    x, s0, par, yb, sb = inputs(p, ns, T, 11)
    par = params_for(name, p, ns, rng) if p.n_param else None
    if name == "div_sqrt_exp":
        x = np.abs(x)
    got = A.grad(p, x, yb, s0, par, sb)
    want = A.torch_grad(p, x, yb, s0, par, sb)
    for k in ("x", "state", "params", "consts"):
        g = got[k][:want[k].shape[0]] if k != "x" else got[k]
        if np.asarray(want[k]).size == 0:
            continue
        e = A.rel_err(g, want[k])
        assert e <= 1e-4, (k, e)


@pytest.mark.parametrize("name", ["df1", "div_sqrt_exp", "moog_ladder"])
def test_reference_matches_central_differences(name):
    p = prog_of(name)
    ns, T = 3, 24
    x, s0, par, yb, sb = inputs(p, ns, T, 5)
    par = params_for(name, p, ns, np.random.default_rng(1)) if p.n_param else None
    if name == "div_sqrt_exp":
        x = np.abs(x)
    fd_check(p, x, s0, par, yb, sb)


def test_reference_follows_the_documented_rules():
    """MIN / MAX ties go to the operand std::min / std::max returned, ABS gives nothing at +-0, comparisons pass nothing on"""
    p = prog_of("rules")
    x = np.array([[[1.0, 1.0], [0.0, -0.0], [-0.0, 0.0], [0.0, 2.0], [-0.0, 2.0], [np.nan, 1.0], [0.75, np.inf], [-3.0, 1.0]]], F32)
    yb = np.ones((1, x.shape[1], 1), F32)
    g = A.grad(p, x, yb, None, None, None)["x"][0]
    # row 0, tie 1 == 1: max(a, b) returns a (a < b false), min(a, b) returns a (b < a false): all to _1; |1| -> +1 to _1
    assert g[0].tolist() == [1 + 0.75 + 1, 1.0]
    # +0 / -0 ties: min and max return a; abs at +-0 gives nothing
    assert g[1].tolist() == [1.75, 0.0] and g[2].tolist() == [1.75, 0.0]
    # an infinite value through a comparison: (_1 > 0.5) * _2 with _2 = inf -- its adjoint does not reach _1
    assert g[6].tolist() == [1.75, 2.0]
    # a NaN operand: max(NaN, 1) and min(NaN, 1) return NaN = a (every comparison with it is false), |NaN| gives nothing
    assert g[5, 0] == 1.75
