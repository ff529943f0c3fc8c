"""The backward of a block without a GPU: the support matrix, the workspace size, argument checks, the adjoint kernel's resources and
instructions (JIT for gfx950), and tests/adjoint_ref.py -- the numpy statement of the documented order the GPU tests hold the kernel
to -- against float64 autograd and central finite differences."""
import ctypes
import glob
import os
import re
import subprocess

import numpy as np
import pytest

import adjoint_ref as A
import grad_graphs as GG
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
        cd = int(p.grad_kernel_symbol().split("_c")[1].split("b")[0])
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
class FakeBufs:
    """distinct, 16-byte aligned, never dereferenced addresses for every buffer of a call"""

    def __init__(self, p, ns, T):
        self.p, self.ns, self.T = p, ns, T
        self.ws = p.grad_workspace_bytes(ns, T)
        base, off = 1 << 40, 0
        sizes = {"in_": T * ns * p.n_in * 4, "state": p.n_state * ns * 4, "params": p.n_param * ns * 4, "out_grad": T * ns * p.n_out * 4,
                 "state_grad": p.n_state * ns * 4, "in_grad": T * ns * p.n_in * 4, "state0_grad": p.n_state * ns * 4,
                 "param_grad": p.n_param * ns * 4, "const_grad": p.n_const * ns * 4, "workspace": self.ws}
        self.addr, self.size = {}, sizes
        for k, n in sizes.items():
            self.addr[k] = base + off
            off += (max(n, 16) + 4095) // 4096 * 4096

    def args(self, **over):
        a = C.GradArgs()
        a.struct_size = ctypes.sizeof(C.GradArgs)
        for k, v in self.addr.items():
            setattr(a, k, v if self.size[k] else None)
        a.workspace_bytes = self.ws
        for k, v in over.items():
            setattr(a, k, v)
        return a

    def run(self, a, ns=None, T=None):
        return C.lib.fz_run_block_grad(self.p._h, ctypes.byref(a), self.ns if ns is None else ns, self.T if T is None else T, None)


def test_argument_checks():
    p = prog_of("df1_cascade_params6")
    assert p.n_const == 0
    q = prog_of("moog_ladder")
    b = FakeBufs(p, 1000, 40)
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
    empty = C.GradArgs()
    empty.struct_size = ctypes.sizeof(C.GradArgs)
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
    assert r["unroll"] == int(p.grad_kernel_symbol().split("_c")[1].split("b")[0])
    if name in ("df1_cascade6", "moog_ladder"):
        for c in (1, 4):
            assert p.grad_resources(c)["scratch_bytes"] == 0


@pytest.mark.parametrize("name", ["df1_cascade6", "osc_chain6", "envelope_follower", "moog_ladder", "div_sqrt_exp", "rules"])
def test_adjoint_kernel_has_no_fma(name, tmp_path, monkeypatch):
    monkeypatch.setenv("FLOWZ_HIP_CACHE", str(tmp_path))
    p = prog_of(name)
    p.grad_resources()
    objs = glob.glob(str(tmp_path / "*.hsaco"))
    assert len(objs) == 1
    dis = subprocess.check_output(["/opt/rocm/lib/llvm/bin/llvm-objdump", "-d", objs[0]], text=True)
    assert p.grad_kernel_symbol() in dis
    ops = [ln.split()[0] for ln in dis.splitlines() if ln.strip().startswith("v_")]
    assert len(ops) > 20
    # no contraction: the only fused multiply-adds are the refinement steps of the correctly rounded float32 division (five:
    # v_div_scale, v_rcp, Newton steps, v_div_fmas, v_div_fixup) and square root (two after v_sqrt) -- tanh divides, so do DIV
    # and the SQRT adjoint; graphs without them hold none at all
    fused = [o for o in ops if o.startswith(("v_fma", "v_fmac"))]
    divisions, roots = ops.count("v_div_fixup_f32"), ops.count("v_sqrt_f32_e32") + ops.count("v_sqrt_f32_e64")
    assert len(fused) == 5 * divisions + 2 * roots and ops.count("v_div_fmas_f32") == divisions
    assert not [o for o in ops if re.match(r"v_(pk_(fma|mad|mac)|mad|mac)(_mix|_mixlo|_mixhi|_legacy)?_(f16|f32|f64|bf16)", o)]
    kinds = {k for k, *_ in p.ir()}
    if not kinds & {"div", "tanh", "sqrt"}:
        assert divisions == 0 and roots == 0 and not fused


def test_forward_kernel_sources_unchanged_by_the_adjoint():
    """the adjoint kernel has a text of its own: the forward kernels' sources do not mention it"""
    p = prog_of("df1_cascade6")
    src = p.source()
    assert "fz_adj" not in src and "fz_adjoint_kernel" not in src


# ---- the numpy restatement against float64 autograd and finite differences --------------------------------------------------------
def inputs(p, ns, T, seed, scale=0.5):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((T, ns, p.n_in)) * scale).astype(F32)
    s0 = (rng.standard_normal((p.n_state, ns)) * 0.1).astype(F32)
    par = None
    if p.n_param:
        par = (rng.uniform(-0.3, 0.3, (p.n_param, ns))).astype(F32)
    yb = rng.standard_normal((T, ns, p.n_out)).astype(F32)
    sb = rng.standard_normal((p.n_state, ns)).astype(F32)
    return x, s0, par, yb, sb


def params_for(name, p, ns, rng):
    """coefficients that keep the recursions stable"""
    if name == "moog_ladder":
        return rng.uniform(0.05, 0.5, (1, ns)).astype(F32)
    if name in ("df1_cascade_params6", "osc_chain6"):
        import graphs as G
        if name == "osc_chain6":
            return np.asarray(G.osc_chain_params(G.SEED, np.arange(ns)), F32)
        out = np.empty((p.n_param, ns), F32)
        for j in range(p.n_param // 5):
            out[5 * j:5 * j + 5] = np.asarray(G.STABLE, F32)[:, None] * rng.uniform(0.9, 1.0, (5, ns)).astype(F32)
        return out
    return None


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


def fd_check(p, x, s0, par, yb, sb, h=1e-6):
    """central differences of the float64 torch forward against the numpy restatement, a few coordinates of every tensor"""
    import torch

    L = A.Layout(p)
    ns = x.shape[1]
    c = np.repeat(L.consts.astype(np.float64)[:, None], ns, 1)
    base = dict(x=np.asarray(x, np.float64), state=np.asarray(s0, np.float64),
                params=np.zeros((L.n_param, ns)) if par is None else np.asarray(par, np.float64), consts=c)

    def loss(d):
        t = {k: torch.tensor(v, dtype=torch.float64) for k, v in d.items()}
        y, sT = A.torch_forward(L, t["x"], t["state"], t["params"], t["consts"])
        return float((y * torch.tensor(np.asarray(yb, np.float64))).sum() + (sT * torch.tensor(np.asarray(sb, np.float64))).sum())
    got = A.grad(p, x, yb, s0, par, sb)
    rng = np.random.default_rng(3)
    for k in ("x", "state", "params", "consts"):
        if base[k].size == 0:
            continue
        for _ in range(6):
            idx = tuple(rng.integers(0, n) for n in base[k].shape)
            d1 = {kk: vv.copy() for kk, vv in base.items()}
            d2 = {kk: vv.copy() for kk, vv in base.items()}
            d1[k][idx] += h
            d2[k][idx] -= h
            fd = (loss(d1) - loss(d2)) / (2 * h)
            g = float(got[k][idx])
            assert abs(g - fd) <= 2e-4 * max(1.0, abs(fd)), (k, idx, g, fd)


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
