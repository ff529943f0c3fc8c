"""The backward under a squared-error loss without a GPU (fz_run_block_loss_grad, fz_run_block_loss_grad_stream_major): the refusals,
the argument checks, the two loss kernels' JIT for gfx950 (symbols of their own, no scratch, no VGPR spills, the plain kernel's LDS),
the plain adjoint kernels' text and symbol untouched by them, manifests, and tests/loss_grad_ref.py -- the numpy statement of the rule
the GPU tests hold the kernels to -- against float64 autograd of the mean squared error."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import adjoint_ref as A
import grad_graphs as GG
import loss_grad_ref as LR
from grad_host_harness import (ADJOINT, ADJOINT_LOSS, ADJOINT_SM, FakeCall, code_objects, empty_args, inputs, invalid, params_for, recipe_of, replay,
                               symbol_shape, write_manifest)
from zignal_amd import _capi as C
from zignal_amd import flowz as F

F32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
NEW_EXPORTS = ("fz_run_block_loss_grad", "fz_run_block_loss_grad_stream_major", "fz_program_loss_grad_resources_for",
               "fz_program_loss_grad_kernel_symbol_for", "fz_program_loss_grad_source_for")


def prog_of(name):
    return F.compile(F.from_sexpr(GG.SUPPORTED[name]()))


def test_the_new_entry_points_are_declared_and_exported():
    header = open(os.path.join(HERE, "..", "include", "flowz_hip.h")).read()
    for name in NEW_EXPORTS:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in C.EXPORTS and getattr(C.lib, name)
    assert "fz_loss_grad_args" in header


@pytest.mark.parametrize("name", sorted(GG.REFUSED))
def test_refusals_are_the_backwards(name):
    build, typed, word = GG.REFUSED[name]
    p = F.compile(F.from_sexpr(build()), typed=typed)
    g, a = empty_args(), empty_args(True)
    assert C.lib.fz_run_block_grad(p._h, ctypes.byref(g), 64, 16, None) == C.FZ_E_UNSUPPORTED
    why = C.last_error()
    assert word.lower() in why.lower()
    assert C.lib.fz_run_block_loss_grad(p._h, ctypes.byref(a), 64, 16, None) == C.FZ_E_UNSUPPORTED and C.last_error() == why
    assert C.lib.fz_run_block_loss_grad_stream_major(p._h, ctypes.byref(a), 64, 16, 0, 16, None) == C.FZ_E_UNSUPPORTED and C.last_error() == why
    for sm in (False, True):
        for call in (p.loss_grad_kernel_symbol, p.loss_grad_resources, p.loss_grad_source):
            with pytest.raises(F.FlowzError) as ei:
                call(stream_major=sm)
            assert ei.value.code == C.FZ_E_UNSUPPORTED and word.lower() in str(ei.value).lower()


# ---- argument checks: every one fails before the device is needed ----------------------------------------------------------------
@pytest.mark.parametrize("rows", [None, 48])
def test_argument_checks_fail_one_by_one_with_their_reason(rows):
    p = prog_of("moog_ladder")                                    # 1 in, 1 out, state, a parameter and coefficients
    assert p.n_in == 1 and p.n_out == 1 and p.n_state and p.n_param and p.n_const
    b = FakeCall(p, 1000, 40, loss=True, window=rows and (rows, 0))
    size = ctypes.sizeof(C.LossGradArgs)
    for bad in (size - 8, size + 8, 0, ctypes.sizeof(C.GradArgs)):
        assert invalid(b.run(b.args(struct_size=bad)), "struct_size")
    assert invalid(b.run(b.args(checkpoint_rows=3)), "checkpoint_rows")
    assert invalid(b.run(b.args(target=None)), "target")
    assert invalid(b.run(b.args(in_=None)), "in is null") and invalid(b.run(b.args(state=None)), "state") and invalid(b.run(b.args(params=None)), "params")
    assert invalid(b.run(b.args(workspace=None)), "workspace") and invalid(b.run(b.args(workspace_bytes=b.ws - 4)), "workspace")
    for k in ("in_", "target", "loss", "out", "in_grad", "workspace"):
        assert invalid(b.run(b.args(**{k: b.addr[k] + 4})), "aligned"), k
    # loss and out are outputs: they overlap nothing, the target included; inputs may still overlap each other
    for k, other in (("loss", "target"), ("loss", "in_"), ("loss", "param_grad"), ("loss", "workspace"), ("out", "target"), ("out", "in_"),
                     ("out", "in_grad"), ("out", "loss"), ("out", "state"), ("in_grad", "target"), ("state0_grad", "target")):
        assert invalid(b.run(b.args(**{k: b.addr[other]})), "overlap"), (k, other)
        assert k in C.last_error() and other.rstrip("_") in C.last_error()
    assert invalid(b.run(b.args(out=b.addr["target"] + b.size["target"] - 16)), "overlap")
    assert C.lib.fz_run_block_loss_grad(p._h, None, 10, 10, None) == C.FZ_E_INVALID and "null arguments" in C.last_error()
    assert C.lib.fz_run_block_loss_grad(None, ctypes.byref(b.args()), 10, 10, None) == C.FZ_E_INVALID
    if rows is not None:                                          # windows and alignment: fz_run_block_grad_stream_major's
        assert invalid(b.run(b.args(), rows=47), "rows_total") and invalid(b.run(b.args(), row0=2, T=8), "row0")
        assert invalid(b.run(b.args(), row0=12), "beyond rows_total")
    big = FakeCall(p, 1, 1, loss=True, window=rows and (rows, 0))
    assert big.run(big.args(), ns=1 << 30) == C.FZ_E_UNSUPPORTED and "2^30" in C.last_error()
    # what passes every check stops at the missing device (with one, fake addresses are not launched on): everything given, the exact
    # alias state0_grad == state_grad, every optional pointer NULL
    if C.lib.fz_device_count() == 0:
        assert b.run(b.args()) == C.FZ_E_NO_DEVICE, C.last_error()
        assert b.run(b.args(state0_grad=b.addr["state_grad"])) == C.FZ_E_NO_DEVICE, C.last_error()
        assert b.run(b.args(in_grad=None, state0_grad=None, param_grad=None, const_grad=None, state_grad=None, loss=None, out=None)) == C.FZ_E_NO_DEVICE


def test_an_empty_block_is_ok_and_needs_no_buffer():
    for name in ("df1_cascade_params6", "moog_ladder"):
        p = prog_of(name)
        empty = empty_args(True)
        for ns, T in ((0, 100), (100, 0), (0, 0)):
            assert C.lib.fz_run_block_loss_grad(p._h, ctypes.byref(empty), ns, T, None) == C.FZ_OK, C.last_error()
            assert C.lib.fz_run_block_loss_grad_stream_major(p._h, ctypes.byref(empty), ns, 100, 0, T, None) == C.FZ_OK, C.last_error()
        empty.struct_size = 8                                     # ... but a bad struct_size is refused even then
        assert C.lib.fz_run_block_loss_grad(p._h, ctypes.byref(empty), 0, 0, None) == C.FZ_E_INVALID


# ---- the loss kernels for gfx950 -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(GG.SUPPORTED))
def test_loss_kernels_jit_compile_without_scratch_or_vgpr_spills(name, capsys):
    p = prog_of(name)
    lines = []
    for sm in (False, True):
        r, plain = p.loss_grad_resources(stream_major=sm), p.grad_resources(stream_major=sm)
        sym, psym = p.loss_grad_kernel_symbol(stream_major=sm), p.grad_kernel_symbol(stream_major=sm)
        assert sym != psym and sym == psym.replace("fz_adjoint_", "fz_adjoint_loss_", 1), (sym, psym)   # the same C, R, lanes and graph tag
        assert r["scratch_bytes"] == 0 and r["vgpr_spills"] == 0, r
        assert r["lds_bytes"] == plain["lds_bytes"] and r["unroll"] == plain["unroll"]
        assert r["vgprs"] + r["agprs"] <= 256
        lines.append(f"{sym}: {r['vgprs']} VGPRs ({plain['vgprs']} plain), {r['sgpr_spills']} SGPR spills ({plain['sgpr_spills']} plain), {r['lds_bytes']} B LDS")
    with capsys.disabled():                                       # (SGPR spills are reported, not asserted: correct, slower)
        print("\n" + "\n".join(lines))


def test_the_plain_adjoint_kernels_are_untouched_by_the_loss_variant(tmp_path):
    """grad_source() and grad_kernel_symbol() of the plain adjoint in a process that never asked for a loss kernel, and in this one before
    and after a loss kernel was built"""
    code = ("import sys, json, hashlib\nsys.path.insert(0, %r)\nsys.path.insert(0, %r)\nimport grad_graphs as GG\nfrom zignal_amd import flowz as F\n"
            "p = F.compile(F.from_sexpr(GG.SUPPORTED['moog_ladder']()))\n"
            "print(json.dumps([[p.grad_kernel_symbol(0, sm), hashlib.sha256(p.grad_source(0, sm).encode()).hexdigest()] for sm in (False, True)]))\n"
            ) % (os.path.dirname(HERE), HERE)
    never = eval(subprocess.check_output([sys.executable, "-c", code], text=True).splitlines()[-1])
    import hashlib
    p = prog_of("moog_ladder")
    snap = lambda: [[p.grad_kernel_symbol(0, sm), hashlib.sha256(p.grad_source(0, sm).encode()).hexdigest()] for sm in (False, True)]   # noqa: E731
    before = snap()
    for sm in (False, True):
        p.loss_grad_resources(stream_major=sm)
        src = p.loss_grad_source(stream_major=sm)
        assert "#define FZ_LOSS 1 " in src and "static void out(" in src
        assert "#define FZ_LOSS 0 " in p.grad_source(0, sm) and "static void out(" not in p.grad_source(0, sm)
    assert before == snap() == never


def test_a_manifest_with_a_sound_and_an_impossible_loss_variant_builds_one_and_refuses_one(tmp_path):
    expr = F.from_sexpr(GG.SUPPORTED["integrator"]())
    recipe = recipe_of(GG.SUPPORTED["integrator"]())
    c = symbol_shape(F.compile(expr).loss_grad_kernel_symbol(), "c")[0]
    path = tmp_path / "m.fzm"
    write_manifest(path, [(1, c, 256, ADJOINT | ADJOINT_LOSS, recipe), (1, c, 256, ADJOINT | ADJOINT_LOSS | 256, recipe)])   # (a forward flag next to it: nothing the backward makes)
    r = replay(path, {"FLOWZ_HIP_CACHE": str(tmp_path / "cache")}, jobs=2)
    assert r["records"] == 2 and r["built"] == 1 and r["failed"] == 1 and r["at_hand"] == 0, r
    assert len(code_objects(tmp_path / "cache")) == 1
    # the loss bit without the adjoint bit is no variant of anything: a caller's forward variant with it is refused as reserved
    with pytest.raises(F.FlowzError):
        F.compile(expr).build(F.make_variant(1, 8, 256, ADJOINT_LOSS))


def test_the_recorded_manifest_holds_the_loss_kernels_of_the_gpu_tests(tmp_path):
    """tests/golden/loss_grad_kernels.fzm.gz: every record a loss variant, none refused"""
    import gzip
    path = os.path.join(HERE, "golden", "loss_grad_kernels.fzm.gz")
    flags = [int(m.group(1)) for m in re.finditer(rb"FZM1 \d+ \d+ 256 (\d+) \d+\n", gzip.open(path, "rb").read())]
    assert flags and all(f & ADJOINT and f & ADJOINT_LOSS for f in flags) and any(f & ADJOINT_SM for f in flags)
    r = F.manifest_build(path)
    assert r["failed"] == 0 and r["at_hand"] + r["built"] == r["records"] == len(flags), r


# ---- the numpy restatement against float64 autograd of the mean squared error --------------------------------------------------------
@pytest.mark.parametrize("name", ["df1", "moog_ladder"])
def test_restatement_matches_float64_autograd_of_the_mse(name):
    import torch

    p = prog_of(name)
    ns, T = 16, 24
    x, s0, par, _, sb = inputs(p, ns, T, 11)
    par = params_for(name, p, ns, np.random.default_rng(7)) if p.n_param else None
    target = (np.random.default_rng(5).standard_normal((T, ns, p.n_out)) * 0.5).astype(F32)
    n = T * ns * p.n_out
    got = LR.loss_grad(p, x, target, 2.0 / n, s0, par, None)
    # float64: the mean squared error of the torch restatement of the IR, and its gradients
    L = A.Layout(p)
    t = lambda a, shape: torch.tensor(np.asarray(a, np.float64).reshape(shape), dtype=torch.float64, requires_grad=True)   # noqa: E731
    xt, st = t(x, x.shape), t(s0, (L.n_state, ns))
    pt = t(par if par is not None else np.zeros((L.n_param, ns)), (L.n_param, ns))
    ct = t(np.repeat(L.consts.astype(np.float64)[:, None], ns, 1), (L.n_const, ns))
    y, _ = A.torch_forward(L, xt, st, pt, ct)
    mse = ((y - torch.tensor(target, dtype=torch.float64)) ** 2).mean()
    grads = torch.autograd.grad(mse, (xt, st, pt, ct), allow_unused=True)
    # the bound test_grad_host.py holds its own restatement to (test_reference_matches_float64_autograd)
    bound = 1e-4
    mean = float(got["loss"].astype(np.float64).sum() / n)
    assert abs(mean - mse.item()) <= bound * mse.item(), (mean, mse.item())
    assert A.rel_err(got["out"], y.detach().numpy()) <= bound
    for k, g in zip(("x", "state", "params", "consts"), grads):
        if g is None or g.numel() == 0:
            continue
        e = A.rel_err(got[k], g.numpy())
        assert e <= bound, (k, e)
