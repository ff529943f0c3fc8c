"""The ring backward under a squared-error loss without a GPU (fz_run_block_ring_loss_grad: fz_run_block_loss_grad for graphs with delay
lines deeper than 8 samples): its scope and the refusals that stay, the calls it IS for a graph without such a line, the argument checks
of fz_run_block_loss_grad, the kernel's resources and instructions (JIT for gfx950), the code pins' names for every other kernel, the kernel
manifest of the GPU tests, and tests/loss_grad_ref.py on the ring graphs against float64 autograd of the mean squared error."""
import ctypes
import os
import re

import numpy as np
import pytest

import adjoint_ref as A
import grad_graphs as GG
import loss_grad_ref as LR
import ring_grad_graphs as RG
import ring_loss_graphs as RL
from grad_host_harness import (ADJOINT, ADJOINT_LOSS, ADJOINT_RING, LDS_BYTES, FakeCall, assert_no_contraction, code_pins, empty_args, invalid,
                               kernel_ops, recorded_recipe, replay, symbol_shape, write_manifest)
from zignal_amd import _capi as C
from zignal_amd import flowz as F

F32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
RING_LOSS_BITS = ADJOINT | ADJOINT_RING | ADJOINT_LOSS
NEW_EXPORTS = ("fz_run_block_ring_loss_grad", "fz_program_ring_loss_grad_resources", "fz_program_ring_loss_grad_kernel_symbol",
               "fz_program_ring_loss_grad_source")


def test_the_new_entry_points_are_declared_and_exported():
    header = open(os.path.join(HERE, "..", "include", "flowz_hip.h")).read()
    for name in NEW_EXPORTS:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in C.EXPORTS and getattr(C.lib, name)


# ---- scope -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(RL.GRAPHS))
def test_the_ten_graphs_are_taken(name):
    p = RL.prog(name)
    assert C.lib.fz_program_ring_grad_check(p._h) == C.FZ_OK, C.last_error()
    sym = p.ring_loss_grad_kernel_symbol()
    assert re.fullmatch(r"fz_adjoint_ring_loss_kernel_c(1|2|4|8|16)b(256|128|64)_g[0-9a-f]{8}", sym), sym
    # the C, the lanes and the graph tag of the plain ring kernel, at the default stride and at a given one
    for c in (0, 1, 4):
        assert p.ring_loss_grad_kernel_symbol(c) == p.ring_grad_kernel_symbol(c).replace("fz_adjoint_ring_", "fz_adjoint_ring_loss_", 1)
    src = p.ring_loss_grad_source()
    assert "#define FZ_LOSS 1 " in src and "#define FZ_LOSS 0 " in p.ring_grad_source() and "fz_adj_ring_args" in src and "const float* rv, float* y)" in src and "__syncthreads" not in src
    assert "static void out(" not in p.ring_grad_source()
    # an empty block is FZ_OK with nothing touched
    for ns, T in ((0, 100), (100, 0), (0, 0)):
        assert C.lib.fz_run_block_ring_loss_grad(p._h, ctypes.byref(empty_args(True)), ns, T, None) == C.FZ_OK, C.last_error()
    # the loss calls without the rings keep refusing it
    with pytest.raises(F.FlowzError) as ei:
        p.loss_grad_resources()
    assert ei.value.code == C.FZ_E_UNSUPPORTED and "LDS" in str(ei.value)


def test_the_two_output_graphs_have_two_outputs_and_rings():
    for name, n_param in (("two_out_ff", 0), ("two_out_fb", 1)):
        p = RL.prog(name)
        assert p.n_out == 2 and p.n_param == n_param and max(d for _, d in p.lines()) == RL.DEEPEST[name] > 8


@pytest.mark.parametrize("name", sorted(n for n in GG.REFUSED if n != "lds_ring_comb"))
def test_refusals_keep_their_reasons(name):
    build, typed, word = GG.REFUSED[name]
    p = F.compile(F.from_sexpr(build()), typed=typed)
    assert C.lib.fz_program_grad_check(p._h) == C.FZ_E_UNSUPPORTED
    why = C.last_error()
    assert word.lower() in why.lower()
    for ns, T in ((64, 16), (0, 0)):
        assert C.lib.fz_run_block_ring_loss_grad(p._h, ctypes.byref(empty_args(True)), ns, T, None) == C.FZ_E_UNSUPPORTED and C.last_error() == why
    for call in (p.ring_loss_grad_kernel_symbol, p.ring_loss_grad_source, p.ring_loss_grad_resources):
        with pytest.raises(F.FlowzError) as ei:
            call()
        assert ei.value.code == C.FZ_E_UNSUPPORTED and word.lower() in str(ei.value).lower()


def test_rings_that_fit_no_workgroup_are_refused_with_the_bytes():
    p = F.compile(F.from_sexpr(RG.six_lines_256()))
    for ns, T in ((64, 16), (0, 0)):
        assert C.lib.fz_run_block_ring_loss_grad(p._h, ctypes.byref(empty_args(True)), ns, T, None) == C.FZ_E_UNSUPPORTED
        why = C.last_error()
        assert "393216 bytes" in why and str(LDS_BYTES) in why and "LDS" in why, why
    for call in (p.ring_loss_grad_kernel_symbol, p.ring_loss_grad_source, p.ring_loss_grad_resources):
        with pytest.raises(F.FlowzError) as ei:
            call()
        assert ei.value.code == C.FZ_E_UNSUPPORTED and "393216" in str(ei.value)


def test_the_other_loss_calls_still_refuse_the_ring_comb():
    p = RL.prog("lds_ring_comb")
    a = empty_args(True)
    calls = (lambda: C.lib.fz_run_block_loss_grad(p._h, ctypes.byref(a), 64, 16, None),
             lambda: C.lib.fz_run_block_loss_grad_stream_major(p._h, ctypes.byref(a), 64, 16, 0, 16, None),
             lambda: C.lib.fz_run_recording_loss_grad(p._h, ctypes.byref(a), 0, 64, 0, 0, 16, 0, None, None),
             lambda: C.lib.fz_run_recording_loss_grad(p._h, ctypes.byref(a), 1, 64, 16, 0, 16, 0, None, None))
    for call in calls:
        assert call() == C.FZ_E_UNSUPPORTED and "LDS" in C.last_error(), C.last_error()
    g = empty_args()
    assert C.lib.fz_run_recording_grad(p._h, ctypes.byref(g), 0, 64, 0, 0, 16, 0, None, None) == C.FZ_E_UNSUPPORTED and "LDS" in C.last_error()
    for sm in (False, True):
        for call in (p.loss_grad_kernel_symbol, p.loss_grad_resources, p.loss_grad_source):
            with pytest.raises(F.FlowzError) as ei:
                call(stream_major=sm)
            assert ei.value.code == C.FZ_E_UNSUPPORTED and "LDS" in str(ei.value)
    with pytest.raises(F.FlowzError) as ei:
        p.recording_workspace_bytes(64, 16)
    assert ei.value.code == C.FZ_E_UNSUPPORTED and "LDS" in str(ei.value)
    from zignal_amd import autograd as AG
    for fn in (AG.mse, AG.mse_recording):
        with pytest.raises(F.FlowzError) as ei:
            fn(p, None, None)
        assert ei.value.code == C.FZ_E_UNSUPPORTED and "LDS" in str(ei.value)


def test_mse_rings_refuses_what_the_ring_check_refuses():
    from zignal_amd import autograd as AG
    p = F.compile(F.from_sexpr(RG.six_lines_256()))
    with pytest.raises(F.FlowzError) as ei:
        AG.mse_rings(p, None, None)
    assert ei.value.code == C.FZ_E_UNSUPPORTED and str(ei.value).endswith(p.ring_grad_unsupported_reason()) and "393216" in str(ei.value)


def test_a_forward_variant_naming_ring_and_loss_is_refused_as_reserved():
    p = RL.prog("fb9")
    for flags in (ADJOINT_RING | ADJOINT_LOSS, RING_LOSS_BITS):
        with pytest.raises(F.FlowzError) as ei:
            p.kernel_name(F.make_variant(1, 8, 256, flags), 4096, 64)
        assert ei.value.code == C.FZ_E_INVALID and "reserved" in str(ei.value)
        with pytest.raises(F.FlowzError):
            p.build(F.make_variant(1, 8, 256, flags))


# ---- a graph without a ring line: the calls ARE the time-major loss calls ------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(GG.SUPPORTED))
def test_for_a_graph_without_a_ring_the_calls_are_the_loss_grad_calls(name):
    p = F.compile(F.from_sexpr(GG.SUPPORTED[name]()))
    for c in (0, 1, 4):
        assert p.ring_loss_grad_kernel_symbol(c) == p.loss_grad_kernel_symbol(c)
        assert p.ring_loss_grad_source(c) == p.loss_grad_source(c)
    assert p.ring_loss_grad_resources() == p.loss_grad_resources()


# ---- argument checks: fz_run_block_loss_grad's, before a device is needed ------------------------------------------------------------
@pytest.mark.parametrize("name", ["lds_ring_comb", "two_out_fb"])
def test_argument_checks_fail_one_by_one_with_their_reason(name):
    p = RL.prog(name)
    b = FakeCall(p, 1000, 40, ring=True, loss=True)
    assert b.ws == p.ring_grad_workspace_bytes(1000, 40) > 0
    size = ctypes.sizeof(C.LossGradArgs)
    for bad in (size - 8, size + 8, 0, ctypes.sizeof(C.GradArgs)):
        assert invalid(b.run(b.args(struct_size=bad)), "struct_size")
    assert invalid(b.run(b.args(checkpoint_rows=3)), "checkpoint_rows") and invalid(b.run(b.args(checkpoint_rows=64)), "checkpoint_rows")
    assert invalid(b.run(b.args(target=None)), "target")
    assert invalid(b.run(b.args(in_=None)), "in is null") and invalid(b.run(b.args(state=None)), "state")
    if p.n_param:
        assert invalid(b.run(b.args(params=None)), "params")
    assert invalid(b.run(b.args(workspace=None)), "fz_program_ring_grad_workspace")
    assert invalid(b.run(b.args(workspace_bytes=b.ws - 4)), "fz_program_ring_grad_workspace")
    for k in ("in_", "target", "loss", "out", "in_grad", "workspace", "state0_grad"):
        assert invalid(b.run(b.args(**{k: b.addr[k] + 4})), "aligned"), k
    # loss and out are outputs: they overlap nothing, the target included
    for k, other in (("loss", "target"), ("loss", "in_"), ("loss", "state0_grad"), ("loss", "workspace"), ("out", "target"), ("out", "in_"),
                     ("out", "in_grad"), ("out", "loss"), ("out", "state"), ("in_grad", "target"), ("state0_grad", "target"), ("workspace", "target"),
                     ("workspace", "out")):
        assert invalid(b.run(b.args(**{k: b.addr[other]})), "overlap"), (k, other)
        assert k in C.last_error() and other.rstrip("_") in C.last_error()
    assert invalid(b.run(b.args(state0_grad=b.addr["state_grad"] + 16)), "overlap")      # (only the exact alias of state_grad is allowed)
    assert invalid(b.run(b.args(out=b.addr["target"] + b.size["target"] - 16)), "overlap")
    assert C.lib.fz_run_block_ring_loss_grad(p._h, None, 10, 10, None) == C.FZ_E_INVALID and "null arguments" in C.last_error()
    assert C.lib.fz_run_block_ring_loss_grad(None, ctypes.byref(b.args()), 10, 10, None) == C.FZ_E_INVALID
    big = FakeCall(p, 1, 1, ring=True, loss=True)
    assert big.run(big.args(), ns=1 << 30) == C.FZ_E_UNSUPPORTED and "2^30" in C.last_error()
    # an empty block is FZ_OK and needs no buffer, but a bad struct_size is refused even then
    empty = empty_args(True)
    for ns, T in ((0, 100), (100, 0), (0, 0)):
        assert b.run(empty, ns, T) == C.FZ_OK, C.last_error()
    empty.struct_size = 8
    assert b.run(empty, 0, 0) == C.FZ_E_INVALID
    # what passes every check stops at the missing device (with one, fake addresses are not launched on)
    if C.lib.fz_device_count() == 0:
        assert b.run(b.args()) == C.FZ_E_NO_DEVICE, C.last_error()
        assert b.run(b.args(state0_grad=b.addr["state_grad"])) == C.FZ_E_NO_DEVICE, C.last_error()
        assert b.run(b.args(in_grad=None, state0_grad=None, param_grad=None, const_grad=None, state_grad=None, loss=None, out=None)) == C.FZ_E_NO_DEVICE


# ---- the kernel for gfx950 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(RL.GRAPHS))
def test_ring_loss_kernel_jit_compiles_without_scratch_with_the_ring_kernels_lds(name, capsys):
    p = RL.prog(name)
    depths = [d for _, d in p.lines() if d > 8]
    lines = []
    for c in (0, 1):
        r, plain = p.ring_loss_grad_resources(c), p.ring_grad_resources(c)
        assert r["scratch_bytes"] == 0 and r["vgpr_spills"] == 0, (c, r)
        sym = p.ring_loss_grad_kernel_symbol(c)
        unroll, block = symbol_shape(sym, "c")
        assert r["unroll"] == plain["unroll"] == unroll
        assert r["lds_bytes"] == plain["lds_bytes"] == sum(depths) * block * 4 <= LDS_BYTES, (r, plain)
        assert r["vgprs"] + r["agprs"] <= 256
        lines.append(f"{sym}: {r['vgprs']} VGPRs ({plain['vgprs']} plain ring), {r['sgpr_spills']} SGPR spills ({plain['sgpr_spills']} plain ring), "
                     f"{r['lds_bytes']} B LDS")
    with capsys.disabled():                                       # (SGPR spills are reported, not asserted: correct, slower)
        print("\n" + "\n".join(lines))


@pytest.mark.parametrize("name", ["lds_ring_comb", "two_out_fb", "ks_tanh11"])
def test_ring_loss_kernel_has_no_fma(name, tmp_path, monkeypatch):
    """the method of test_ring_grad_host.py: test_ring_kernel_has_no_fma; and no barrier, no atomic, the rings in LDS"""
    _, _, _, every = kernel_ops(monkeypatch, tmp_path, RL.GRAPHS[name](), "ring_loss_grad_resources")
    assert_no_contraction(every, divides=name == "ks_tanh11", lds=True)


# ---- every existing kernel's code is the parent's: tests/golden/adjoint_code_pins.json, held by test_adjoint_code_pins_host.py --------------
PINS = code_pins()


def test_the_pins_cover_every_graph():
    for kind in ("ring", "ring_loss"):
        assert sorted(k.split("/")[3] for k in PINS if k.startswith(kind + "/tm/c0/")) == sorted(RL.GRAPHS) and set(RG.RINGS) <= set(RL.GRAPHS)
    for kind in ("adjoint", "loss", "states"):
        assert sorted(k.split("/")[2] for k in PINS if k.startswith(kind + "/tm/")) == sorted(GG.SUPPORTED)


@pytest.mark.parametrize("name", sorted(RG.RINGS))
def test_the_ring_kernel_has_the_parents_text(name):
    """the pins name the ring kernel the library makes, at the default stride and at C = 1, and the ring loss kernel is not the ring kernel:
    other instructions, other metadata (that both are the parent's code: test_adjoint_code_pins_host.py)"""
    p = RL.prog(name)
    for c in (0, 1):
        ring, loss = PINS[f"ring/tm/c{c}/{name}"], PINS[f"ring_loss/tm/c{c}/{name}"]
        assert ring["symbol"] == p.ring_grad_kernel_symbol(c) and loss["symbol"] == p.ring_loss_grad_kernel_symbol(c)
        assert loss[".text"] != ring[".text"] and loss[".note"] != ring[".note"]
        assert p.ring_loss_grad_source(c) != p.ring_grad_source(c)


@pytest.mark.parametrize("name", sorted(GG.SUPPORTED))
def test_the_adjoint_loss_and_states_kernels_have_the_parents_texts(name):
    """the pins name this graph's kernels, and for a graph without a ring line the ring loss kernel IS the loss kernel"""
    p = F.compile(F.from_sexpr(GG.SUPPORTED[name]()))
    for sm, layout in ((False, "tm"), (True, "sm")):
        assert PINS[f"adjoint/{layout}/{name}"]["symbol"] == p.grad_kernel_symbol(0, sm)
        assert PINS[f"loss/{layout}/{name}"]["symbol"] == p.loss_grad_kernel_symbol(0, sm)
        assert PINS[f"states/{layout}/{name}"]["symbol"] == p.states_kernel_symbol(sm)
    assert p.ring_loss_grad_source() == p.loss_grad_source()


# ---- the kernel manifest of the GPU tests ------------------------------------------------------------------------------------------
def test_the_committed_manifest_holds_exactly_the_kernels_the_gpu_tests_launch():
    recs = RL.manifest_variants()
    got = sorted((v[:4], v[4]) for v in recs if v[3] == RING_LOSS_BITS)
    want = []
    for p, c in RL.kernel_requests():
        want.append((1, *symbol_shape(p.ring_loss_grad_kernel_symbol(c), "c"), RING_LOSS_BITS))
    assert sorted(g[0] for g in got) == sorted(want) and len(set(got)) == len(got) == len(want)
    assert len({g[1] for g in got}) == len(RL.GRAPHS)             # one recipe per graph, two strides each
    # nothing else but the plain ring kernels and the forward kernels the comparisons launch
    others = [v for v in recs if v[3] != RING_LOSS_BITS]
    assert sorted(v[:4] for v in others if v[3] & ADJOINT) == sorted((1, *symbol_shape(RL.prog(n).ring_grad_kernel_symbol(), "c"), ADJOINT | ADJOINT_RING)
                                                                    for n in RL.GRAPHS)
    assert all(not (v[3] & (ADJOINT_LOSS | ADJOINT_RING)) for v in others if not v[3] & ADJOINT) and len(set(recs)) <= 60
    # what the library rebuilds from it is what the programs resolve now (at hand or built, none failed)
    counts = replay(RL.MANIFEST)
    assert counts["failed"] == 0 and counts["records"] == len(set(recs)), counts


def test_a_manifest_cannot_ask_for_a_ring_loss_kernel_the_backward_would_not_make(tmp_path):
    """a wrong block, a C that is no power of two <= 32, a graph without a ring: counted as failed, nothing built.  (A graph without
    outputs -- refused by the same check, as the n_out == 0 refusal of the call itself -- cannot be written down: every expression of
    the notation has an output wire.)"""
    block, ring_recipe = next((v[2], v[4]) for v in RL.manifest_variants() if v[3] == RING_LOSS_BITS)
    plain_recipe = recorded_recipe(tmp_path, "grad_graphs", "SUPPORTED['integrator']()", "grad_resources")
    bad = [(1, 16, 512, ring_recipe), (1, 16, block // 2 if block > 64 else 128, ring_recipe), (1, 3, block, ring_recipe), (1, 64, block, ring_recipe),
           (1, 0, block, ring_recipe), (2, 16, block, ring_recipe), (1, 16, 256, plain_recipe)]
    write_manifest(tmp_path / "bad.fzm", [(P, U, blk, RING_LOSS_BITS, recipe) for P, U, blk, recipe in bad])
    counts = replay(tmp_path / "bad.fzm", {"FLOWZ_HIP_CACHE": str(tmp_path / "cache")})
    assert counts["failed"] == len(bad) and counts["built"] == 0 and counts["at_hand"] == 0, counts


# ---- the numpy restatement on the ten graphs against float64 autograd of the mean squared error ---------------------------------------
@pytest.mark.parametrize("name", sorted(RL.GRAPHS))
def test_restatement_matches_float64_autograd_of_the_mse(name):
    p = RL.prog(name)
    ns, T = 8, 300 if name == "tap256" else 96
    x, s0, par, tg, _, _, _, _ = RL.draw(p, ns, T, 11)
    n = T * ns * p.n_out
    got = LR.loss_grad(p, x, tg, 2.0 / n, s0, par, None, ref=A)
    mse, y, grads = RL.mse_float64(p, x, tg, s0, par)
    bound = 1e-4                                                  # the bound test_ring_grad_host.py holds the plain restatement to
    mean = float(got["loss"].astype(np.float64).sum() / n)
    assert abs(mean - mse) <= bound * mse, (mean, mse)
    assert A.rel_err(got["out"], y) <= bound
    for k, g in grads.items():
        if g.size == 0:
            continue
        e = A.rel_err(got[k][:g.shape[0]] if k != "x" else got[k], g)
        assert e <= bound, (k, e)


@pytest.mark.parametrize("name", sorted(RL.GRAPHS))
def test_restatement_chains_bitwise_with_a_first_block_shorter_than_the_line(name):
    """block 2, then block 1 on the same accumulators (loss included) with block 2's state adjoint: the bits of one block -- block 1 is
    D - 2 rows"""
    p = RL.prog(name)
    D = RL.DEEPEST[name]
    ns, T1, T2 = 5, D - 2, D + 5
    x, s0, par, tg, sb, ap, ac, al = RL.draw(p, ns, T1 + T2, 13)
    whole = LR.loss_grad(p, x, tg, RL.K, s0, par, sb, ap, ac, al, ref=A)
    _, s_mid = A.forward(p, x[:T1], s0, par)
    second = LR.loss_grad(p, x[T1:], tg[T1:], RL.K, s_mid, par, sb, ap, ac, al, ref=A)
    first = LR.loss_grad(p, x[:T1], tg[:T1], RL.K, s0, par, second["state"], second["params"], second["consts"], second["loss"], ref=A)
    same = lambda a, b: np.array_equal(np.asarray(a, F32).view(np.uint32), np.asarray(b, F32).view(np.uint32))   # noqa: E731
    assert same(np.concatenate([first["x"], second["x"]]), whole["x"]) and same(np.concatenate([first["out"], second["out"]]), whole["out"])
    for k in ("state", "params", "consts", "loss"):
        assert same(first[k], whole[k]), k
