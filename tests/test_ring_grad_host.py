"""The ring backward without a GPU (fz_run_block_ring_grad: the backward of graphs with delay lines deeper than 8 samples): its scope next
to fz_program_grad_check's, the workspace query, the argument checks, the kernel's resources and instructions (JIT for gfx950), the
texts of the other adjoint kernels (unchanged), the kernel manifest of the GPU tests, and tests/adjoint_ref.py on the ring graphs
against float64 autograd."""
import ctypes
import re

import numpy as np
import pytest

import adjoint_ref as A
import grad_graphs as GG
import ring_grad_graphs as RG
import ring_loss_graphs as RL
from grad_host_harness import (ADJOINT, ADJOINT_RING, LDS_BYTES, FakeCall, assert_no_contraction, code_pins, empty_args, kernel_ops, recorded_recipe, replay,
                               symbol_shape, write_manifest)
from zignal_amd import _capi as C
from zignal_amd import flowz as F

F32 = np.float32
RING_BITS = ADJOINT | ADJOINT_RING

ring_prog = RG.prog


def stride(p):
    return symbol_shape(p.ring_grad_kernel_symbol(), "c")[0]


# ---- scope -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(RG.RINGS))
def test_ring_graphs_pass_the_check(name):
    p = ring_prog(name)
    assert C.lib.fz_program_ring_grad_check(p._h) == C.FZ_OK, C.last_error()
    assert p.ring_grad_supported() and p.ring_grad_unsupported_reason() == ""
    sym = p.ring_grad_kernel_symbol()
    assert re.fullmatch(r"fz_adjoint_ring_kernel_c(1|2|4|8|16)b(256|128|64)_g[0-9a-f]{8}", sym), sym
    assert sym.split("_g")[1] == p.kernel_symbol().split("_g")[-1]
    # the plain backward keeps refusing every one of them
    assert C.lib.fz_program_grad_check(p._h) == C.FZ_E_UNSUPPORTED and not p.grad_supported()


@pytest.mark.parametrize("name", sorted(GG.SUPPORTED))
def test_for_a_graph_without_a_ring_the_calls_are_the_grad_calls(name):
    p = F.compile(F.from_sexpr(GG.SUPPORTED[name]()))
    assert C.lib.fz_program_ring_grad_check(p._h) == C.FZ_OK, C.last_error()
    for c in (0, 1, 4):
        assert p.ring_grad_kernel_symbol(c) == p.grad_kernel_symbol(c)
        assert p.ring_grad_source(c) == p.grad_source(c)
        for ns, T in ((1, 1), (63, 7), (1000, 1000)):
            assert p.ring_grad_workspace_bytes(ns, T, c) == p.grad_workspace_bytes(ns, T, c)


@pytest.mark.parametrize("name", sorted(n for n in GG.REFUSED if n != "lds_ring_comb"))
def test_refusals_keep_their_reasons(name):
    build, typed, word = GG.REFUSED[name]
    p = F.compile(F.from_sexpr(build()), typed=typed)
    assert C.lib.fz_program_grad_check(p._h) == C.FZ_E_UNSUPPORTED
    why = C.last_error()
    assert C.lib.fz_program_ring_grad_check(p._h) == C.FZ_E_UNSUPPORTED
    assert C.last_error() == why and word.lower() in why.lower()
    assert not p.ring_grad_supported()
    for call in (lambda: p.ring_grad_workspace_bytes(64, 16), p.ring_grad_kernel_symbol, p.ring_grad_source, p.ring_grad_resources):
        with pytest.raises(F.FlowzError) as ei:
            call()
        assert ei.value.code == C.FZ_E_UNSUPPORTED and word.lower() in str(ei.value).lower()
    a = empty_args()
    assert C.lib.fz_run_block_ring_grad(p._h, ctypes.byref(a), 64, 16, None) == C.FZ_E_UNSUPPORTED


def test_far_comb_says_hbm():
    p = F.compile(F.from_sexpr(GG.REFUSED["far_comb"][0]()))
    assert C.lib.fz_program_ring_grad_check(p._h) == C.FZ_E_UNSUPPORTED and "HBM" in C.last_error()


def test_rings_that_fit_no_workgroup_are_refused_with_the_bytes():
    p = F.compile(F.from_sexpr(RG.six_lines_256()))
    assert C.lib.fz_program_ring_grad_check(p._h) == C.FZ_E_UNSUPPORTED
    why = C.last_error()
    assert "393216 bytes" in why and str(LDS_BYTES) in why and "LDS" in why, why
    for call in (lambda: p.ring_grad_workspace_bytes(64, 16), p.ring_grad_kernel_symbol, p.ring_grad_resources):
        with pytest.raises(F.FlowzError) as ei:
            call()
        assert ei.value.code == C.FZ_E_UNSUPPORTED and "393216" in str(ei.value)
    a = empty_args()
    for ns, T in ((64, 16), (0, 0)):
        assert C.lib.fz_run_block_ring_grad(p._h, ctypes.byref(a), ns, T, None) == C.FZ_E_UNSUPPORTED


def test_the_plain_backward_still_refuses_the_ring_comb():
    p = ring_prog("lds_ring_comb")
    assert C.lib.fz_program_grad_check(p._h) == C.FZ_E_UNSUPPORTED and "LDS" in C.last_error()
    for call in (lambda: p.grad_workspace_bytes(64, 16), p.grad_kernel_symbol):
        with pytest.raises(F.FlowzError) as ei:
            call()
        assert ei.value.code == C.FZ_E_UNSUPPORTED and "LDS" in str(ei.value)
    from zignal_amd import autograd as AG
    with pytest.raises(F.FlowzError) as ei:
        AG.run(p, None)
    assert ei.value.code == C.FZ_E_UNSUPPORTED


def test_a_forward_variant_naming_the_ring_bit_is_refused_as_reserved():
    p = ring_prog("fb9")
    with pytest.raises(F.FlowzError) as ei:
        p.kernel_name(F.make_variant(1, 8, 256, ADJOINT_RING), 4096, 64)
    assert ei.value.code == C.FZ_E_INVALID and "reserved" in str(ei.value)


# ---- the workspace query -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(RG.RINGS))
def test_workspace_query(name):
    p = ring_prog(name)
    cd = stride(p)
    assert cd & (cd - 1) == 0 and 1 <= cd <= 16
    n_ring_lines = sum(1 for _, depth in p.lines() if depth > 8)
    n_reg = sum(depth for _, depth in p.lines() if depth <= 8)
    for c in (0, 1, 2, 4, 8, 16, 32):
        last = 0
        for T in (1, 2, 15, 16, 17, 100, 1000):
            b = p.ring_grad_workspace_bytes(1000, T, c)
            assert b == (-(-T // (c or cd)) * n_reg + T * n_ring_lines) * 1000 * 4     # the formula include/flowz_hip.h states
            assert b >= last and b > 0
            last = b
        last = 0
        for ns in (1, 63, 64, 65, 1000, 65537):
            b = p.ring_grad_workspace_bytes(ns, 100, c)
            assert b > last
            last = b
    for ns, T in ((1, 1), (63, 7), (1000, 1000), (65537, 33)):
        assert p.ring_grad_workspace_bytes(ns, T) == p.ring_grad_workspace_bytes(ns, T, cd)
    for bad in (3, 6, 64):
        with pytest.raises(F.FlowzError) as ei:
            p.ring_grad_workspace_bytes(64, 64, bad)
        assert ei.value.code == C.FZ_E_INVALID
        with pytest.raises(F.FlowzError) as ei:
            p.ring_grad_kernel_symbol(bad)
        assert ei.value.code == C.FZ_E_INVALID


def test_default_stride_counts_what_a_chunk_keeps():
    """16, halved while C (n_register_state + n_in + n_ring_reads) exceeds 64"""
    want = {"fb9": 16, "ff16": 16, "lds_ring_comb": 16, "tap256": 16, "taps12_31": 16, "ks_tanh11": 16, "two_in": 16,
            "biquad_comb17": 8}       # (4 register rows + 1 wire + 1 ring read: 16 x 6 = 96 floats, 8 x 6 = 48)
    for name, c in want.items():
        assert stride(ring_prog(name)) == c, name


# ---- argument checks: every one fails before the device is needed, and they are fz_run_block_grad's --------------------------------
@pytest.mark.parametrize("name", ["lds_ring_comb", "biquad_comb17"])
def test_argument_checks(name):
    p = ring_prog(name)
    b = FakeCall(p, 1000, 40, ring=True)
    bad = [
        b.args(struct_size=ctypes.sizeof(C.GradArgs) - 8),
        b.args(struct_size=ctypes.sizeof(C.GradArgs) + 8),
        b.args(struct_size=0),
        b.args(checkpoint_rows=3),
        b.args(checkpoint_rows=64),
        b.args(in_=b.addr["in_"] + 4),                          # misaligned
        b.args(const_grad=b.addr["const_grad"] + 8),
        b.args(workspace=b.addr["workspace"] + 4),
        b.args(in_=None),                                        # NULL where a size needs data
        b.args(state=None),
        b.args(out_grad=None),
        b.args(workspace=None),
        b.args(workspace_bytes=b.ws - 4),                        # smaller than the query's answer
        b.args(in_grad=b.addr["in_"]),                           # outputs overlapping inputs / each other / the workspace
        b.args(in_grad=b.addr["out_grad"] + 16),
        b.args(state0_grad=b.addr["state"]),
        b.args(const_grad=b.addr["state"]),
        b.args(const_grad=b.addr["state0_grad"]),
        b.args(state0_grad=b.addr["state_grad"] + 16),           # (only the exact alias of state_grad is allowed)
        b.args(workspace=b.addr["in_grad"]),
        b.args(workspace=b.addr["out_grad"]),
    ]
    if p.n_param:
        bad += [b.args(params=None), b.args(param_grad=b.addr["params"]), b.args(param_grad=b.addr["param_grad"] + 8)]
    for i, a in enumerate(bad):
        assert b.run(a) == C.FZ_E_INVALID, (i, C.last_error())
    assert b.run(b.args(workspace_bytes=b.ws - 4)) == C.FZ_E_INVALID and "fz_program_ring_grad_workspace" in C.last_error()
    assert C.lib.fz_run_block_ring_grad(p._h, None, 10, 10, None) == C.FZ_E_INVALID
    assert b.ws == p.ring_grad_workspace_bytes(1000, 40) > 0
    # the exact alias and NULL outputs pass every check: without a device the call then stops at FZ_E_NO_DEVICE (with one these fake
    # addresses would be LAUNCHED on: not there -- test_ring_grad_gpu.py runs the alias and the NULL outputs on real buffers)
    if C.lib.fz_device_count() == 0:
        assert b.run(b.args(state0_grad=b.addr["state_grad"])) == C.FZ_E_NO_DEVICE, C.last_error()
        assert b.run(b.args(in_grad=None, state0_grad=None, param_grad=None, const_grad=None, state_grad=None)) == C.FZ_E_NO_DEVICE
    # an empty block is FZ_OK and touches nothing: no buffer is needed at all
    empty = empty_args()
    for ns, T in ((0, 100), (100, 0), (0, 0)):
        assert C.lib.fz_run_block_ring_grad(p._h, ctypes.byref(empty), ns, T, None) == C.FZ_OK, C.last_error()
    empty.struct_size = 8
    assert C.lib.fz_run_block_ring_grad(p._h, ctypes.byref(empty), 0, 0, None) == C.FZ_E_INVALID


# ---- the kernel for gfx950 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(RG.RINGS))
def test_ring_kernel_jit_compiles_without_scratch(name):
    p = ring_prog(name)
    depths = [d for _, d in p.lines() if d > 8]
    for c in (0, 1):
        r = p.ring_grad_resources(c)
        assert r["scratch_bytes"] == 0 and r["vgpr_spills"] == 0, (c, r)
        sym = p.ring_grad_kernel_symbol(c)
        unroll, block = symbol_shape(sym, "c")
        assert r["unroll"] == unroll
        assert r["lds_bytes"] == sum(depths) * block * 4 <= LDS_BYTES, r
        # the largest of 256 / 128 / 64 lanes that leaves room for two workgroups per compute unit, else the largest that fits one
        two = [b for b in (256, 128, 64) if 2 * sum(depths) * b * 4 <= LDS_BYTES]
        assert block == (two[0] if two else [b for b in (256, 128, 64) if sum(depths) * b * 4 <= LDS_BYTES][0])
    if name == "tap256":
        assert block == 64 and r["lds_bytes"] == 65536


@pytest.mark.parametrize("name", ["lds_ring_comb", "ks_tanh11"])
def test_ring_kernel_has_no_fma(name, tmp_path, monkeypatch):
    """the check of test_grad_host.py: test_adjoint_kernel_has_no_fma; and the kernel keeps its rings in LDS, without a barrier"""
    _, _, _, every = kernel_ops(monkeypatch, tmp_path, RG.RINGS[name](), "ring_grad_resources")
    assert_no_contraction(every, divides=name != "lds_ring_comb", lds=True)


@pytest.mark.parametrize("name", ["df1_cascade6", "moog_ladder", "rules"])
def test_the_other_adjoint_kernels_have_the_parents_texts(name):
    """tests/golden/adjoint_code_pins.json: the code of the adjoint, loss and states kernels in both layouts, recorded from the parent of
    the commit that folded the loss kernels into their siblings; test_adjoint_code_pins_host.py holds what the library builds now to
    them.  Here: the pins name this graph's kernels by the symbols the library gives them, and for a graph without a ring line the ring
    kernel IS the adjoint kernel."""
    pins = code_pins()
    p = F.compile(F.from_sexpr(GG.SUPPORTED[name]()))
    for sm, layout in ((False, "tm"), (True, "sm")):
        assert pins[f"adjoint/{layout}/{name}"]["symbol"] == p.grad_kernel_symbol(0, sm)
        assert pins[f"loss/{layout}/{name}"]["symbol"] == p.loss_grad_kernel_symbol(0, sm)
        assert pins[f"states/{layout}/{name}"]["symbol"] == p.states_kernel_symbol(sm)
    assert p.ring_grad_source() == p.grad_source() and p.ring_grad_kernel_symbol() == p.grad_kernel_symbol()


def test_the_ring_kernel_has_a_text_of_its_own():
    p = ring_prog("biquad_comb17")
    src = p.ring_grad_source()
    assert "fz_adj_ring_args" in src and "FZ_RING_SLOTS" in src and "__shared__" in src and "__syncthreads" not in src
    plain = F.compile(F.from_sexpr(GG.SUPPORTED["df1_cascade6"]())).grad_source()
    assert "fz_adj_ring_args" not in plain and "FZ_RING_SLOTS" not in plain and "ring" not in plain.split("// ==== fz_block_kernel.hip.inc ====")[0]
    assert "#define FZ_LOSS 0 " in src and "#define FZ_LOSS 0 " in plain and "static void out(" not in src + plain
    assert "fz_adj" not in p.source()


# ---- the kernel manifest of the GPU tests (ring_grad_graphs.record_manifest records it) --------------------------------------------------
def test_the_committed_manifest_holds_the_kernels_the_gpu_tests_launch():
    recs = RL.manifest_variants(RG.MANIFEST)
    rings = sorted(v[:4] for v in recs if v[3] == RING_BITS)
    want = sorted((1, *symbol_shape(p.ring_grad_kernel_symbol(c), "c"), RING_BITS) for p, c in RG.kernel_requests())
    assert rings == want
    assert len(set(recs)) <= 40
    # what the library rebuilds from it is what the programs resolve now (at hand or built, none failed)
    counts = replay(RG.MANIFEST)
    assert counts["failed"] == 0 and counts["records"] == len(set(recs)), counts


def test_a_manifest_cannot_ask_for_a_ring_kernel_the_backward_would_not_make(tmp_path):
    """wrong block, a C that is no power of two <= 32, a graph without a ring: counted as failed, nothing built"""
    block, ring_recipe = next((v[2], v[4]) for v in RL.manifest_variants(RG.MANIFEST) if v[3] == RING_BITS)
    plain_recipe = recorded_recipe(tmp_path, "grad_graphs", "SUPPORTED['integrator']()", "grad_resources")
    bad = [(1, 16, 512, ring_recipe), (1, 16, block // 2 if block > 64 else 128, ring_recipe), (1, 3, block, ring_recipe), (1, 64, block, ring_recipe),
           (1, 0, block, ring_recipe), (2, 16, block, ring_recipe), (1, 16, 256, plain_recipe)]
    write_manifest(tmp_path / "bad.fzm", [(P, U, blk, RING_BITS, recipe) for P, U, blk, recipe in bad])
    counts = replay(tmp_path / "bad.fzm", {"FLOWZ_HIP_CACHE": str(tmp_path / "cache")})
    assert counts["failed"] == len(bad) and counts["built"] == 0 and counts["at_hand"] == 0, counts


# ---- the numpy restatement on the ring graphs against float64 autograd ---------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(RG.RINGS))
def test_reference_matches_float64_autograd(name):
    p = ring_prog(name)
    ns, T = 8, 300 if name == "tap256" else 96
    x, s0, par, yb, sb, _, _ = RG.inputs(p, ns, T, 11)
    got = A.grad(p, x, yb, s0, par, sb)
    want = A.torch_grad(p, x, yb, s0, par, sb)
    for k in ("x", "state", "params", "consts"):
        if np.asarray(want[k]).size == 0:
            continue
        e = A.rel_err(got[k][:want[k].shape[0]] if k != "x" else got[k], want[k])
        assert e <= 1e-4, (k, e)


@pytest.mark.parametrize("name", sorted(RG.RINGS))
def test_reference_chains_bitwise_with_a_first_block_shorter_than_the_line(name):
    """block 2, then block 1 on the same accumulators with block 2's state adjoint: the bits of one block -- block 1 is D - 2 rows"""
    p = ring_prog(name)
    D = RG.DEEPEST[name]
    ns, T1, T2 = 5, D - 2, D + 5
    x, s0, par, yb, sb, ap, ac = RG.inputs(p, ns, T1 + T2, 13)
    whole = A.grad(p, x, yb, s0, par, sb, ap, ac)
    _, s_mid = A.forward(p, x[:T1], s0, par)
    second = A.grad(p, x[T1:], yb[T1:], s_mid, par, sb, ap, ac)
    first = A.grad(p, x[:T1], yb[:T1], s0, par, second["state"], second["params"], second["consts"])
    same = lambda a, b: np.array_equal(np.asarray(a, F32).view(np.uint32), np.asarray(b, F32).view(np.uint32))   # noqa: E731
    assert same(np.concatenate([first["x"], second["x"]]), whole["x"])
    for k in ("state", "params", "consts"):
        assert same(first[k], whole[k]), k

