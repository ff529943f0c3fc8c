"""The far backward without a GPU (fz_run_block_far_grad, fz_run_block_far_loss_grad: the backward of graphs with delay lines deeper
than 256 samples, whose rings live in HBM): its scope next to fz_program_ring_grad_check's, the workspace query, the argument checks, the
kernels' resources and instructions (JIT for gfx950), the static rule that picks the path, the kernel manifest of the GPU tests, and
tests/far_grad_ref.py -- the slot <-> age conversion, the restatement against float64 autograd, and its chaining identity."""
import ctypes
import re

import numpy as np
import pytest

import adjoint_ref as A
import far_grad_graphs as FG
import far_grad_ref as FR
import grad_graphs as GG
import ring_grad_graphs as RG
import ring_loss_graphs as RL
from grad_host_harness import (ADJOINT, ADJOINT_LOSS, ADJOINT_RING, LDS_BYTES, FakeCall, assert_no_contraction, empty_args, kernel_ops, recorded_recipe, replay,
                               symbol_shape, write_manifest)
from zignal_amd import _capi as C
from zignal_amd import flowz as F

F32 = np.float32
ADJOINT_FAR = 1                                                    # fz_internal.hpp: FZ_VF_ADJOINT_FAR
FAR_BITS = ADJOINT | ADJOINT_RING | ADJOINT_FAR

far_prog = FG.prog


def stride(p):
    return symbol_shape(p.far_grad_kernel_symbol(), "c")[0]


def counts(p):
    """(n_register_state, n_ring_lines, n_far_lines, the sum of the far depths, the LDS ring slots) of a program"""
    d = [depth for _, depth in p.lines()]
    return (sum(x for x in d if x <= 8), sum(1 for x in d if 8 < x <= 256), sum(1 for x in d if x > 256), sum(x for x in d if x > 256),
            sum(x for x in d if 8 < x <= 256))


# ---- scope -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(FG.FARS))
def test_far_graphs_pass_the_check(name):
    p = far_prog(name)
    assert C.lib.fz_program_far_grad_check(p._h) == C.FZ_OK, C.last_error()
    assert p.far_grad_supported() and p.far_grad_unsupported_reason() == ""
    sym, lsym = p.far_grad_kernel_symbol(), p.far_loss_grad_kernel_symbol()
    assert re.fullmatch(r"fz_adjoint_far_kernel_c(1|2|4|8|16)b(256|128|64)_g[0-9a-f]{8}", sym), sym
    assert lsym == sym.replace("fz_adjoint_far_kernel", "fz_adjoint_far_loss_kernel")
    assert sym.split("_g")[1] == p.kernel_symbol().split("_g")[-1]
    # every other backward keeps refusing every one of them, in the words it had
    assert C.lib.fz_program_ring_grad_check(p._h) == C.FZ_E_UNSUPPORTED and "HBM" in C.last_error() and not p.ring_grad_supported()
    assert C.lib.fz_program_grad_check(p._h) == C.FZ_E_UNSUPPORTED and not p.grad_supported()
    from zignal_amd import autograd as AG
    for front_door in (AG.run_rings, AG.run):
        with pytest.raises(F.FlowzError) as ei:
            front_door(p, None)
        assert ei.value.code == C.FZ_E_UNSUPPORTED


@pytest.mark.parametrize("name", sorted(RG.RINGS) + sorted(GG.SUPPORTED))
def test_for_a_graph_without_a_far_line_the_calls_are_the_ring_calls(name):
    p = F.compile(F.from_sexpr((RG.RINGS.get(name) or GG.SUPPORTED[name])()))
    assert C.lib.fz_program_far_grad_check(p._h) == C.FZ_OK, C.last_error()
    assert p.far_grad_supported()
    for c in (0, 1, 4):
        assert p.far_grad_kernel_symbol(c) == p.ring_grad_kernel_symbol(c)
        assert p.far_grad_source(c) == p.ring_grad_source(c)
        if p.n_out:
            assert p.far_loss_grad_kernel_symbol(c) == p.ring_loss_grad_kernel_symbol(c)
            assert p.far_loss_grad_source(c) == p.ring_loss_grad_source(c)
        for ns, T in ((1, 1), (63, 7), (1000, 1000)):
            assert p.far_grad_workspace_bytes(ns, T, c) == p.ring_grad_workspace_bytes(ns, T, c)


@pytest.mark.parametrize("name", sorted(n for n in GG.REFUSED if n not in ("lds_ring_comb", "far_comb")))
def test_refusals_keep_their_reasons(name):
    build, typed, word = GG.REFUSED[name]
    p = F.compile(F.from_sexpr(build()), typed=typed)
    assert C.lib.fz_program_ring_grad_check(p._h) == C.FZ_E_UNSUPPORTED
    why = C.last_error()
    assert C.lib.fz_program_far_grad_check(p._h) == C.FZ_E_UNSUPPORTED
    assert C.last_error() == why and word.lower() in why.lower()
    assert not p.far_grad_supported()
    for call in (lambda: p.far_grad_workspace_bytes(64, 16), p.far_grad_kernel_symbol, p.far_grad_source, p.far_grad_resources,
                 p.far_loss_grad_kernel_symbol, p.far_loss_grad_source, p.far_loss_grad_resources):
        with pytest.raises(F.FlowzError) as ei:
            call()
        assert ei.value.code == C.FZ_E_UNSUPPORTED and word.lower() in str(ei.value).lower()
    for loss in (False, True):
        a = empty_args(loss)
        fn = C.lib.fz_run_block_far_loss_grad if loss else C.lib.fz_run_block_far_grad
        assert fn(p._h, ctypes.byref(a), 64, 16, None) == C.FZ_E_UNSUPPORTED


def test_rings_that_fit_no_workgroup_are_refused_with_the_bytes():
    p = F.compile(F.from_sexpr(RG.six_lines_256()))
    assert C.lib.fz_program_ring_grad_check(p._h) == C.FZ_E_UNSUPPORTED
    why = C.last_error()
    assert C.lib.fz_program_far_grad_check(p._h) == C.FZ_E_UNSUPPORTED and C.last_error() == why
    assert "393216 bytes" in why and str(LDS_BYTES) in why and "LDS" in why, why
    for call in (lambda: p.far_grad_workspace_bytes(64, 16), p.far_grad_kernel_symbol, p.far_grad_resources):
        with pytest.raises(F.FlowzError) as ei:
            call()
        assert ei.value.code == C.FZ_E_UNSUPPORTED and "393216" in str(ei.value)


def test_a_forward_variant_naming_the_far_bit_is_refused_as_reserved():
    p = far_prog("far_comb")
    with pytest.raises(F.FlowzError) as ei:
        p.kernel_name(F.make_variant(1, 8, 256, ADJOINT_FAR), 4096, 64)
    assert ei.value.code == C.FZ_E_INVALID and "reserved" in str(ei.value)


# ---- the workspace query -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(FG.FARS) + sorted(RG.RINGS) + ["df1_cascade6", "moog_ladder"])
def test_workspace_query(name):
    p = F.compile(F.from_sexpr((FG.FARS.get(name) or RG.RINGS.get(name) or GG.SUPPORTED[name])()))
    cd = stride(p)
    assert cd & (cd - 1) == 0 and 1 <= cd <= 16
    n_reg, n_rl, n_fl, far_slots, _ = counts(p)
    if not n_rl and not n_fl:
        n_reg = p.n_state                                             # (no deep line: fz_program_grad_workspace's formula)
    for c in (0, 1, 32):
        for ns, T in ((1, 1), (1000, 15), (1000, 16), (1000, 17), (63, 1000), (65537, 33)):
            # the formula include/flowz_hip.h states
            assert p.far_grad_workspace_bytes(ns, T, c) == (-(-T // (c or cd)) * n_reg + T * (n_rl + n_fl) + far_slots) * ns * 4, (c, ns, T)
    for bad in (3, 6, 64):
        with pytest.raises(F.FlowzError) as ei:
            p.far_grad_workspace_bytes(64, 64, bad)
        assert ei.value.code == C.FZ_E_INVALID
        with pytest.raises(F.FlowzError) as ei:
            p.far_grad_kernel_symbol(bad)
        assert ei.value.code == C.FZ_E_INVALID


def test_default_stride_counts_what_a_chunk_keeps():
    """16, halved while C (n_register_state + n_in + n_ring_reads + n_far_reads + (n_far_lines + n_far_reads)) exceeds 64"""
    want = {"far257": 16, "far_comb": 16, "far1031": 16,      # 1 wire + 1 read + (1 line + 1 read) = 4
            "far_tap1": 8,                                     # 1 + 3 + (1 + 3) = 8
            "far_taps": 8,                                     # 1 + 2 + (1 + 2) = 6: 96, 48
            "far_adjacent": 8,                                 # 1 + 2 + (1 + 2) = 6
            "far_mixed": 4,                                    # 4 register rows + 1 + 1 ring read + 1 + (1 + 1) = 9: 144, 72, 36
            "far_two_in": 8}                                   # 2 wires + 2 + (2 + 2) = 8
    for name, c in want.items():
        assert stride(far_prog(name)) == c, name
        assert far_prog(name).far_loss_grad_kernel_symbol() == far_prog(name).far_grad_kernel_symbol().replace("far_kernel", "far_loss_kernel")


# ---- argument checks: grad_host_harness's fake call, for both calls ------------------------------------------------------------------------
class AsRing:
    """a program whose ring workspace query is the far one: what FakeCall(ring=True) asks of it"""

    def __init__(self, p):
        self._p = p

    def __getattr__(self, k):
        return getattr(self._p, "far_grad_workspace_bytes" if k == "ring_grad_workspace_bytes" else k)


def far_fake_call(p, ns, T, loss):
    b = FakeCall(AsRing(p), ns, T, ring=True, loss=loss)
    b.fn = C.lib.fz_run_block_far_loss_grad if loss else C.lib.fz_run_block_far_grad
    return b


@pytest.mark.parametrize("loss", [False, True])
def test_argument_checks(loss):
    p = far_prog("far_comb")
    b = far_fake_call(p, 1000, 40, loss)
    y = "target" if loss else "out_grad"
    size = ctypes.sizeof(C.LossGradArgs if loss else C.GradArgs)
    bad = [
        b.args(struct_size=size - 8),
        b.args(struct_size=size + 8),
        b.args(struct_size=0),
        b.args(checkpoint_rows=3),
        b.args(checkpoint_rows=64),
        b.args(in_=b.addr["in_"] + 4),                          # misaligned
        b.args(const_grad=b.addr["const_grad"] + 8),
        b.args(workspace=b.addr["workspace"] + 4),
        b.args(in_=None),                                        # NULL where a size needs data
        b.args(state=None),
        b.args(**{y: None}),
        b.args(workspace=None),
        b.args(workspace_bytes=b.ws - 4),                        # smaller than the query's answer
        b.args(in_grad=b.addr["in_"]),                           # outputs overlapping inputs / each other / the workspace
        b.args(in_grad=b.addr[y] + 16),
        b.args(state0_grad=b.addr["state"]),
        b.args(const_grad=b.addr["state"]),
        b.args(const_grad=b.addr["state0_grad"]),
        b.args(state0_grad=b.addr["state_grad"] + 16),           # (only the exact alias of state_grad is allowed)
        b.args(workspace=b.addr["in_grad"]),
        b.args(workspace=b.addr[y]),
    ]
    if loss:
        bad += [b.args(loss=b.addr["state"]), b.args(out=b.addr["target"]), b.args(out=b.addr["in_grad"])]
    for i, a in enumerate(bad):
        assert b.run(a) == C.FZ_E_INVALID, (i, C.last_error())
    assert b.run(b.args(workspace_bytes=b.ws - 4)) == C.FZ_E_INVALID and "fz_program_far_grad_workspace" in C.last_error()
    assert b.fn(p._h, None, 10, 10, None) == C.FZ_E_INVALID
    assert b.ws == p.far_grad_workspace_bytes(1000, 40) == (40 + 300) * 1000 * 4
    if C.lib.fz_device_count() == 0:                             # (with a device these fake addresses would be LAUNCHED on: not there)
        assert b.run(b.args()) == C.FZ_E_NO_DEVICE, C.last_error()
        assert b.run(b.args(state0_grad=b.addr["state_grad"])) == C.FZ_E_NO_DEVICE, C.last_error()
        assert b.run(b.args(in_grad=None, state0_grad=None, param_grad=None, const_grad=None, state_grad=None)) == C.FZ_E_NO_DEVICE
    empty = empty_args(loss)
    for ns, T in ((0, 100), (100, 0), (0, 0)):
        assert b.fn(p._h, ctypes.byref(empty), ns, T, None) == C.FZ_OK, C.last_error()
    empty.struct_size = 8
    assert b.fn(p._h, ctypes.byref(empty), 0, 0, None) == C.FZ_E_INVALID


# ---- the kernels for gfx950 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(FG.FARS))
def test_far_kernels_jit_compile_without_scratch(name):
    p = far_prog(name)
    lds_slots = counts(p)[4]
    for c in (0, 1):
        for loss in (False, True):
            r = (p.far_loss_grad_resources if loss else p.far_grad_resources)(c)
            assert r["scratch_bytes"] == 0 and r["vgpr_spills"] == 0, (c, loss, r)
            unroll, block = symbol_shape((p.far_loss_grad_kernel_symbol if loss else p.far_grad_kernel_symbol)(c), "c")
            assert r["unroll"] == unroll
            # the LDS rings alone, and the ring rule's workgroup for them alone: 256 lanes without any
            assert r["lds_bytes"] == lds_slots * block * 4, r
            two = [b for b in (256, 128, 64) if 2 * lds_slots * b * 4 <= LDS_BYTES]
            assert block == two[0]
    if name == "far_comb":
        assert r["lds_bytes"] == 0 and block == 256
    if name == "far_mixed":
        assert r["lds_bytes"] == 17 * 256 * 4


@pytest.mark.parametrize("loss", [False, True])
@pytest.mark.parametrize("name", sorted(FG.FARS))
def test_far_kernel_has_no_fma(name, loss, tmp_path, monkeypatch):
    """the no-contraction rule of grad_host_harness on every far kernel; the far lines use no LDS, so only far_mixed touches it"""
    _, r, _, every = kernel_ops(monkeypatch, tmp_path, FG.FARS[name](), "far_loss_grad_resources" if loss else "far_grad_resources")
    assert_no_contraction(every, divides=name == "far_adjacent", lds=name == "far_mixed")
    if name != "far_mixed":
        assert not [o for o in every if o.startswith("ds_")] and r["lds_bytes"] == 0
    assert "s_barrier" not in every and not [o for o in every if "atomic" in o]


def test_the_far_kernel_has_a_text_of_its_own():
    p = far_prog("far_mixed")
    src = p.far_grad_source()
    assert "#define FZ_FAR 1 " in src and "#define FZ_FAR_SLOTS " in src.split("// ==== fz_graph_body.h ====")[0] and "__syncthreads" not in src and "atomicAdd" not in src and "__shared__" in src
    assert "#define FZ_LOSS 0 " in src and "static void out(" not in src
    lsrc = p.far_loss_grad_source()
    assert "#define FZ_LOSS 1 " in lsrc and "static void out(" in lsrc
    assert lsrc.split("// ==== fz_block_kernel.hip.inc ====")[1] == src.split("// ==== fz_block_kernel.hip.inc ====")[1]
    ring = RG.prog("biquad_comb17").ring_grad_source()
    assert "#define FZ_FAR 0 " in ring and "FZ_NFL" not in ring.split("// ==== fz_graph_body.h ====")[0]


# ---- the static rule that picks the path -------------------------------------------------------------------------------------------------
def fast(p, c=0):
    m = re.search(r"#define FZ_FAR_FAST ([01]) ", p.far_grad_source(c))
    assert m
    assert "#define FZ_FAR_FAST %s " % m.group(1) in p.far_loss_grad_source(c)
    return m.group(1) == "1"


def test_path_choice():
    for name in ("far257", "far_comb", "far1031", "far_two_in"):
        assert fast(far_prog(name)), name
    for name in ("far_tap1", "far_adjacent"):
        assert not fast(far_prog(name)), name
    assert {n: fast(far_prog(n)) for n in FG.FARS} == FG.FAST
    # the rule is about the chunk: at C = 1 no slot is touched twice in a chunk; 300 and 301 never are at least C apart beyond that
    assert fast(far_prog("far_tap1"), 1) and fast(far_prog("far_adjacent"), 1)
    assert not fast(far_prog("far_adjacent"), 2) and not fast(far_prog("far_tap1"), 2)
    assert fast(far_prog("far_comb"), 32) and fast(far_prog("far_taps"), 32)
    # the generated body follows it: the fast path's bwd() takes the chunk's slots in registers, the per-row one the workspace column
    assert "const float* f2, float* fq)" in far_prog("far_comb").far_grad_source() and "float* fa, const unsigned* fpt, size_t ns)" in far_prog("far_tap1").far_grad_source()
    # sweep 1: a far read at least C rows old travels with its chunk's x rows (far_tap1 at C = 8: the reads at 300, 1, 20)
    assert "fz_fr_chunked[3] = {1u, 0u, 1u}" in far_prog("far_tap1").far_grad_source()


# ---- the kernel manifest of the GPU tests (far_grad_graphs.record_manifest records it) -----------------------------------------------------
def test_the_committed_manifest_holds_the_kernels_the_gpu_tests_launch():
    recs = RL.manifest_variants(FG.MANIFEST)
    fars = sorted(v[:4] for v in recs if v[3] & ADJOINT_FAR and v[3] & ADJOINT)
    want = sorted((1, *symbol_shape((p.far_loss_grad_kernel_symbol if loss else p.far_grad_kernel_symbol)(c), "c"), FAR_BITS | (ADJOINT_LOSS if loss else 0))
                  for p, c, loss in FG.kernel_requests())
    assert fars == want
    assert len(set(recs)) <= 60
    counts_ = replay(FG.MANIFEST)
    assert counts_["failed"] == 0 and counts_["records"] == len(set(recs)), counts_


def test_a_manifest_cannot_ask_for_a_far_kernel_the_backward_would_not_make(tmp_path):
    """a wrong block, a C that is no power of two <= 32, the far bit without the ring bit or next to the stream-major bit, a graph
    without a far line: counted as failed, nothing built"""
    far_recipe = next(v[4] for v in RL.manifest_variants(FG.MANIFEST) if v[3] == FAR_BITS and v[1] == 16)
    ring_recipe = recorded_recipe(tmp_path, "ring_grad_graphs", "RINGS['fb9']()", "ring_grad_resources")
    bad = [(1, 16, 512, FAR_BITS, far_recipe), (1, 16, 128, FAR_BITS, far_recipe), (1, 3, 256, FAR_BITS, far_recipe), (1, 64, 256, FAR_BITS, far_recipe),
           (1, 0, 256, FAR_BITS, far_recipe), (2, 16, 256, FAR_BITS, far_recipe), (1, 16, 256, ADJOINT | ADJOINT_FAR, far_recipe),
           (1, 16, 256, FAR_BITS | (1 << 18), far_recipe), (1, 16, 256, FAR_BITS | (1 << 16), far_recipe), (1, 16, 256, ADJOINT | ADJOINT_RING, far_recipe),
           (1, 16, 256, FAR_BITS, ring_recipe)]
    write_manifest(tmp_path / "bad.fzm", bad)
    got = replay(tmp_path / "bad.fzm", {"FLOWZ_HIP_CACHE": str(tmp_path / "cache")})
    assert got["failed"] == len(bad) and got["built"] == 0 and got["at_hand"] == 0, got


# ---- tests/far_grad_ref.py -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["far257", "far_two_in", "far_mixed"])
def test_the_conversion_is_its_own_inverse(name):
    p = far_prog(name)
    far = FG.far_rows(p)
    assert far and all(pr >= sum(d for _, d in p.lines()) for _, _, pr in far) and far[-1][2] == p.n_state - 1
    rows = np.random.default_rng(5).standard_normal((p.n_state, 3)).astype(F32)
    D = far[0][1]
    for p0 in (0, 1, D - 1):
        ph = [p0 % d for _, d, _ in far]
        once = FR.convert(rows, ph, far)
        assert np.array_equal(FR.convert(once, ph, far), rows)
        for (r0, d, _), q in zip(far, ph):                         # the header's rule: the value j + 1 samples ago sits in slot (p - 1 - j) mod D
            for j in (0, 1, d - 1):
                assert np.array_equal(once[r0 + j], rows[r0 + (q - 1 - j) % d])
        keep = np.ones(p.n_state, bool)
        for r0, d, _ in far:
            keep[r0:r0 + d] = False
        assert np.array_equal(once[keep], rows[keep])              # register rows, LDS ring rows and phase rows stay
    s0 = FG.inputs(p, 3, 4, 1, p0=D - 3)[1]
    assert FR.phases(s0, far) == [(D - 3) % d for _, d, _ in far]


@pytest.mark.parametrize("p0", [0, 5])
@pytest.mark.parametrize("name", sorted(n for n in FG.FARS if n != "far1031"))
def test_reference_matches_float64_autograd(name, p0):
    """far_grad_ref.grad in the caller's layout against float64 autograd of adjoint_ref.torch_forward in ages: the ring tests' bound"""
    p = far_prog(name)
    far = FG.far_rows(p)
    ns, T = 8, FG.DEEPEST[name] + 40
    x, s0, par, yb, sb, _, _ = FG.inputs(p, ns, T, 11, p0=p0)
    got = FR.grad(p, x, yb, s0, par, sb)
    ph = FR.phases(s0, far)
    n = sum(d for _, d in p.lines())                               # the line rows: adjoint_ref knows no phase rows
    want = A.torch_grad(p, x, yb, FR.convert(s0, ph, far)[:n], par, FR.convert(sb, [(q + T) % d for q, (_, d, _) in zip(ph, far)], far)[:n])
    assert want["state"].shape[0] == n
    assert A.rel_err(FR.convert(got["state"], ph, far)[:n], want["state"]) <= 1e-4
    assert not got["state"][n:].any() and got["state"].shape[0] == p.n_state      # the phase rows: zero
    for k in ("x", "params", "consts"):
        if np.asarray(want[k]).size:
            e = A.rel_err(got[k][:want[k].shape[0]] if k != "x" else got[k], want[k])
            assert e <= 1e-4, (k, e)


@pytest.mark.parametrize("name", sorted(n for n in FG.FARS if n != "far1031"))
def test_reference_chains_bitwise_with_a_first_block_shorter_than_the_line(name):
    """block 2, then block 1 on the same accumulators with block 2's state adjoint AS IT IS -- slots, no permutation: the bits of one
    block; block 1 is D - 2 rows, the state between the blocks carries the phase p0 + T1"""
    p = far_prog(name)
    D = FG.DEEPEST[name]
    ns, T1, T2 = 5, D - 2, D + 5
    x, s0, par, yb, sb, ap, ac = FG.inputs(p, ns, T1 + T2, 13, p0=7)
    whole = FR.grad(p, x, yb, s0, par, sb, ap, ac)
    _, s_mid = FR.forward(p, x[:T1], s0, par)
    assert FR.phases(s_mid, FG.far_rows(p)) == [(7 + T1) % d for _, d, _ in FG.far_rows(p)]
    second = FR.grad(p, x[T1:], yb[T1:], s_mid, par, sb, ap, ac)
    first = FR.grad(p, x[:T1], yb[:T1], s0, par, second["state"], second["params"], second["consts"])
    same = lambda a, b: np.array_equal(np.asarray(a, F32).view(np.uint32), np.asarray(b, F32).view(np.uint32))   # noqa: E731
    assert same(np.concatenate([first["x"], second["x"]]), whole["x"])
    for k in ("state", "params", "consts"):
        assert same(first[k], whole[k]), k
