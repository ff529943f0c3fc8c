"""The ring backward without a GPU (fz_run_block_ring_grad: the backward of graphs with delay lines deeper than 8 samples): its scope next
to fz_program_grad_check's, the workspace query, the argument checks, the kernel's resources and instructions (JIT for gfx950), the
texts of the other adjoint kernels (unchanged), the kernel manifest of the GPU tests, and tests/adjoint_ref.py on the ring graphs
against float64 autograd."""
import ctypes
import glob
import gzip
import json
import os
import re
import subprocess

import numpy as np
import pytest

import adjoint_ref as A
import grad_graphs as GG
import ring_grad_graphs as RG
from test_grad_host import FakeBufs
from zignal_amd import _capi as C
from zignal_amd import flowz as F

F32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
MANIFEST = os.path.join(HERE, "golden", "ring_grad_kernels.fzm.gz")
LDS_BYTES = 163840

_progs = {}


def ring_prog(name):
    if name not in _progs:
        _progs[name] = F.compile(F.from_sexpr(RG.RINGS[name]()))
    return _progs[name]


def stride(p):
    return int(p.ring_grad_kernel_symbol().split("_c")[1].split("b")[0])


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
    a = C.GradArgs()
    a.struct_size = ctypes.sizeof(C.GradArgs)
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
    a = C.GradArgs()
    a.struct_size = ctypes.sizeof(C.GradArgs)
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
        p.kernel_name(F.make_variant(1, 8, 256, 1 << 14), 4096, 64)
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
class RingFakeBufs(FakeBufs):
    def __init__(self, p, ns, T):
        FakeBufs.__init__(self, _Ws(p), ns, T)
        self.p = p

    def run(self, a, ns=None, T=None):
        return C.lib.fz_run_block_ring_grad(self.p._h, ctypes.byref(a), self.ns if ns is None else ns, self.T if T is None else T, None)


class _Ws:
    """a program whose grad_workspace_bytes is the ring query (FakeBufs sizes its workspace with it)"""

    def __init__(self, p):
        self._p = p

    def __getattr__(self, k):
        return self._p.ring_grad_workspace_bytes if k == "grad_workspace_bytes" else getattr(self._p, k)


@pytest.mark.parametrize("name", ["lds_ring_comb", "biquad_comb17"])
def test_argument_checks(name):
    p = ring_prog(name)
    b = RingFakeBufs(p, 1000, 40)
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
    empty = C.GradArgs()
    empty.struct_size = ctypes.sizeof(C.GradArgs)
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
        block = int(sym.split("_g")[0].split("b")[1])
        assert r["unroll"] == int(sym.split("_c")[1].split("b")[0])
        assert r["lds_bytes"] == sum(depths) * block * 4 <= LDS_BYTES, r
        # the largest of 256 / 128 / 64 lanes that leaves room for two workgroups per compute unit, else the largest that fits one
        two = [b for b in (256, 128, 64) if 2 * sum(depths) * b * 4 <= LDS_BYTES]
        assert block == (two[0] if two else [b for b in (256, 128, 64) if sum(depths) * b * 4 <= LDS_BYTES][0])
    if name == "tap256":
        assert block == 64 and r["lds_bytes"] == 65536


@pytest.mark.parametrize("name", ["lds_ring_comb", "ks_tanh11"])
def test_ring_kernel_has_no_fma(name, tmp_path, monkeypatch):
    """the check of test_grad_host.py: test_adjoint_kernel_has_no_fma; and the kernel keeps its rings in LDS, without a barrier"""
    monkeypatch.setenv("FLOWZ_HIP_CACHE", str(tmp_path))
    p = F.compile(F.from_sexpr(RG.RINGS[name]()))
    p.ring_grad_resources()
    objs = glob.glob(str(tmp_path / "*.hsaco"))
    assert len(objs) == 1
    dis = subprocess.check_output(["/opt/rocm/lib/llvm/bin/llvm-objdump", "-d", objs[0]], text=True)
    assert p.ring_grad_kernel_symbol() in dis
    lines = [ln.split() for ln in dis.splitlines() if ln.strip()]
    ops = [w[0] for w in lines if w[0].startswith("v_")]
    assert len(ops) > 20
    fused = [o for o in ops if o.startswith(("v_fma", "v_fmac"))]
    divisions, roots = ops.count("v_div_fixup_f32"), ops.count("v_sqrt_f32_e32") + ops.count("v_sqrt_f32_e64")
    assert len(fused) == 5 * divisions + 2 * roots and ops.count("v_div_fmas_f32") == divisions
    assert not [o for o in ops if re.match(r"v_(pk_(fma|mad|mac)|mad|mac)(_mix|_mixlo|_mixhi|_legacy)?_(f16|f32|f64|bf16)", o)]
    if name == "lds_ring_comb":
        assert divisions == 0 and roots == 0 and not fused
    every = [w[0] for w in lines]
    assert any(o.startswith("ds_read") for o in every) and any(o.startswith("ds_write") for o in every)
    assert "s_barrier" not in every and not [o for o in every if "atomic" in o]


@pytest.mark.parametrize("name", ["df1_cascade6", "moog_ladder", "rules"])
def test_the_other_adjoint_kernels_have_the_parents_texts(name):
    """tests/golden/adjoint_code_pins.json: the code of the adjoint, loss and states kernels in both layouts, recorded from the parent of
    the commit that folded the loss kernels into their siblings; test_adjoint_code_pins_host.py holds what the library builds now to
    them.  Here: the pins name this graph's kernels by the symbols the library gives them, and for a graph without a ring line the ring
    kernel IS the adjoint kernel."""
    pins = json.load(open(os.path.join(HERE, "golden", "adjoint_code_pins.json")))
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


# ---- the kernel manifest of the GPU tests ------------------------------------------------------------------------------------------
def kernel_requests():
    """(program, checkpoint_rows) of every ring kernel test_ring_grad_gpu.py launches"""
    out = [(ring_prog(n), 0) for n in sorted(RG.RINGS)]
    out += [(ring_prog(n), c) for n in ("lds_ring_comb", "biquad_comb17") for c in (1, 32)]
    return out


def record_manifest():
    """tests/golden/ring_grad_kernels.fzm.gz: resolve every kernel of kernel_requests() -- and the forward kernels the chaining and
    autograd tests launch -- in a process that records (FLOWZ_HIP_MANIFEST); needs no GPU.  build() replays every manifest under
    tests/golden/, so a GPU run finds them built.  By hand: PYTHONPATH=. python tests/test_ring_grad_host.py"""
    import sys
    import tempfile
    code = ("import sys\nsys.path[:0] = [%r, %r]\nimport test_ring_grad_host as T\nimport ring_grad_graphs as RG\n"
            "for p, c in T.kernel_requests():\n    p.ring_grad_resources(c)\n"
            "for n, shapes in T.FORWARD_SHAPES.items():\n    for ns, rows in shapes:\n        T.ring_prog(n).build(None, ns, rows)\n") % (os.path.dirname(HERE), HERE)
    with tempfile.TemporaryDirectory() as td:
        raw = os.path.join(td, "manifest.fzm")
        subprocess.check_call([sys.executable, "-c", code], env=dict(os.environ, FLOWZ_HIP_MANIFEST=raw))
        with open(raw, "rb") as f, open(MANIFEST, "wb") as out:
            out.write(gzip.compress(f.read(), 9, mtime=0))
    return F.manifest_build(MANIFEST)


# the forward launches of test_ring_grad_gpu.py: (streams, rows) of run_block per graph (chaining: D - 2 rows; autograd: fb9)
FORWARD_SHAPES = {n: [(65, RG.DEEPEST[n] - 2)] for n in RG.RINGS}
FORWARD_SHAPES["fb9"] = FORWARD_SHAPES["fb9"] + [(130, 30)]


def manifest_variants():
    """(P, U, block, flags, recipe) of every record of the committed manifest"""
    text = gzip.open(MANIFEST, "rb").read()
    out, pos = [], 0
    while pos < len(text):
        eol = text.index(b"\n", pos)
        tag, P, U, block, flags, n = text[pos:eol].split()
        assert tag == b"FZM1"
        out.append((int(P), int(U), int(block), int(flags), text[eol + 1:eol + 1 + int(n)]))
        pos = eol + 1 + int(n)
    return out


def test_the_committed_manifest_holds_the_kernels_the_gpu_tests_launch():
    ring_bits = (1 << 27) | (1 << 14)
    recs = manifest_variants()
    rings = sorted(v[:4] for v in recs if v[3] == ring_bits)
    want = sorted((1, int(p.ring_grad_kernel_symbol(c).split("_c")[1].split("b")[0]), int(p.ring_grad_kernel_symbol(c).split("_g")[0].split("b")[1]), ring_bits)
                  for p, c in kernel_requests())
    assert rings == want
    assert len(set(recs)) <= 40
    # what the library rebuilds from it is what the programs resolve now (at hand or built, none failed)
    env = {k: v for k, v in os.environ.items() if k != "FLOWZ_HIP_MANIFEST"}
    out = subprocess.check_output([os.sys.executable, "-c", "import sys\nsys.path.insert(0, %r)\nfrom zignal_amd import flowz as F\nprint(F.manifest_build(%r))"
                                   % (os.path.dirname(HERE), MANIFEST)], env=env, text=True)
    counts = eval(out.strip().splitlines()[-1])
    assert counts["failed"] == 0 and counts["records"] == len(set(recs)), counts


def test_a_manifest_cannot_ask_for_a_ring_kernel_the_backward_would_not_make(tmp_path):
    """wrong block, a C that is no power of two <= 32, a graph without a ring: counted as failed, nothing built"""
    text = gzip.open(MANIFEST, "rb").read()
    ring_bits = (1 << 27) | (1 << 14)
    pos, recipes = 0, {}
    while pos < len(text):
        eol = text.index(b"\n", pos)
        _, P, U, block, flags, n = text[pos:eol].split()
        recipes.setdefault(int(flags) == ring_bits, (int(block), text[eol + 1:eol + 1 + int(n)]))
        pos = eol + 1 + int(n)
    block, ring_recipe = recipes[True]
    _, plain_recipe = F_plain_recipe(tmp_path)
    bad = [(1, 16, 512, ring_recipe), (1, 16, block // 2 if block > 64 else 128, ring_recipe), (1, 3, block, ring_recipe), (1, 64, block, ring_recipe),
           (1, 0, block, ring_recipe), (2, 16, block, ring_recipe), (1, 16, 256, plain_recipe)]
    path = tmp_path / "bad.fzm"
    with open(path, "wb") as f:
        for P, U, blk, recipe in bad:
            f.write(b"FZM1 %d %d %d %d %d\n" % (P, U, blk, ring_bits, len(recipe)) + recipe)
    env = dict({k: v for k, v in os.environ.items() if k != "FLOWZ_HIP_MANIFEST"}, FLOWZ_HIP_CACHE=str(tmp_path / "cache"))
    out = subprocess.check_output([os.sys.executable, "-c", "import sys\nsys.path.insert(0, %r)\nfrom zignal_amd import flowz as F\nprint(F.manifest_build(%r))"
                                   % (os.path.dirname(HERE), str(path))], env=env, text=True)
    counts = eval(out.strip().splitlines()[-1])
    assert counts["failed"] == len(bad) and counts["built"] == 0 and counts["at_hand"] == 0, counts


def F_plain_recipe(tmp_path):
    """the recipe (input types and expression text) of a graph without a ring, as a recording process writes it"""
    raw = tmp_path / "plain.fzm"
    code = ("import sys\nsys.path[:0] = [%r, %r]\nimport grad_graphs as GG\nfrom zignal_amd import flowz as F\n"
            "F.compile(F.from_sexpr(GG.SUPPORTED['integrator']())).grad_source()\nF.compile(F.from_sexpr(GG.SUPPORTED['integrator']())).grad_resources()\n"
            ) % (os.path.dirname(HERE), HERE)
    subprocess.check_call([os.sys.executable, "-c", code], env=dict(os.environ, FLOWZ_HIP_MANIFEST=str(raw), FLOWZ_HIP_CACHE=str(tmp_path / "c0")))
    text = open(raw, "rb").read()
    eol = text.index(b"\n")
    n = int(text[:eol].split()[5])
    return None, text[eol + 1:eol + 1 + n]


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


if __name__ == "__main__":                         # record the kernel manifest of the library as it is
    print("kernel manifest:", record_manifest())
