"""What the host tests of the backward family share (the sibling of tests/grad_harness.py for the files that need no GPU): the variant bits
and the LDS size, empty_args() and invalid(), ONE fake call for every corner of the family (plain or ring, dL/dy or loss, time-major
block or stream-major window, one block or a whole recording), ONE statement of what "no contraction" means in a kernel's disassembly,
the manifest replay and its helpers, the code pins, and the draws the restatement tests share.  Imports without torch and without a
GPU.  tests/test_grad_host_harness_host.py holds the helpers to their word."""
import ctypes
import functools
import glob
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

import grad_harness as H
from zignal_amd import _capi as C
from zignal_amd import flowz as F

F32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ADJOINT, ADJOINT_SM, ADJOINT_LOSS, STATES, ADJOINT_RING, ADJOINT_FAR = 1 << 27, 1 << 18, 1 << 17, 1 << 16, 1 << 14, 1     # fz_internal.hpp
LDS_BYTES = 163840                                                # per CU and the most one workgroup may declare (gfx950)


@functools.lru_cache(None)
def code_pins():
    """tests/golden/adjoint_code_pins.json (tests/adjoint_code_pins.py writes it, test_adjoint_code_pins_host.py holds the library to
    it), loaded once -- on the first call, not on import: the module that writes the file imports this one"""
    return json.load(open(os.path.join(HERE, "golden", "adjoint_code_pins.json")))


def empty_args(loss=False):
    """the args struct of a call with nothing but its size"""
    a = C.LossGradArgs() if loss else C.GradArgs()
    a.struct_size = ctypes.sizeof(a)
    return a


def invalid(rc, word):
    return rc == C.FZ_E_INVALID and word in C.last_error()


# ---- one fake call -----------------------------------------------------------------------------------------------------------------------
class FakeCall:
    """distinct, 16-byte aligned, never dereferenced addresses for exactly the buffers a call of one corner of the family has, in the
    coordinates of grad_harness.launch: the entry point is grad_harness.ENTRY's, the workspace the query launch() makes for that corner.
    window: (rows, row0) of stream-major buffers (rows None: up4(row0 + T)); recording: the block_rows of a call over a whole recording.
    addr / size: per buffer; a buffer of no bytes is passed as null."""

    def __init__(self, p, ns, T, ring=False, loss=False, window=None, recording=None, c=0):
        self.p, self.ns, self.T, self.ring, self.loss, self.B = p, ns, T, bool(ring), bool(loss), recording
        self.sm, self.rec = window is not None, recording is not None
        self.rows, self.row0 = window or (None, 0)
        if self.sm and self.rows is None:
            self.rows = H.up4(self.row0 + T)
        self.fn = getattr(C.lib, H.ENTRY[(self.ring, self.loss, self.sm, self.rec)])
        if self.rec:
            self.ws = p.ring_recording_workspace_bytes(ns, T, recording, c) if ring else p.recording_workspace_bytes(ns, T, recording, c, self.sm)
        else:
            self.ws = (p.ring_grad_workspace_bytes if ring else p.grad_workspace_bytes)(ns, T, c)
        fr, per = (self.rows if self.sm else T) * ns * 4, ns * 4
        self.size = {"in_": fr * p.n_in, "state": p.n_state * per, "params": p.n_param * per, "target" if loss else "out_grad": fr * p.n_out,
                     "state_grad": p.n_state * per, "in_grad": fr * p.n_in, "state0_grad": p.n_state * per, "param_grad": p.n_param * per,
                     "const_grad": p.n_const * per, "workspace": self.ws}
        if loss:
            self.size.update(loss=per, out=fr * p.n_out)
        if self.rec:
            self.size["state_out"] = p.n_state * per
        self.addr, off = {}, 0
        for k, n in self.size.items():
            self.addr[k] = (1 << 40) + off
            off += (2 * max(n, 16) + 4095) // 4096 * 4096       # (room behind each: a call with smaller blocks asks for a larger workspace)

    def args(self, **over):
        a = empty_args(self.loss)
        for k, v in self.addr.items():
            if k != "state_out":
                setattr(a, k, v if self.size[k] else None)
        a.workspace_bytes = self.ws
        if self.loss:
            a.grad_scale = 0.5
        for k, v in over.items():
            setattr(a, k, v)
        return a

    def run(self, a, ns=None, T=None, rows=None, row0=None, B=None, state_out="given"):
        """the one call shape of the corner, on the corner's own numbers unless given; state_out: "given", None or an address"""
        ns, T, B = self.ns if ns is None else ns, self.T if T is None else T, self.B if B is None else B
        rows, row0 = self.rows if rows is None else rows, self.row0 if row0 is None else row0
        h, a = self.p._h, ctypes.byref(a) if a is not None else None
        if not self.rec:
            return self.fn(h, a, ns, rows, row0, T, None) if self.sm else self.fn(h, a, ns, T, None)
        so = (self.addr["state_out"] if self.size["state_out"] else None) if state_out == "given" else state_out
        if not self.ring:
            return self.fn(h, a, int(self.sm), ns, rows or 0, row0, T, B, so, None)
        return self.fn(h, a, ns, rows, row0, T, B, so, None) if self.sm else self.fn(h, a, ns, T, B, so, None)


# ---- a kernel's instructions -------------------------------------------------------------------------------------------------------------
def kernel_ops(monkeypatch, cache, sexpr, resources, *args, least=20, **kw):
    """Compile the graph and resolve ONE kernel -- Program.<resources>(*args, **kw), named by the `_kernel_symbol` call of the same
    arguments -- into the empty directory `cache`: exactly one code object, which names the kernel.  (program, the resources, the
    vector mnemonics of its disassembly, all mnemonics)"""
    monkeypatch.setenv("FLOWZ_HIP_CACHE", str(cache))
    p = F.compile(F.from_sexpr(sexpr))
    r = getattr(p, resources)(*args, **kw)
    objs = glob.glob(os.path.join(str(cache), "*.hsaco"))
    assert len(objs) == 1
    dis = subprocess.check_output(["/opt/rocm/lib/llvm/bin/llvm-objdump", "-d", objs[0]], text=True)
    assert getattr(p, resources.replace("_resources", "_kernel_symbol"))(*args, **kw) in dis
    every = [ln.split()[0] for ln in dis.splitlines() if ln.strip()]
    ops = [o for o in every if o.startswith("v_")]
    assert len(ops) > least
    return p, r, ops, every


def assert_no_contraction(every, divides=True, lds=False):
    """every: all mnemonics of a kernel.  No contraction: the only fused multiply-adds are the refinement steps of the correctly
    rounded float32 division (five: v_div_scale, v_rcp, Newton steps, v_div_fmas, v_div_fixup) and square root (two after v_sqrt) --
    tanh divides, so do DIV and the SQRT adjoint; graphs without them (divides=False) hold none at all.
    lds: the kernel keeps its rings in LDS (it reads and writes it), without a barrier and without an atomic"""
    ops = [o for o in every if o.startswith("v_")]
    fused = [o for o in ops if o.startswith(("v_fma", "v_fmac"))]
    divisions, roots = ops.count("v_div_fixup_f32"), ops.count("v_sqrt_f32_e32") + ops.count("v_sqrt_f32_e64")
    assert len(fused) == 5 * divisions + 2 * roots and ops.count("v_div_fmas_f32") == divisions, (fused, divisions, roots)
    assert not [o for o in ops if re.match(r"v_(pk_(fma|mad|mac)|mad|mac)(_mix|_mixlo|_mixhi|_legacy)?_(f16|f32|f64|bf16)", o)]
    if not divides:
        assert divisions == 0 and roots == 0 and not fused
    if lds:
        assert any(o.startswith("ds_read") for o in every) and any(o.startswith("ds_write") for o in every)
        assert "s_barrier" not in every and not [o for o in every if "atomic" in o]


# ---- manifests ---------------------------------------------------------------------------------------------------------------------------
def replay(path, env_extra=None, jobs=None):
    """the counts F.manifest_build answers for a manifest in a process of its own that records nothing"""
    env = dict({k: v for k, v in os.environ.items() if k != "FLOWZ_HIP_MANIFEST"}, **(env_extra or {}))
    code = "import sys\nsys.path.insert(0, %r)\nfrom zignal_amd import flowz as F\nprint(F.manifest_build(%r%s))" % (
        ROOT, str(path), "" if jobs is None else ", %d" % jobs)
    return eval(subprocess.check_output([sys.executable, "-c", code], env=env, text=True).strip().splitlines()[-1])


def recipe_of(sexpr, typed=0):
    """the recipe (input types and expression text) of a graph, as a manifest record holds it"""
    expr, buf = F.from_sexpr(sexpr), ctypes.create_string_buffer(1 << 16)      # (the expression lives until its handle has been read)
    n = C.lib.fz_expr_recipe(expr._h, buf, 1 << 16)
    assert 0 < n < 1 << 16
    return b"typed %d\n" % typed + buf.raw[:n]


def recorded_recipe(tmp_path, module, graph, resolve):
    """the recipe of the first record a recording process (FLOWZ_HIP_MANIFEST) writes that compiles <module>.<graph> and calls the
    Program method `resolve`"""
    td = tempfile.mkdtemp(dir=str(tmp_path))
    raw = os.path.join(td, "recorded.fzm")
    code = ("import sys\nsys.path[:0] = [%r, %r]\nimport %s as M\nfrom zignal_amd import flowz as F\nF.compile(F.from_sexpr(M.%s)).%s()\n"
            % (ROOT, HERE, module, graph, resolve))
    subprocess.check_call([sys.executable, "-c", code], env=dict(os.environ, FLOWZ_HIP_MANIFEST=raw, FLOWZ_HIP_CACHE=os.path.join(td, "cache")))
    text = open(raw, "rb").read()
    eol = text.index(b"\n")
    return text[eol + 1:eol + 1 + int(text[:eol].split()[5])]


def write_manifest(path, records):
    """records: (P, U, block, flags, recipe) each, as ring_loss_graphs.manifest_variants reads them"""
    with open(path, "wb") as f:
        for P, U, block, flags, recipe in records:
            f.write(b"FZM1 %d %d %d %d %d\n" % (P, U, block, flags, len(recipe)) + recipe)


def code_objects(cache):
    return [f for f in os.listdir(cache) if f.endswith(".hsaco")]


def symbol_shape(sym, letter):
    """the numbers a kernel symbol of the family names behind `letter` (c: the checkpoint stride, u: the unroll): (n, block) of a
    time-major kernel, (n, patch rows, block) of a stream-major one"""
    m = re.search(r"_kernel_%s(\d+)(?:r(\d+))?b(\d+)_g[0-9a-f]{8}$" % letter, sym)
    assert m, sym
    return tuple(int(g) for g in m.groups() if g is not None)


# ---- the draws of the restatement tests --------------------------------------------------------------------------------------------------
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


def fd_check(p, x, s0, par, yb, sb, h=1e-6):
    """central differences of the float64 torch forward against the numpy restatement, a few coordinates of every tensor"""
    import torch

    import adjoint_ref as A
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
