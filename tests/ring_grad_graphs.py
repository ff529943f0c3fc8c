"""Graphs of the ring backward tests (fz_run_block_ring_grad): delay lines deeper than 8 samples, one graph per class of thing the
kernel does with them; the graph it refuses; the inputs both test files draw; and the kernels the GPU tests launch
(tests/golden/ring_grad_kernels.fzm.gz)."""
import gzip
import os
import subprocess
import sys
import tempfile

import numpy as np

import graphs as G
from graphs import DEL, IN, add, fb, fn, lit, mul, param, seq, sub, uniform

F32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
MANIFEST = os.path.join(HERE, "golden", "ring_grad_kernels.fzm.gz")


def fb9():
    """~(0.7*_1[_9] + _2): the smallest ring, 9 slots, in a feedback"""
    return fb(add(mul(lit(0.7), DEL(1, 9)), IN(2)))


def ff16():
    """_1 + 0.5*_1[_16]: a power-of-two ring on an input wire, no recursion"""
    return add(IN(1), mul(lit(0.5), DEL(1, 16)))


def tap256():
    """~(0.4*_1[_256] + 0.3*_1[_1] + _2): the deepest ring, and a read at delay 1 of a deep line"""
    return fb(add(add(mul(lit(0.4), DEL(1, 256)), mul(lit(0.3), DEL(1, 1))), IN(2)))


def taps12_31():
    """_1 + 0.5*_1[_12] - 0.25*_1[_31]: two reads of one line, whose other state rows nobody reads"""
    return sub(add(IN(1), mul(lit(0.5), DEL(1, 12))), mul(lit(0.25), DEL(1, 31)))


def biquad_comb17():
    """df1 |= 0.8 (a uniform) * _1 |= ~(param(0)*_1[_17] + _2): register lines and a ring in one kernel, param_grad and const_grad"""
    return seq(G.df1(), mul(uniform(0, 0.8), IN(1)), fb(add(mul(param(0), DEL(1, 17)), IN(2))))


def ks_tanh11():
    """~(tanh(0.5*(_1[_11] + _1[_10])) + _2), a plucked string's averaging loop through a saturator: ring values a nonlinear adjoint needs"""
    return fb(add(fn("tanh", mul(lit(0.5), add(DEL(1, 11), DEL(1, 10)))), IN(2)))


def two_in():
    """two wires, _1[_20]*_2 + _2[_9]: a product with a ring read, rings on two wires"""
    return add(mul(DEL(1, 20), IN(2)), DEL(2, 9))


def six_lines_256():
    """six input wires, each read 256 samples back: 1536 samples of adjoint ring per lane, 393 216 bytes per 64 lanes -- no workgroup fits"""
    e = DEL(1, 256)
    for w in range(2, 7):
        e = add(e, DEL(w, 256))
    return e


# name -> s-expression builder: every graph the ring backward must take beyond grad_graphs.SUPPORTED
RINGS = {
    "fb9": fb9,
    "ff16": ff16,
    "lds_ring_comb": G.lds_ring_comb,
    "tap256": tap256,
    "taps12_31": taps12_31,
    "biquad_comb17": biquad_comb17,
    "ks_tanh11": ks_tanh11,
    "two_in": two_in,
}
# the deepest line of each
DEEPEST = {"fb9": 9, "ff16": 16, "lds_ring_comb": 40, "tap256": 256, "taps12_31": 31, "biquad_comb17": 17, "ks_tanh11": 11, "two_in": 20}


def inputs(p, ns, T, seed):
    """x, state, params, out_grad, state_grad, accum_params, accum_consts (float32, random; the recursions of RINGS stay stable)"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((T, ns, p.n_in)) * 0.5).astype(F32)
    s0 = (rng.standard_normal((p.n_state, ns)) * 0.1).astype(F32)
    par = rng.uniform(0.3, 0.8, (p.n_param, ns)).astype(F32) if p.n_param else None
    yb = rng.standard_normal((T, ns, p.n_out)).astype(F32)
    sb = rng.standard_normal((p.n_state, ns)).astype(F32)
    ap = rng.standard_normal((p.n_param, ns)).astype(F32)
    ac = rng.standard_normal((p.n_const, ns)).astype(F32)
    return x, s0, par, yb, sb, ap, ac


# ---- the kernels the GPU tests launch: tests/golden/ring_grad_kernels.fzm.gz -------------------------------------------------------------
_progs = {}


def prog(name):
    from zignal_amd import flowz as F
    if name not in _progs:
        _progs[name] = F.compile(F.from_sexpr(RINGS[name]()))
    return _progs[name]


def kernel_requests():
    """(program, checkpoint_rows) of every ring kernel test_ring_grad_gpu.py launches"""
    out = [(prog(n), 0) for n in sorted(RINGS)]
    out += [(prog(n), c) for n in ("lds_ring_comb", "biquad_comb17") for c in (1, 32)]
    return out


# the forward launches of test_ring_grad_gpu.py: (streams, rows) of run_block per graph (chaining: D - 2 rows; autograd: fb9)
FORWARD_SHAPES = {n: [(65, DEEPEST[n] - 2)] for n in RINGS}
FORWARD_SHAPES["fb9"] = FORWARD_SHAPES["fb9"] + [(130, 30)]


def resolve():
    """what a recording process calls (FLOWZ_HIP_MANIFEST set): every kernel of kernel_requests() and the forward kernels the chaining
    and autograd tests launch"""
    for p, c in kernel_requests():
        p.ring_grad_resources(c)
    for n, shapes in FORWARD_SHAPES.items():
        for ns, rows in shapes:
            prog(n).build(None, ns, rows)


def record_manifest():
    """record the manifest with the library as it is; needs no GPU.  build() replays every manifest under tests/golden/, so a GPU run
    finds them built.  By hand: PYTHONPATH=. python tests/ring_grad_graphs.py"""
    from zignal_amd import flowz as F
    code = "import sys\nsys.path[:0] = [%r, %r]\nimport ring_grad_graphs as RG\nRG.resolve()\n" % (os.path.dirname(HERE), HERE)
    with tempfile.TemporaryDirectory() as td:
        raw = os.path.join(td, "manifest.fzm")
        subprocess.check_call([sys.executable, "-c", code], env=dict(os.environ, FLOWZ_HIP_MANIFEST=raw))
        with open(raw, "rb") as f, open(MANIFEST, "wb") as out:
            out.write(gzip.compress(f.read(), 9, mtime=0))
    return F.manifest_build(MANIFEST)


if __name__ == "__main__":                         # record the kernel manifest of the library as it is
    print("kernel manifest:", record_manifest())
