"""Graphs of the far backward tests (fz_run_block_far_grad): delay lines deeper than 256 samples, whose rings live in HBM -- one graph
per class of thing the kernel does with such a line; where the lines' slots and phases lie in the state rows; the inputs both test
files draw; and the kernels the GPU tests launch (tests/golden/far_grad_kernels.fzm.gz)."""
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
MANIFEST = os.path.join(HERE, "golden", "far_grad_kernels.fzm.gz")


def far257():
    """~(0.7*_1[_257] + _2): the smallest far line, in a feedback; the fast path"""
    return fb(add(mul(lit(0.7), DEL(1, 257)), IN(2)))


def far_tap1():
    """~(0.4*_1[_300] + 0.3*_1[_1] + 0.2*_1[_20] + _2): reads younger than a chunk; the per-row path"""
    return fb(add(add(add(mul(lit(0.4), DEL(1, 300)), mul(lit(0.3), DEL(1, 1))), mul(lit(0.2), DEL(1, 20))), IN(2)))


def far_taps():
    """_1 + 0.5*_1[_270] - 0.25*_1[_400]: two reads of one line on an input wire, no recursion"""
    return sub(add(IN(1), mul(lit(0.5), DEL(1, 270))), mul(lit(0.25), DEL(1, 400)))


def far_adjacent():
    """~(tanh(0.5*(_1[_301] + _1[_300])) + _2): reads one apart (the per-row path), values under a nonlinear adjoint"""
    return fb(add(fn("tanh", mul(lit(0.5), add(DEL(1, 301), DEL(1, 300)))), IN(2)))


def far_mixed():
    """df1 |= uniform(0, 0.8)*_1 |= ~(param(0)*_1[_17] + _2) |= ~(param(1)*_1[_260] + _2): register lines, an LDS ring and a far line in
    one kernel; param_grad and const_grad"""
    return seq(G.df1(), mul(uniform(0, 0.8), IN(1)), fb(add(mul(param(0), DEL(1, 17)), IN(2))), fb(add(mul(param(1), DEL(1, 260)), IN(2))))


def far_two_in():
    """_1[_280]*_2 + _2[_257]: far lines on two wires under a product"""
    return add(mul(DEL(1, 280), IN(2)), DEL(2, 257))


def far1031():
    """~(0.6*_1[_1031] + _2): a prime depth beyond a power of two"""
    return fb(add(mul(lit(0.6), DEL(1, 1031)), IN(2)))


# name -> s-expression builder: every graph the far backward must take beyond ring_grad_graphs.RINGS and grad_graphs.SUPPORTED
FARS = {
    "far257": far257,
    "far_comb": G.far_comb,
    "far_tap1": far_tap1,
    "far_taps": far_taps,
    "far_adjacent": far_adjacent,
    "far_mixed": far_mixed,
    "far_two_in": far_two_in,
    "far1031": far1031,
}
# the deepest line of each
DEEPEST = {"far257": 257, "far_comb": 300, "far_tap1": 300, "far_taps": 400, "far_adjacent": 301, "far_mixed": 260, "far_two_in": 280, "far1031": 1031}
# the path the static rule picks at the default stride (include/flowz_hip.h: STATIC RULE 2 of fz_run_block_far_grad)
FAST = {"far257": True, "far_comb": True, "far_tap1": False, "far_taps": True, "far_adjacent": False, "far_mixed": True, "far_two_in": True, "far1031": True}
MAX_STREAMS, MAX_ROWS = 65, 1032                 # of far1031: adjoint_ref keeps the state before every row, T x n_state x n_streams floats


def far_rows(p):
    """(first state row, depth, phase row) of every far line, in line order: the phase rows follow all line rows"""
    lines = p.lines()
    total, out, r = sum(d for _, d in lines), [], 0
    for _, d in lines:
        if d > 256:
            out.append((r, d, total + len(out)))
        r += d
    return out


def inputs(p, ns, T, seed, p0=0):
    """x, state, params, out_grad, state_grad, accum_params, accum_consts (float32, random; the recursions of FARS stay stable).  Every far
    line's phase row of `state` holds p0 (modulo its depth); the phase rows of state_grad hold noise, which must not matter"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((T, ns, p.n_in)) * 0.5).astype(F32)
    s0 = (rng.standard_normal((p.n_state, ns)) * 0.1).astype(F32)
    for _, d, pr in far_rows(p):
        s0[pr] = F32(p0 % d)
    par = rng.uniform(0.3, 0.8, (p.n_param, ns)).astype(F32) if p.n_param else None
    yb = rng.standard_normal((T, ns, p.n_out)).astype(F32)
    sb = rng.standard_normal((p.n_state, ns)).astype(F32)
    ap = rng.standard_normal((p.n_param, ns)).astype(F32)
    ac = rng.standard_normal((p.n_const, ns)).astype(F32)
    return x, s0, par, yb, sb, ap, ac


# ---- the kernels the GPU tests launch: tests/golden/far_grad_kernels.fzm.gz --------------------------------------------------------------
_progs = {}
STRIDES = ("far_comb", "far_tap1", "far_mixed")   # the graphs whose bits are also taken at C = 1 and C = 32


def prog(name):
    from zignal_amd import flowz as F
    if name not in _progs:
        _progs[name] = F.compile(F.from_sexpr(FARS[name]()))
    return _progs[name]


def kernel_requests():
    """(program, checkpoint_rows, loss) of every far kernel test_far_grad_gpu.py launches"""
    out = [(prog(n), 0, loss) for n in sorted(FARS) for loss in (False, True)]
    out += [(prog(n), c, False) for n in STRIDES for c in (1, 32)]
    return out


# the forward launches of test_far_grad_gpu.py: (streams, rows) of run_block per graph (chaining: D - 2 rows; the loss's `out`: D + 1;
# autograd: far257)
FORWARD_SHAPES = {n: [(65, DEEPEST[n] - 2), (65, DEEPEST[n] + 1)] for n in FARS}
FORWARD_SHAPES["far257"] = FORWARD_SHAPES["far257"] + [(130, 300)]


def resolve():
    """what a recording process calls (FLOWZ_HIP_MANIFEST set): every kernel of kernel_requests() and the forward kernels the chaining,
    loss and autograd tests launch"""
    for p, c, loss in kernel_requests():
        (p.far_loss_grad_resources if loss else p.far_grad_resources)(c)
    for n, shapes in FORWARD_SHAPES.items():
        c = int(prog(n).far_grad_kernel_symbol().split("_c")[1].split("b")[0])
        for ns, rows in shapes + [(65, c + 1)]:                   # (the loss test's shortest block: C + 1 rows)
            prog(n).build(None, ns, rows)


def record_manifest():
    """record the manifest with the library as it is; needs no GPU.  build() replays every manifest under tests/golden/, so a GPU run
    finds them built.  By hand: PYTHONPATH=. python tests/far_grad_graphs.py"""
    from zignal_amd import flowz as F
    code = "import sys\nsys.path[:0] = [%r, %r]\nimport far_grad_graphs as FG\nFG.resolve()\n" % (os.path.dirname(HERE), HERE)
    with tempfile.TemporaryDirectory() as td:
        raw = os.path.join(td, "manifest.fzm")
        subprocess.check_call([sys.executable, "-c", code], env=dict(os.environ, FLOWZ_HIP_MANIFEST=raw))
        with open(raw, "rb") as f, open(MANIFEST, "wb") as out:
            out.write(gzip.compress(f.read(), 9, mtime=0))
    return F.manifest_build(MANIFEST)


if __name__ == "__main__":                         # record the kernel manifest of the library as it is
    print("kernel manifest:", record_manifest())
