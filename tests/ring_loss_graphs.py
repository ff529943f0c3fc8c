"""Graphs and draws of the ring loss backward tests (fz_run_block_ring_loss_grad): the eight graphs of tests/ring_grad_graphs.py, all
with one output, and two with two outputs -- the rule's slot order shows only there; the target draw; the grad_scale of the bitwise
tests; the cases both test files share; and the kernels the GPU tests launch (tests/golden/ring_loss_kernels.fzm.gz)."""
import gzip
import os
import subprocess
import sys
import tempfile

import numpy as np

import adjoint_ref as A
import loss_grad_ref as LR
import ring_grad_graphs as RG
from graphs import DEL, IN, add, fb, lit, mul, par, param, seq

F32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
MANIFEST = os.path.join(HERE, "golden", "ring_loss_kernels.fzm.gz")
K = 0.37                                                          # grad_scale of the bitwise tests: no power of two, so e * k rounds


def two_out_ff():
    """(_1 + 0.5*_1[_12]) | _1[_9]: two inputs, two outputs, rings on two wires, no recursion"""
    return par(add(IN(1), mul(lit(0.5), DEL(1, 12))), DEL(1, 9))


def two_out_fb():
    """~(param(0)*_1[_13] + _2) |= (_1 | 0.5*_1[_10]): two outputs of one recursion through a ring, a per-stream coefficient"""
    return seq(fb(add(mul(param(0), DEL(1, 13)), IN(2))), par(IN(1), mul(lit(0.5), DEL(1, 10))))


# name -> s-expression builder: every graph of the ring loss tests
GRAPHS = dict(RG.RINGS, two_out_ff=two_out_ff, two_out_fb=two_out_fb)
# the deepest line of each
DEEPEST = dict(RG.DEEPEST, two_out_ff=12, two_out_fb=13)

_progs = {}


def prog(name):
    from zignal_amd import flowz as F
    if name not in _progs:
        _progs[name] = F.compile(F.from_sexpr(GRAPHS[name]()))
    return _progs[name]


def stride(p):
    """the default checkpoint stride of the ring kernels of p"""
    return int(p.ring_grad_kernel_symbol().split("_c")[1].split("b")[0])


def draw(p, ns, T, seed):
    """x, state, params, target, state_grad, accum_params, accum_consts, accum_loss: the draws of ring_grad_graphs.inputs with a target
    (standard normal, a seed of its own) where dL/dy was, and a loss accumulator that is not zero"""
    x, s0, par_, _, sb, ap, ac = RG.inputs(p, ns, T, seed)
    rng = np.random.default_rng(770_000 + seed)
    tg = rng.standard_normal((T, ns, p.n_out)).astype(F32)
    al = rng.standard_normal(ns).astype(F32)
    return x, s0, par_, tg, sb, ap, ac, al


def restate(p, d, k=K, state_grad=True):
    """tests/loss_grad_ref.py on a draw: dict x / state / params / consts / loss / out"""
    x, s0, par_, tg, sb, ap, ac, al = d
    return LR.loss_grad(p, x, tg, k, s0, par_, sb if state_grad else None, ap, ac, al, ref=A)


def mse_float64(p, x, tg, s0, par_):
    """float64 autograd of ((y - target) ** 2).mean() over the torch restatement of the IR: (the mean, y, dict x / state / params / consts
    of its gradients; consts per stream)"""
    import torch

    L = A.Layout(p)
    ns = x.shape[1]
    t = lambda a, shape: torch.tensor(np.asarray(a, np.float64).reshape(shape), dtype=torch.float64, requires_grad=True)   # noqa: E731
    xt, st = t(x, x.shape), t(s0, (L.n_state, ns))
    pt = t(par_ if par_ is not None else np.zeros((L.n_param, ns)), (L.n_param, ns))
    ct = t(np.repeat(L.consts.astype(np.float64)[:, None], ns, 1), (L.n_const, ns))
    y, _ = A.torch_forward(L, xt, st, pt, ct)
    mse = ((y - torch.tensor(np.asarray(tg), dtype=torch.float64)) ** 2).mean()
    grads = torch.autograd.grad(mse, (xt, st, pt, ct), allow_unused=True)
    z = lambda g, like: np.zeros(tuple(like.shape)) if g is None else g.numpy()   # noqa: E731
    return mse.item(), y.detach().numpy(), {k: z(g, like) for k, g, like in zip(("x", "state", "params", "consts"), grads, (xt, st, pt, ct))}


_cases = {}


def case(name, ns, T, seed=0):
    """a draw and the restatement's answer to it, computed once, shared by the tests and never modified"""
    key = (name, ns, T, seed)
    if key not in _cases:
        p = prog(name)
        d = draw(p, ns, T, 1000 * seed + 7 * ns + T)
        want = restate(p, d)
        for a in (*d, *want.values()):
            if a is not None:
                a.setflags(write=False)
        _cases[key] = (d, want)
    return _cases[key]


STREAMS = (1, 64, 65, 257)                                        # one lane, a full wave, the masked tail, a second workgroup at 256 lanes


def shapes(name):
    """(streams, rows) of the bitwise cases of a graph: every row count around its deepest line D and its default stride C at every
    stream count of STREAMS (the largest: tap256 at 515 rows x 257 streams)"""
    D, C = DEEPEST[name], stride(prog(name))
    return [(ns, T) for T in sorted({1, D - 1, D, D + 1, C + 1, 2 * D + 3}) for ns in STREAMS]


# ---- the kernels the GPU tests launch: tests/golden/ring_loss_kernels.fzm.gz ------------------------------------------------------------
def kernel_requests():
    """(program, checkpoint_rows) of every ring loss kernel tests/test_ring_loss_grad_gpu.py launches and
    tests/test_ring_loss_grad_host.py builds"""
    return [(prog(n), c) for n in sorted(GRAPHS) for c in (0, 1)]


# the launches of run_block and run_block_ring_grad the GPU tests compare with: (streams, rows) of run_block per graph (out and chaining)
FORWARD_SHAPES = {n: [(65, DEEPEST[n] + 1), (65, DEEPEST[n] - 2)] for n in GRAPHS}


def resolve():
    """what a recording process calls (FLOWZ_HIP_MANIFEST set): the loss kernels, the plain ring kernels and the forward kernels"""
    for p, c in kernel_requests():
        p.ring_loss_grad_resources(c)
    for n, shp in FORWARD_SHAPES.items():
        prog(n).ring_grad_resources()
        for ns, rows in shp:
            prog(n).build(None, ns, rows)


def record():
    """record the manifest with the library as it is; needs no GPU.  By hand: PYTHONPATH=. python tests/ring_loss_graphs.py"""
    from zignal_amd import flowz as F
    code = "import sys\nsys.path[:0] = [%r, %r]\nimport ring_loss_graphs as RL\nRL.resolve()\n" % (os.path.dirname(HERE), HERE)
    with tempfile.TemporaryDirectory() as td:
        raw = os.path.join(td, "manifest.fzm")
        subprocess.check_call([sys.executable, "-c", code], env=dict(os.environ, FLOWZ_HIP_MANIFEST=raw))
        with open(raw, "rb") as f, open(MANIFEST, "wb") as out:
            out.write(gzip.compress(f.read(), 9, mtime=0))
    return F.manifest_build(MANIFEST)


def manifest_variants(path=MANIFEST):
    """(P, U, block, flags, recipe) of every record of a manifest"""
    text = gzip.open(path, "rb").read()
    out, pos = [], 0
    while pos < len(text):
        eol = text.index(b"\n", pos)
        tag, P, U, block, flags, n = text[pos:eol].split()
        assert tag == b"FZM1"
        out.append((int(P), int(U), int(block), int(flags), text[eol + 1:eol + 1 + int(n)]))
        pos = eol + 1 + int(n)
    return out


if __name__ == "__main__":
    print("kernel manifest:", record())
