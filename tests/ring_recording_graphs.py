"""Graphs, rules and cases of the ring recording tests (fz_run_recording_ring_grad, fz_run_recording_ring_loss_grad): the ten graphs of
tests/ring_loss_graphs.py with what the block rule counts of each; the block rule and the workspace formula restated; the (streams,
rows, block_rows) triples both test files share, their draws and the restatement's answers (tests/recording_ref.py chaining
tests/adjoint_ref.py / tests/loss_grad_ref.py block by block), computed once; and the kernels
the GPU tests launch (tests/golden/ring_recording_kernels.fzm.gz)."""
import gzip
import math
import os
import subprocess
import sys
import tempfile

import numpy as np

import adjoint_ref as A
import loss_grad_ref as LR
import recording_ref as RR
import ring_grad_graphs as RG
import ring_loss_graphs as RL

F32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
MANIFEST = os.path.join(HERE, "golden", "ring_recording_kernels.fzm.gz")
K = RL.K

GRAPHS = RL.GRAPHS
DEEPEST = RL.DEEPEST
prog = RL.prog
stride = RL.stride
# name -> (n_register_state, n_ring_lines): the state floats of the lines of depth <= 8, and the lines deeper than that
COUNTS = {"fb9": (0, 1), "ff16": (0, 1), "lds_ring_comb": (0, 2), "tap256": (0, 1), "taps12_31": (0, 1), "biquad_comb17": (4, 1), "ks_tanh11": (0, 1),
          "two_in": (0, 2), "two_out_ff": (0, 2), "two_out_fb": (0, 2)}


def ring_rows(p):
    """the state rows of the lines deeper than 8 samples: [(first row, depth)]"""
    return [(r0, d) for _, d, r0 in A.Layout(p).lines if d > 8]


# ---- the two rules, restated ---------------------------------------------------------------------------------------------------------
def block_rows(T, C, n_state, n_reg, n_rl, B=0):
    """the rows per block: B, at most T; B = 0: the least b with b^2 (n_reg + C n_rl) >= T n_state C, rounded up to a multiple of
    max(4, C), and T when that is not smaller.  Without a ring line: recording_ref.block_rows"""
    if not n_rl:
        return RR.block_rows(T, C, B)
    if B:
        return min(B, T)
    den, num = n_reg + C * n_rl, T * n_state * C
    b = math.isqrt(-(-num // den))                                 # (integers throughout: b^2 den >= num  <=>  b^2 >= ceil(num / den))
    while b * b * den < num:
        b += 1
    m = max(4, C)
    b = (b + m - 1) // m * m
    return b if b < T else T


def rows_kept(T, B, C, n_state, n_reg, n_rl):
    """the [n_streams] rows of workspace: the block starts, one block's checkpoints, one block's tape"""
    return -(-T // B) * n_state + -(-B // C) * n_reg + B * n_rl if T else 0


def workspace_bytes(ns, T, B, C, n_state, n_reg, n_rl):
    return rows_kept(T, B, C, n_state, n_reg, n_rl) * ns * 4


# ---- shapes, draws and the restatement's answers ---------------------------------------------------------------------------------------
def triples(name):
    """(streams, rows, block_rows) of the bitwise cases of a graph, D its deepest line: blocks far shorter than the line at the stream counts
    around a wave and a workgroup (several block starts inside one unrolled group, a short last block); a recording shorter than the line; B
    just below D; B above D; the default B.  The largest: tap256 at 515 rows x 257 streams"""
    D = DEEPEST[name]
    return [(ns, D + 5, 4) for ns in RL.STREAMS] + [(64, D - 1, 4), below_depth(name), (257, 2 * D + 3, 4 * -(-D // 4) + 4), (65, 2 * D + 3, 0)]


def below_depth(name):
    """the triple whose B is just below D (also run at checkpoint_rows 1)"""
    D = DEEPEST[name]
    return (65, 2 * D + 3, 4 * ((D - 1) // 4))


def draw(p, ns, T, seed):
    """x, state, params, out_grad, target, state_grad, accum_params, accum_consts, accum_loss: the draws of ring_grad_graphs.inputs and of
    ring_loss_graphs.draw (the same x, state and accumulators for the plain call and the loss call)"""
    x, s0, par, yb, sb, ap, ac = RG.inputs(p, ns, T, seed)
    _, _, _, tg, _, _, _, al = RL.draw(p, ns, T, seed)
    return x, s0, par, yb, tg, sb, ap, ac, al


_draws, _wants = {}, {}


def case(name, ns, T):
    """the draw of a shape, computed once and never modified"""
    key = (name, ns, T)
    if key not in _draws:
        d = draw(prog(name), ns, T, 31 * ns + T)
        for a in d:
            if a is not None:
                a.setflags(write=False)
        _draws[key] = d
    return _draws[key]


def chained(p, d, B, loss, state_grad=True, zero_accum=False):
    """tests/recording_ref.py on a draw, block by block with blocks of B rows (B >= 1)"""
    x, s0, par, yb, tg, sb, ap, ac, al = d
    if zero_accum:
        ap, ac, al = np.zeros_like(ap), np.zeros_like(ac), np.zeros_like(al)
    kw = dict(state=s0, params=par, state_grad=sb if state_grad else None, accum_params=ap, accum_consts=ac, ref=A)
    return RR.grad(p, x, B, target=tg, k=K, accum_loss=al, **kw) if loss else RR.grad(p, x, B, out_grad=yb, **kw)


def single(p, d, loss):
    """the single restated call over all rows"""
    x, s0, par, yb, tg, sb, ap, ac, al = d
    return LR.loss_grad(p, x, tg, K, s0, par, sb, ap, ac, al, ref=A) if loss else A.grad(p, x, yb, s0, par, sb, ap, ac)


def want(name, ns, T, B, loss, c=0):
    """the restatement's answer to a triple (B = 0: the library's default at checkpoint stride c), computed once, read-only"""
    p = prog(name)
    Be = block_rows(T, c or stride(p), p.n_state, *COUNTS[name], B)
    key = (name, ns, T, Be, loss)
    if key not in _wants:
        r = chained(p, case(name, ns, T), Be, loss)
        for a in r.values():
            if a is not None:
                a.setflags(write=False)
        _wants[key] = r
    return _wants[key]


# ---- the kernels the GPU tests launch: tests/golden/ring_recording_kernels.fzm.gz ------------------------------------------------------
def forward_shapes(name):
    """(streams, rows) of the run_block launch state_out is compared with, once per graph"""
    return [(65, DEEPEST[name] + 5)]


def resolve():
    """what a recording process calls (FLOWZ_HIP_MANIFEST set): the ring states kernels, the ring and ring loss kernels at C in (0, 1), and
    the forward kernels compared with"""
    for n in sorted(GRAPHS):
        p = prog(n)
        p.ring_states_resources()
        for c in (0, 1):
            p.ring_grad_resources(c)
            p.ring_loss_grad_resources(c)
        for ns, rows in forward_shapes(n):
            p.build(None, ns, rows)


def record():
    """record the manifest with the library as it is; needs no GPU.  By hand: PYTHONPATH=. python tests/ring_recording_graphs.py"""
    from zignal_amd import flowz as F
    code = "import sys\nsys.path[:0] = [%r, %r]\nimport ring_recording_graphs as R\nR.resolve()\n" % (os.path.dirname(HERE), HERE)
    with tempfile.TemporaryDirectory() as td:
        raw = os.path.join(td, "manifest.fzm")
        subprocess.check_call([sys.executable, "-c", code], env=dict(os.environ, FLOWZ_HIP_MANIFEST=raw))
        with open(raw, "rb") as f, open(MANIFEST, "wb") as out:
            out.write(gzip.compress(f.read(), 9, mtime=0))
    return F.manifest_build(MANIFEST)


if __name__ == "__main__":
    print("kernel manifest:", record())
