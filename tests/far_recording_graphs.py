"""Graphs, rules and shapes of the far recording tests (fz_run_recording_far_grad, fz_run_recording_far_loss_grad: the backward of a
whole recording whose graph has delay lines deeper than 256 samples): the eight graphs of far_grad_graphs.FARS with what the two
rules count of each; the rule for the rows per block and the rule for the workspace, restated from include/flowz_hip.h; the shapes
both test files run; the kernels the GPU tests launch (tests/golden/far_recording_kernels.fzm.gz)."""
import gzip
import os
import subprocess
import sys
import tempfile

import far_grad_graphs as FG

HERE = os.path.dirname(os.path.abspath(__file__))
MANIFEST = os.path.join(HERE, "golden", "far_recording_kernels.fzm.gz")

FARS = FG.FARS
DEEPEST = FG.DEEPEST
# name -> (n_register_state, n_ring_lines, n_far_lines, the far depths): the state floats of the lines of depth <= 8, the lines of depth
# 9 .. 256 (LDS rings), the lines deeper than that (rings in HBM)
COUNTS = {
    "far257": (0, 0, 1, (257,)),
    "far_comb": (0, 0, 1, (300,)),
    "far_tap1": (0, 0, 1, (300,)),          # three reads of one line
    "far_taps": (0, 0, 1, (400,)),          # two reads of one line
    "far_adjacent": (0, 0, 1, (301,)),
    "far_mixed": (4, 1, 1, (260,)),         # df1's two lines and two more of depth 1; the 17-sample ring; the 260-sample far line
    "far_two_in": (0, 0, 2, (280, 257)),
    "far1031": (0, 0, 1, (1031,)),
}
MAX_STREAMS = {"far1031": 65}               # (the restatement keeps the state before every row of a block: 1032 rows of state per row)
STREAM_SWEEP = ("far_comb", "far_tap1", "far_mixed")

prog = FG.prog


def n_state(name):
    """every line's rows and one phase row per far line"""
    return sum(d for _, d in prog(name).lines()) + len(COUNTS[name][3])


# ---- the two rules, restated (include/flowz_hip.h: fz_run_recording_far_grad) -------------------------------------------------------------
def block_rows(name, T, C, B=0):
    """B: block_rows capped at T; for 0 the least B with B^2 (n_register_state + C (n_ring_lines + n_far_lines)) >= T n_state C, rounded
    up to a multiple of max(4, C), and T when that is not smaller"""
    if B:
        return min(B, T)
    n_reg, n_rl, n_fl, _ = COUNTS[name]
    den, num, m = n_reg + C * (n_rl + n_fl), T * n_state(name) * C, max(4, C)
    b = 0
    while b * b * den < num:                                       # (integers throughout: no square root to round)
        b += 1
    b = (b + m - 1) // m * m
    return b if b < T else T


def rows_kept(name, T, B, C):
    """the rows kept per stream: the block-start states, one block's checkpoints and tape, the adjoint ring"""
    n_reg, n_rl, n_fl, depths = COUNTS[name]
    return -(-T // B) * n_state(name) + -(-B // C) * n_reg + B * (n_rl + n_fl) + sum(depths)


def workspace_bytes(name, ns, T, C, B=0):
    return rows_kept(name, T, block_rows(name, T, C, B), C) * ns * 4 if T else 0


# ---- the shapes ---------------------------------------------------------------------------------------------------------------------------
def shapes(name):
    """(streams, rows, block_rows, checkpoint_rows) of every case of a graph; D its deepest line.  Blocks far shorter than the line with
    several starts inside one unrolled group and a short last block; a recording shorter than the line; the longest blocks shorter than
    the line (also at C = 1); blocks just longer than the line, a second workgroup; the library's B; the stream sweep"""
    D = DEEPEST[name]
    cap = lambda ns: min(ns, MAX_STREAMS.get(name, ns))           # noqa: E731
    out = [(65, D + 5, 4, 0), (64, D - 1, 4, 0), (65, 2 * D + 3, 4 * ((D - 1) // 4), 0), (65, 2 * D + 3, 4 * ((D - 1) // 4), 1),
           (cap(257), 2 * D + 3, 4 * -(-D // 4) + 4, 0), (65, 2 * D + 3, 0, 0)]
    if name in STREAM_SWEEP:
        out += [(ns, D + 5, 4, 0) for ns in (1, 64, 257)]
    return out


def p0_of(name):
    """the phase every case starts from: the ring wraps inside a block"""
    return DEEPEST[name] - 3


def inputs(name, ns, T, loss=False):
    """far_grad_graphs.inputs at the case's own seed and p0 = D - 3; under the loss an eighth array, the loss accumulator"""
    import numpy as np
    d = FG.inputs(prog(name), ns, T, 11 * ns + T, p0=p0_of(name))
    if loss:
        d = d + (np.random.default_rng(ns + T).standard_normal(ns).astype(np.float32),)
    return d


# ---- the kernels the GPU tests launch: tests/golden/far_recording_kernels.fzm.gz ----------------------------------------------------------
def kernel_requests():
    """(program, checkpoint_rows, loss) of every far adjoint kernel test_far_recording_gpu.py launches: the default stride and C = 1"""
    return [(prog(n), c, loss) for n in sorted(FARS) for c in (0, 1) for loss in (False, True)]


def forward_shapes(name):
    """(streams, rows) of the run_block launches the GPU test chains its block-start states through: every block length of every shape"""
    p, out = prog(name), set()
    for ns, T, B, c in shapes(name):
        Be = p.far_recording_block_rows(T, B, c)
        out |= {(ns, Be), (ns, T - (-(-T // Be) - 1) * Be)}
    return sorted(out)


def resolve():
    """what a recording process calls (FLOWZ_HIP_MANIFEST set): the far states kernels, every kernel of kernel_requests(), the forward
    kernels, and what the autograd test and examples/fit_echo_feedback_recording.py launch"""
    for n in sorted(FARS):
        prog(n).far_states_resources()
    for p, c, loss in kernel_requests():
        (p.far_loss_grad_resources if loss else p.far_grad_resources)(c)
    for n in sorted(FARS):
        for ns, rows in forward_shapes(n):
            prog(n).build(None, ns, rows)


def record_manifest():
    """record the manifest with the library as it is; needs no GPU.  build() replays every manifest under tests/golden/, so a GPU run
    finds them built.  By hand: PYTHONPATH=. python tests/far_recording_graphs.py"""
    from zignal_amd import flowz as F
    code = "import sys\nsys.path[:0] = [%r, %r]\nimport far_recording_graphs as FRG\nFRG.resolve()\n" % (os.path.dirname(HERE), HERE)
    with tempfile.TemporaryDirectory() as td:
        raw = os.path.join(td, "manifest.fzm")
        subprocess.check_call([sys.executable, "-c", code], env=dict(os.environ, FLOWZ_HIP_MANIFEST=raw))
        with open(raw, "rb") as f, open(MANIFEST, "wb") as out:
            out.write(gzip.compress(f.read(), 9, mtime=0))
    return F.manifest_build(MANIFEST)


if __name__ == "__main__":                         # record the kernel manifest of the library as it is
    print("kernel manifest:", record_manifest())
