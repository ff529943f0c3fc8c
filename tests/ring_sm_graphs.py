"""Graphs, geometry and kernels of the stream-major ring backward tests (fz_run_block_ring_grad_stream_major,
fz_run_block_ring_loss_grad_stream_major): the graphs are those of tests/ring_grad_graphs.py and tests/ring_loss_graphs.py; the rule
that chooses the workgroup and the patch length together, restated; the graph whose rings plus the shortest patch fit no workgroup;
the transposition helpers; and the kernels the GPU tests launch (tests/golden/ring_sm_kernels.fzm.gz)."""
import gzip
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

import ring_grad_graphs as RG
import ring_loss_graphs as RL
from grad_harness import from_sm, to_sm, up4  # noqa: F401  (the transposition, under the names the users of this module know)
from grad_host_harness import LDS_BYTES, symbol_shape
from graphs import DEL, add

F32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
MANIFEST = os.path.join(HERE, "golden", "ring_sm_kernels.fzm.gz")

RINGS = RG.RINGS                                                  # the eight graphs of the plain backward
GRAPHS = RL.GRAPHS                                                # the ten of the loss: those and two with two outputs
DEEPEST = RL.DEEPEST
prog = RL.prog
STRIDES = (0, 1, 4)                                               # checkpoint_rows the tests ask for: the default, and two others
AUTOGRAD_GRAPHS = ("lds_ring_comb", "two_in")                     # autograd.run_rings / mse_rings (stream_major=True): 130 streams, up4(2 D + 3) rows
STRIDE_GRAPHS = ("lds_ring_comb", "biquad_comb17", "tap256")      # the graphs the GPU tests launch at every stride of STRIDES


def three_wires_612():
    """three input wires read 256, 256 and 100 samples back: 612 samples of ring, 156 672 bytes per 64 lanes.  The time-major ring
    backward takes it (one workgroup of 64 lanes).  Default C = 8 (6 saved floats per row: 3 frames, 3 ring reads); the shortest patch,
    R = 8 rows of 4 wires + 4 floats, makes 4 * 64 * (612 + 32 + 4) = 165 888 bytes: refused.  checkpoint_rows = 4: R = 4,
    4 * 64 * (612 + 16 + 4) = 161 792 bytes: taken."""
    return add(add(DEL(1, 256), DEL(2, 256)), DEL(3, 100))


# ---- the geometry rule, restated (zignal_amd/csrc/fz_grad.cpp: grad_sm_patch_rows, ring_sm_geometry) ----------------------------------
def ring_slots(p):
    """the sum of the depths of the graph's ring lines: the time-major ring kernel's configuration states it"""
    m = re.search(r"#define FZ_RING_SLOTS (\d+)", p.ring_grad_source())
    return int(m.group(1)) if m else 0


def ring_stride(p, c=0):
    """the checkpoint stride the ring kernels use for checkpoint_rows = c"""
    return c or int(re.search(r"_c(\d+)b", p.ring_grad_kernel_symbol()).group(1))


def lds_bytes(p, block, R, slots=None):
    slots = ring_slots(p) if slots is None else slots
    return 4 * block * (slots + R * (p.n_in + p.n_out) + 4)


def patch_rows(p, C):
    """R0: the patch rows of the stream-major adjoint kernel of a graph with these wires at stride C"""
    wide = max(p.n_in, p.n_out, 1)
    narrow = max(min(p.n_in, p.n_out) if p.n_in and p.n_out else wide, 1)
    R = 4
    while R * wide < 32:
        R *= 2
    while R * narrow < 32 and (2 * R * (p.n_in + p.n_out) + 4) * 4 * 256 <= LDS_BYTES // 2:
        R *= 2
    return max(R, C)


def geometry(p, c=0):
    """(C, R, block) of the stream-major ring kernels, or (C, Rmin, 0) when nothing fits: R from R0 halved down to max(4, C), block from
    256, 128, 64; the first pair that fits the LDS twice, failing that the first that fits once"""
    C, slots = ring_stride(p, c), ring_slots(p)
    R0, Rmin = patch_rows(p, C), max(4, C)
    for times in (2, 1):
        R = R0
        while R >= Rmin:
            for block in (256, 128, 64):
                if times * lds_bytes(p, block, R, slots) <= LDS_BYTES:
                    return C, R, block
            R //= 2
    return C, Rmin, 0


SYMBOL = re.compile(r"fz_adjoint_ring(_loss)?_sm_kernel_c(\d+)r(\d+)b(\d+)_g")


def symbol_geometry(sym):
    """(C, R, block) a stream-major ring kernel's symbol names"""
    assert SYMBOL.match(sym), sym
    return symbol_shape(sym, "c")


# ---- the kernels the GPU tests launch: tests/golden/ring_sm_kernels.fzm.gz ---------------------------------------------------------------
def kernel_requests():
    """(program, checkpoint_rows, loss) of every stream-major ring kernel tests/test_ring_sm_gpu.py launches"""
    req = []
    for loss, names in ((False, RINGS), (True, GRAPHS)):
        for n in sorted(names):
            for c in (STRIDES if n in STRIDE_GRAPHS else (0,)):
                req.append((prog(n), c, loss))
    return req


def chain_rows(name):
    """the two window lengths of the chained test: up4(D - 2) rows, then D + 5"""
    D = DEEPEST[name]
    return up4(D - 2), D + 5


def resolve():
    """what a recording process calls (FLOWZ_HIP_MANIFEST set): the stream-major ring kernels, the time-major ring kernels they are
    compared with, and the stream-major forward kernels of the chained windows and of autograd"""
    from zignal_amd import flowz as F
    for p, c, loss in kernel_requests():
        (p.ring_loss_grad_resources if loss else p.ring_grad_resources)(c, stream_major=True)
    for n in sorted(GRAPHS):
        p = prog(n)
        p.ring_loss_grad_resources()
        if n in RINGS:
            p.ring_grad_resources()
            T1, T2 = chain_rows(n)
            p.build(F.make_variant(0, 0, 0, F.C.FZ_VF_STREAM_MAJOR), 65, T1)
    for n in AUTOGRAD_GRAPHS:
        prog(n).build(F.make_variant(0, 0, 0, F.C.FZ_VF_STREAM_MAJOR), 130, up4(2 * DEEPEST[n] + 3))


def record():
    """record the manifest with the library as it is; needs no GPU.  By hand: PYTHONPATH=. python tests/ring_sm_graphs.py"""
    from zignal_amd import flowz as F
    code = "import sys\nsys.path[:0] = [%r, %r]\nimport ring_sm_graphs as RS\nRS.resolve()\n" % (os.path.dirname(HERE), HERE)
    with tempfile.TemporaryDirectory() as td:
        raw = os.path.join(td, "manifest.fzm")
        subprocess.check_call([sys.executable, "-c", code], env=dict(os.environ, FLOWZ_HIP_MANIFEST=raw))
        with open(raw, "rb") as f, open(MANIFEST, "wb") as out:
            out.write(gzip.compress(f.read(), 9, mtime=0))
    return F.manifest_build(MANIFEST)


manifest_variants = RL.manifest_variants


if __name__ == "__main__":
    print("kernel manifest:", record())
