"""Graphs, geometry and kernels of the stream-major far backward tests (fz_run_block_far_grad_stream_major,
fz_run_block_far_loss_grad_stream_major): the eight graphs of tests/far_grad_graphs.py; the rule that chooses the workgroup and the
patch length together, restated from tests/ring_sm_graphs.py over the LDS ring slots alone (the far lines take no LDS); and the
kernels the GPU tests launch (tests/golden/far_sm_kernels.fzm.gz)."""
import contextlib
import gzip
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

import far_grad_graphs as FG
import grad_harness as H
import ring_sm_graphs as RS
from grad_harness import from_sm, to_sm, up4  # noqa: F401  (the transposition, under the names the users of this module know)
from grad_host_harness import LDS_BYTES, symbol_shape

F32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
MANIFEST = os.path.join(HERE, "golden", "far_sm_kernels.fzm.gz")

FARS = FG.FARS                                                    # the eight graphs of the far backward
DEEPEST = FG.DEEPEST
FAST = FG.FAST
STRIDES = FG.STRIDES                                              # the graphs whose bits are also taken at C = 1 and C = 32
prog = FG.prog
AUTOGRAD = ("far257", 130, 300)                                   # autograd.run_far / mse_far (stream_major=True): graph, streams, rows


# ---- the geometry rule, restated (zignal_amd/csrc/fz_grad.cpp: block_variant -- grad_sm_patch_rows / 2, ring_sm_geometry over the LDS ring slots alone)
def lds_ring_slots(p):
    """the sum of the depths of the graph's LDS ring lines (9 .. 256 samples): the time-major far kernel's configuration states it"""
    return int(re.search(r"#define FZ_RING_SLOTS (\d+)", p.far_grad_source()).group(1))


def stride(p, c=0):
    """the checkpoint stride the far kernels use for checkpoint_rows = c"""
    return c or int(re.search(r"_c(\d+)b", p.far_grad_kernel_symbol()).group(1))


def lds_bytes(p, block, R):
    return RS.lds_bytes(p, block, R, lds_ring_slots(p))


def geometry(p, c=0):
    """(C, R, block) of the stream-major far kernels, or (C, Rmin, 0) when nothing fits: ring_sm_graphs.geometry with the far kernel's C,
    the LDS ring slots alone, and R starting from HALF the ring kernels' longest patch (never below Rmin)"""
    C = stride(p, c)
    Rmin = max(4, C)
    R0 = max(RS.patch_rows(p, C) // 2, Rmin)
    for times in (2, 1):
        R = R0
        while R >= Rmin:
            for block in (256, 128, 64):
                if times * lds_bytes(p, block, R) <= LDS_BYTES:
                    return C, R, block
            R //= 2
    return C, Rmin, 0


SYMBOL = re.compile(r"fz_adjoint_far(_loss)?_sm_kernel_c(\d+)r(\d+)b(\d+)_g")


def symbol_geometry(sym):
    """(C, R, block) a stream-major far kernel's symbol names"""
    assert SYMBOL.match(sym), sym
    return symbol_shape(sym, "c")


# ---- the far corner of grad_harness.launch and grad_host_harness.FakeCall, which know the plain and the ring family only -------------------
FAR_ENTRY = {False: "fz_run_block_far_grad_stream_major", True: "fz_run_block_far_loss_grad_stream_major"}


class AsRingFamily:
    """a Program under the ring family's names: its block workspace query answers with the far family's, everything else is the
    program's own"""

    def __init__(self, p):
        self._p = p

    def __getattr__(self, key):
        return getattr(self._p, key)

    def ring_grad_workspace_bytes(self, ns, T, c=0):
        return self._p.far_grad_workspace_bytes(ns, T, c)


@contextlib.contextmanager
def far_entry_points():
    """while the block runs, the two stream-major ring rows of grad_harness.ENTRY name the far calls: launch(ring=True, window=...) and
    FakeCall(ring=True, window=...) then make the far family's stream-major call"""
    keys = {loss: (True, loss, True, False) for loss in (False, True)}
    kept = {loss: H.ENTRY[k] for loss, k in keys.items()}
    try:
        for loss, k in keys.items():
            H.ENTRY[k] = FAR_ENTRY[loss]
        yield
    finally:
        for loss, k in keys.items():
            H.ENTRY[k] = kept[loss]


# ---- the kernels the GPU tests launch: tests/golden/far_sm_kernels.fzm.gz ------------------------------------------------------------------
def kernel_requests():
    """(program, checkpoint_rows, loss) of every stream-major far kernel tests/test_far_sm_gpu.py launches"""
    out = [(prog(n), 0, loss) for n in sorted(FARS) for loss in (False, True)]
    out += [(prog(n), c, False) for n in STRIDES for c in (1, 32)]
    return out


def chain_rows(name):
    """the two window lengths of the chained test: up4(D - 2) rows, then D + 5"""
    D = DEEPEST[name]
    return up4(D - 2), D + 5


def forward_shapes(name):
    """(streams, rows) of the time-major run_block launches of the GPU tests: the state between the chained windows, the loss's `out`,
    autograd"""
    shapes = [(65, chain_rows(name)[0]), (65, DEEPEST[name] + 1)]
    return shapes + ([AUTOGRAD[1:]] if name == AUTOGRAD[0] else [])


def resolve():
    """what a recording process calls (FLOWZ_HIP_MANIFEST set): the stream-major far kernels, the time-major far kernels they are
    compared with, and the time-major forward kernels of the chained windows, the loss's `out` and autograd"""
    for p, c, loss in kernel_requests():
        (p.far_loss_grad_resources if loss else p.far_grad_resources)(c, stream_major=True)
        (p.far_loss_grad_resources if loss else p.far_grad_resources)(c)
    for n in sorted(FARS):
        for ns, rows in forward_shapes(n):
            prog(n).build(None, ns, rows)


def record_manifest():
    """record the manifest with the library as it is; needs no GPU.  build() replays every manifest under tests/golden/, so a GPU run
    finds them built.  By hand: PYTHONPATH=. python tests/far_sm_graphs.py"""
    from zignal_amd import flowz as F
    code = "import sys\nsys.path[:0] = [%r, %r]\nimport far_sm_graphs as FS\nFS.resolve()\n" % (os.path.dirname(HERE), HERE)
    with tempfile.TemporaryDirectory() as td:
        raw = os.path.join(td, "manifest.fzm")
        subprocess.check_call([sys.executable, "-c", code], env=dict(os.environ, FLOWZ_HIP_MANIFEST=raw))
        with open(raw, "rb") as f, open(MANIFEST, "wb") as out:
            out.write(gzip.compress(f.read(), 9, mtime=0))
    return F.manifest_build(MANIFEST)


manifest_variants = RS.manifest_variants


if __name__ == "__main__":                         # record the kernel manifest of the library as it is
    print("kernel manifest:", record_manifest())
