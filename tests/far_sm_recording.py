"""Geometry, cases, launcher and kernels of the stream-major far recording tests (fz_run_recording_far_grad_for,
fz_run_recording_far_loss_grad_for with FZ_GRAD_STREAM_MAJOR: the backward of a whole recording whose graph has delay lines deeper
than 256 samples, on a [batch, time] tensor as it lies): the eight graphs, draws and rules of tests/far_recording_graphs.py; the rule
that chooses the far states kernel's workgroup and patch length together, restated, and the geometry include/flowz_hip.h states, by
hand; the cases; launch(), grad_harness.launch at this corner of the family; and the kernels the GPU tests launch
(tests/golden/far_sm_recording_kernels.fzm.gz)."""
import contextlib
import gzip
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

import far_recording_graphs as FRG
import far_sm_graphs as FS
import grad_harness as H
import ring_sm_recording as RS
from grad_host_harness import LDS_BYTES, symbol_shape

F32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
MANIFEST = os.path.join(HERE, "golden", "far_sm_recording_kernels.fzm.gz")
K = H.K
FARS = FRG.FARS
NAMES = sorted(FARS)
DEEPEST = FRG.DEEPEST
prog = FRG.prog
BOUNDARY_GRAPHS = ("far_comb", "far_tap1", "far_mixed")           # run with a start and a prefetched far read around a patch boundary
STRIDES = (0, 1)                                                  # checkpoint_rows the tests ask for
SWEEP_B = 64                                                      # block_rows of the stream sweep: five blocks of D + 1 rows
STREAM_MAJOR = 1                                                  # include/flowz_hip.h: FZ_GRAD_STREAM_MAJOR
ENTRY = {False: "fz_run_recording_far_grad_for", True: "fz_run_recording_far_loss_grad_for"}


# ---- the geometry rule, restated (zignal_amd/csrc/fz_grad.cpp: states_variant with far lines on stream-major buffers) ----------------------
states_unroll = RS.states_unroll
states_patch_rows = RS.states_patch_rows
lds_ring_slots = FS.lds_ring_slots


def lds_bytes(p, block, R):
    """the LDS ring lines' slots and an x-only patch: 4 block (slots + R n_in + 4); the far lines take none"""
    return RS.lds_bytes(p, block, R, lds_ring_slots(p))


def geometry(p):
    """(U, R, block) of the stream-major far states kernel, or (U, Rmin, 0) when nothing fits: the ring states kernel's rule over the
    LDS ring slots alone, with R from R0 = the plain states kernel's patch rows (HALF the ring states kernel's; never below Rmin =
    max(4, U)) halved down to Rmin; per R the block over 256, 128, 64; the first pair that fits the LDS twice, failing that once"""
    U = states_unroll(p)
    Rmin = max(4, U)
    R0 = max(states_patch_rows(p), Rmin)
    for times in (2, 1):
        R = R0
        while R >= Rmin:
            for block in (256, 128, 64):
                if times * lds_bytes(p, block, R) <= LDS_BYTES:
                    return U, R, block
            R //= 2
    return U, Rmin, 0


# name -> (LDS ring slots, input wires, U, R, block, LDS bytes): derived by hand from the formulas
TABLE = {
    "far_comb": (0, 1, 8, 32, 256, 36864),
    "far257": (0, 1, 8, 32, 256, 36864),
    "far1031": (0, 1, 8, 32, 256, 36864),
    "far_mixed": (17, 1, 8, 32, 256, 54272),                      # (twice fits: 108 544 of 163 840 bytes)
    "far_two_in": (0, 2, 8, 16, 256, 36864),
}

SYMBOL = re.compile(r"fz_states_far_sm_kernel_u(\d+)r(\d+)b(\d+)_g([0-9a-f]{8})")


def symbol_geometry(sym):
    """(U, R, block) the kernel's symbol names"""
    assert SYMBOL.fullmatch(sym), sym
    return symbol_shape(sym, "u")


# ---- shapes ------------------------------------------------------------------------------------------------------------------------------
windows = RS.windows                                              # (rows_total, row0): the whole buffer; four rows in, rows behind it


def cap(name, ns):
    return min(ns, FRG.MAX_STREAMS.get(name, ns))


def cases(name):
    """(streams, rows, block_rows, checkpoint_rows) of every bitwise case of a graph, D its deepest line: blocks far shorter than the
    line, several starts in one group, idle lanes in the second wave; a recording shorter than the line; the longest blocks shorter
    than the line, also at C = 1; blocks just longer than the line, a second workgroup; the library's B; on BOUNDARY_GRAPHS a start
    and a prefetched far read on, before and after a group and a patch boundary; the stream sweep at D + 1 rows"""
    D = DEEPEST[name]
    long_b = 4 * ((D - 1) // 4)
    out = [(65, D + 5, 4, 0), (64, D - 1, 4, 0), (65, 2 * D + 3, long_b, 0), (65, 2 * D + 3, long_b, 1),
           (cap(name, 257), 2 * D + 3, 4 * -(-D // 4) + 4, 0), (65, 2 * D + 3, 0, 0)]
    if name in BOUNDARY_GRAPHS:
        U, R, _ = geometry(prog(name))
        out += [(65, T, B, 0) for T in (1, U - 1, U + 1, R - 1, R, R + 1, 2 * R + 3) for B in (4, 0)]
    for ns in (1, 63, 64, 257):
        if (cap(name, ns), D + 1, SWEEP_B, 0) not in out:
            out.append((cap(name, ns), D + 1, SWEEP_B, 0))
    return out


inputs = FRG.inputs                                               # the time-major draw of a case at p0 = D - 3


def block_rows(name, T, B, c):
    """the B a call will use"""
    p = prog(name)
    return FRG.block_rows(name, T, c or symbol_shape(p.far_grad_kernel_symbol(), "c")[0], B)


AUTOGRAD = ("far257", 130, 300, 64)                               # autograd.mse_recording_far(stream_major=True): graph, streams, rows, block_rows


# ---- one launch through the C ABI ------------------------------------------------------------------------------------------------------
class AsPlainFamily:
    """a Program whose plain recording queries answer with the far family's: what grad_harness.launch and grad_host_harness.FakeCall
    ask of it for a recording call that takes the layout as an argument"""

    def __init__(self, p):
        self._p = p

    def __getattr__(self, key):
        return getattr(self._p, key)

    def recording_workspace_bytes(self, ns, T, B=0, c=0, stream_major=False):
        return self._p.far_recording_workspace_bytes(ns, T, B, c)

    def recording_block_rows(self, T, B=0, c=0):
        return self._p.far_recording_block_rows(T, B, c)


@contextlib.contextmanager
def far_entry_points():
    """while the block runs, the recording rows of grad_harness.ENTRY that take the layout as an argument name the far family's _for
    calls (the argument lists are the same)"""
    keys = [(False, loss, sm, True) for loss in (False, True) for sm in (False, True)]
    kept = {k: H.ENTRY[k] for k in keys}
    try:
        for k in keys:
            H.ENTRY[k] = ENTRY[k[1]]
        yield
    finally:
        H.ENTRY.update(kept)


def launch(p, d, B, loss, window=None, c=0, state_grad=True, alias=False, leave_out=(), time_major=False):
    """grad_harness.launch of fz_run_recording_far_grad_for / fz_run_recording_far_loss_grad_for with FZ_GRAD_STREAM_MAJOR on the
    time-major draw d of far_recording_graphs.inputs (x, s0, par, dL/dy or target, sb, ap, ac[, al]), in blocks of B rows (0: the
    library's choice), grad_scale = K.  window: (rows_total, row0), default windows(T)[0].  time_major: the same entry point with
    FZ_GRAD_TIME_MAJOR on the draw as it is"""
    with far_entry_points():
        return H.launch(AsPlainFamily(p), d, loss=loss, window=None if time_major else window or windows(d[0].shape[0])[0], recording=B, c=c,
                        state_grad=state_grad, alias=alias, leave_out=leave_out, k=K)


# ---- the kernels the GPU tests launch: tests/golden/far_sm_recording_kernels.fzm.gz ----------------------------------------------------
def forward_shapes(name):
    """(streams, rows) of the time-major run_block launches the GPU test chains its block-start states through, and of autograd"""
    out = set()
    for ns, T, B, c in cases(name):
        Be = block_rows(name, T, B, c)
        out |= {(ns, Be), (ns, T - (-(-T // Be) - 1) * Be)}
    if name == AUTOGRAD[0]:
        out.add(AUTOGRAD[1:3])
    return sorted(out)


def resolve():
    """what a recording process calls (FLOWZ_HIP_MANIFEST set): the far states kernels of both layouts, the far and far loss kernels of
    both layouts at the strides used, and the time-major forward kernels starts and state_out are compared with"""
    for n in NAMES:
        p = prog(n)
        for sm in (True, False):
            p.far_states_resources(stream_major=sm)
            for c in STRIDES:
                p.far_grad_resources(c, stream_major=sm)
                p.far_loss_grad_resources(c, stream_major=sm)
        for ns, rows in forward_shapes(n):
            p.build(None, ns, rows)


def record():
    """record the manifest with the library as it is; needs no GPU.  By hand: PYTHONPATH=. python tests/far_sm_recording.py"""
    from zignal_amd import flowz as F
    code = "import sys\nsys.path[:0] = [%r, %r]\nimport far_sm_recording as S\nS.resolve()\n" % (os.path.dirname(HERE), HERE)
    with tempfile.TemporaryDirectory() as td:
        raw = os.path.join(td, "manifest.fzm")
        subprocess.check_call([sys.executable, "-c", code], env=dict(os.environ, FLOWZ_HIP_MANIFEST=raw))
        with open(raw, "rb") as f, open(MANIFEST, "wb") as out:
            out.write(gzip.compress(f.read(), 9, mtime=0))
    return F.manifest_build(MANIFEST)


manifest_variants = RS.manifest_variants


if __name__ == "__main__":
    print("kernel manifest:", record())
