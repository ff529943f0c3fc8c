"""Geometry, cases, launcher and kernels of the stream-major ring recording tests (fz_run_recording_ring_grad_stream_major,
fz_run_recording_ring_loss_grad_stream_major): the graphs, triples, draws and restated answers are those of
tests/ring_recording_graphs.py; the rule that chooses the states kernel's workgroup and patch length together, restated; the windows
and the patch-boundary cases; launch(), grad_harness.launch on the draws of this family; and the kernels the GPU tests launch
(tests/golden/ring_sm_recording_kernels.fzm.gz)."""
import gzip
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

import grad_harness as H
import ring_recording_graphs as R
import ring_sm_graphs as RS
from grad_host_harness import LDS_BYTES, symbol_shape

F32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
MANIFEST = os.path.join(HERE, "golden", "ring_sm_recording_kernels.fzm.gz")
K = R.K
GRAPHS = R.GRAPHS
DEEPEST = R.DEEPEST
prog = R.prog
BOUNDARY_GRAPHS = ("lds_ring_comb", "tap256", "biquad_comb17")    # the graphs run with block starts around a patch boundary
STRIDES = (0, 1)                                                  # checkpoint_rows the tests ask for


# ---- the geometry rule, restated (zignal_amd/csrc/fz_grad.cpp: states_unroll, states_sm_patch_rows, ring_sm_geometry for states_variant)
def states_unroll(p):
    """U: 8 rows per unrolled group, halved while a group's frames pass 16 floats"""
    U = 8
    while U > 1 and U * p.n_in > 16:
        U //= 2
    return U


def states_patch_rows(p):
    """the patch rows of the plain stream-major states kernel: the power of two >= 4 whose run of one stream is a cache line"""
    R_ = 4
    while p.n_in and R_ * p.n_in < 32:
        R_ *= 2
    return R_


def lds_bytes(p, block, R_, slots=None):
    """rings and an x-only patch: 4 block (slots + R n_in + 4); a graph without input wires declares no patch"""
    slots = RS.ring_slots(p) if slots is None else slots
    return 4 * block * (slots + (R_ * p.n_in + 4 if p.n_in else 0))


def geometry(p):
    """(U, R, block) of the stream-major ring states kernel, or (U, Rmin, 0) when nothing fits: R from R0 = twice the plain states
    kernel's, halved down to Rmin = max(4, U); per R the block over 256, 128, 64; the first pair that fits the LDS twice, failing that
    the first that fits once"""
    U, slots = states_unroll(p), RS.ring_slots(p)
    R0, Rmin = 2 * states_patch_rows(p), max(4, U)
    for times in (2, 1):
        R_ = R0
        while R_ >= Rmin:
            for block in (256, 128, 64):
                if times * lds_bytes(p, block, R_, slots) <= LDS_BYTES:
                    return U, R_, block
            R_ //= 2
    return U, Rmin, 0


SYMBOL = re.compile(r"fz_states_ring_sm_kernel_u(\d+)r(\d+)b(\d+)_g([0-9a-f]{8})")


def symbol_geometry(sym):
    """(U, R, block) the kernel's symbol names"""
    assert SYMBOL.fullmatch(sym), sym
    return symbol_shape(sym, "u")


# ---- the states kernels' text: one per layout, the ring a switch (zignal_amd/csrc/fz_kernel_states{,_sm}.hip.inc) ------------------------
HAND_WRITTEN = "// ==== fz_block_kernel.hip.inc ====\n"


def hand_written(src):
    """the hand-written part of a kernel's source: what follows the generated configuration and body"""
    return src.split(HAND_WRITTEN)[1]


def compiled_text(src):
    """the hand-written part of a states kernel's source as the FZ_RING of its configuration compiles it: the other side of every
    `#if FZ_RING` and the comments set aside (conditionals on anything else stay as they stand)"""
    ring = int(re.search(r"^#define FZ_RING ([01]) ", src, re.M).group(1))
    out, open_ifs = [], []                                        # per open #if: None, or for `#if FZ_RING` whether its side here compiles
    for ln in hand_written(src).split("\n"):
        word = ln.split()[0] if ln.strip() else ""
        if word in ("#if", "#ifdef", "#ifndef"):
            open_ifs.append(bool(ring) if re.fullmatch(r"#if FZ_RING\s*", ln) else None)
            switch = open_ifs[-1] is not None                     # the line is one of the switch's own: never kept
        elif word in ("#else", "#elif"):
            switch = open_ifs[-1] is not None
            assert not (switch and word == "#elif"), ln
            if switch:
                open_ifs[-1] = not open_ifs[-1]
        elif word == "#endif":
            switch = open_ifs.pop() is not None
        else:
            switch = False
        if not switch and all(side is not False for side in open_ifs):
            out.append(ln)
    assert not open_ifs
    return re.sub(r"//.*|/\*.*?\*/", "", "\n".join(out))


# ---- shapes ------------------------------------------------------------------------------------------------------------------------------
def windows(T):
    """(rows_total, row0) of the two windows of a recording of T rows: the whole buffer, and four rows in with rows behind it"""
    return [(H.up4(T), 0), (H.up4(4 + T) + 4, 4)]


def boundary_cases(name):
    """(streams, rows, block_rows) that put block starts on, before and after a patch boundary: T in R - 1, R, R + 1, 2 R + 3 (R the states
    kernel's patch rows) at 65 streams with blocks of 4 rows and the default"""
    R_ = geometry(prog(name))[1]
    return [(65, T, B) for T in (R_ - 1, R_, R_ + 1, 2 * R_ + 3) for B in (4, 0)]


def cases(name):
    """((streams, rows, block_rows), checkpoint_rows) of every bitwise case of a graph"""
    out = [(t, 0) for t in R.triples(name)] + [(R.below_depth(name), 1)]
    if name in BOUNDARY_GRAPHS:
        out += [(t, 0) for t in boundary_cases(name)]
    return out


def forward_shape(name):
    """(streams, rows) of the run_block_stream_major launch state_out is compared with, and of autograd: rows on the float4 grid"""
    return 65, H.up4(DEEPEST[name] + 5)


# ---- one launch through the C ABI ------------------------------------------------------------------------------------------------------
def launch(p, d, B, loss, window=None, c=0, state_grad=True, alias=False, leave_out=()):
    """grad_harness.launch of fz_run_recording_ring_grad_stream_major / fz_run_recording_ring_loss_grad_stream_major on the time-major
    draw d of ring_recording_graphs.case (both dL/dy and the target: the call takes the one it needs), in blocks of B rows (0: the
    library's choice), grad_scale = K.  window: (rows_total, row0), default windows(T)[0]"""
    x, s0, par, yb, tg, sb, ap, ac, al = d
    return H.launch(p, (x, s0, par, tg if loss else yb, sb, ap, ac, al), ring=True, loss=loss, window=window or windows(x.shape[0])[0],
                    recording=B, c=c, state_grad=state_grad, alias=alias, leave_out=leave_out, k=K)


# ---- the kernels the GPU tests launch: tests/golden/ring_sm_recording_kernels.fzm.gz ---------------------------------------------------
def resolve():
    """what a recording process calls (FLOWZ_HIP_MANIFEST set): the stream-major ring states kernels, the stream-major ring and ring loss
    kernels at the strides used, the time-major kernels compared with, and the stream-major forward kernels state_out is compared with"""
    from zignal_amd import flowz as F
    for n in sorted(GRAPHS):
        p = prog(n)
        p.ring_states_resources(stream_major=True)
        p.ring_states_resources()
        for c in STRIDES:
            for sm in (True, False):
                p.ring_grad_resources(c, stream_major=sm)
                p.ring_loss_grad_resources(c, stream_major=sm)
        ns, rows = forward_shape(n)
        p.build(F.make_variant(0, 0, 0, F.C.FZ_VF_STREAM_MAJOR), ns, rows)


def record():
    """record the manifest with the library as it is; needs no GPU.  By hand: PYTHONPATH=. python tests/ring_sm_recording.py"""
    from zignal_amd import flowz as F
    code = "import sys\nsys.path[:0] = [%r, %r]\nimport ring_sm_recording as S\nS.resolve()\n" % (os.path.dirname(HERE), HERE)
    with tempfile.TemporaryDirectory() as td:
        raw = os.path.join(td, "manifest.fzm")
        subprocess.check_call([sys.executable, "-c", code], env=dict(os.environ, FLOWZ_HIP_MANIFEST=raw))
        with open(raw, "rb") as f, open(MANIFEST, "wb") as out:
            out.write(gzip.compress(f.read(), 9, mtime=0))
    return F.manifest_build(MANIFEST)


manifest_variants = R.RL.manifest_variants


if __name__ == "__main__":
    print("kernel manifest:", record())
