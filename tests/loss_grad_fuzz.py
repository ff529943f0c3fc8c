"""What the fuzz tests of the two loss-gradient kernels share (fz_run_block_loss_grad, fz_run_block_loss_grad_stream_major over the cells
of tests/grad_fuzz_cells.py and the sin / cos / log graphs of tests/trig_cells.py): the draws, the targets at their edges, the loss
summed in the wrong orders a kernel could sum it in, and the kernel manifest of everything test_loss_grad_fuzz_gpu.py launches
(tests/golden/loss_grad_fuzz_kernels.fzm.gz; `PYTHONPATH=. python tests/loss_grad_fuzz.py` records it, without a GPU).

The named graphs of loss_grad_ref.GPU_GRAPHS all have one output wire; REACHES names what the loss kernels are parametrised over beyond
them, with a cell that gets there."""
import gzip
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

import adjoint_ref as A
import grad_fuzz_cells as GC

F32, F64 = np.float32, np.float64
HERE = os.path.dirname(os.path.abspath(__file__))
MANIFEST = os.path.join(HERE, "golden", "loss_grad_fuzz_kernels.fzm.gz")
K = 0.37                                                          # grad_scale of every launch: no power of two, so e * k rounds
N_CHUNKS = 8                                                      # about six cells per test

# feature -> (a cell that has it, the predicate on (program, C, R))
REACHES = {
    "n_out >= 2": ("make4", lambda p, c, r: p.n_out >= 2),
    "n_out >= 2 and != n_in": ("make11", lambda p, c, r: p.n_out >= 2 and p.n_out != p.n_in and p.n_in > 0),
    "n_in == 0": ("generator_without_input", lambda p, c, r: p.n_in == 0),
    "no state": ("no_delay_line", lambda p, c, r: p.n_state == 0),
    "an output that is an input or a delay": ("passes_input_and_delayed_input", lambda p, c, r: {"out_is_input", "out_is_delay"} <= GC.features(p)),
    "C == 1": ("cascade9_depth8", lambda p, c, r: c == 1),
    "R == 8 with n_out >= 2": ("grad133", lambda p, c, r: r == 8 and p.n_out >= 2),
}
SUBSET_CELL = "make11"                                            # 1 in, 6 out: in_grad and out differ in width
EDGE_CELLS = ("grad11", "generator_without_input")           # 1 in, 6 out, per-stream coefficients; no input wire
AUTOGRAD_CELLS = ("make11", "grad16")                             # multi-output, no node with a tie
TRIG_SHAPE, TRIG_STRIDES, TRIG_ROW0 = (130, 37), (0, 4), 4


def draw(cell, ns, T, seed):
    """grad_fuzz_cells.inputs -- its dL/dy serves as the target -- and a loss accumulator that is not zero"""
    x, s0, par, tg, sb, ap, ac = GC.inputs(cell, ns, T, seed)
    al = np.random.default_rng(seed + 1).standard_normal(ns).astype(F32)
    return x, s0, par, tg, sb, ap, ac, al


def draw_trig(p, ns, T, seed):
    """test_trig_log_gpu.grad_inputs' draws and a loss accumulator"""
    from grad_harness import make_inputs
    d = make_inputs(p, "trig", ns, T, seed, ties=False, draw_params=lambda p_, n, rng: rng.uniform(0.01, 0.5, (p_.n_param, n)).astype(F32))
    return d + (np.random.default_rng(seed + 1).standard_normal(ns).astype(F32),)


def longest_65(cell):
    """(shape index, T) of the cell's longest block at 65 streams among grad_fuzz_cells.shapes"""
    sh = GC.shapes(cell)
    T = max(t for n, t in sh if n == 65)
    return sh.index((65, T)), T


# ---- the loss in the documented order and in the orders a wrong kernel would take ------------------------------------------------
def losses(y, target, al):
    """{order: loss [ns]} -- "documented": rows T-1 .. 0, slots ascending, e * e rounded and then added (loss_grad_ref.loss_grad);
    "rows ascending"; "slots descending"; "unrounded product": loss + e * e rounded once, as a fused multiply-add gives it (the
    product of two float32 is exact in float64)"""
    T, ns, n_out = y.shape
    out = {}
    with np.errstate(all="ignore"):
        e = np.asarray(y, F32) - np.asarray(target, F32)
        for name, rows, slots in (("documented", range(T - 1, -1, -1), range(n_out)), ("rows ascending", range(T), range(n_out)),
                                  ("slots descending", range(T - 1, -1, -1), range(n_out - 1, -1, -1))):
            ls = np.array(al, F32).copy()
            for t in rows:
                for j in slots:
                    ls = ls + e[t, :, j] * e[t, :, j]
            out[name] = ls
        ls = np.array(al, F32).copy()
        for t in range(T - 1, -1, -1):
            for j in range(n_out):
                ls = (ls.astype(F64) + e[t, :, j].astype(F64) * e[t, :, j].astype(F64)).astype(F32)
        out["unrounded product"] = ls
    return out


# ---- targets at their edges --------------------------------------------------------------------------------------------------------
EDGE_KINDS = ("y", "nan", "+inf", "-inf", "zeros", "overflow", "denormal")
TINY = F32(2.0 ** -64)                                            # the scale of the "denormal" streams' x and state


def edge_kind(s):
    """what stream s gets: the kinds in turn, then as many ordinary streams (None)"""
    k = s % (2 * len(EDGE_KINDS))
    return EDGE_KINDS[k] if k < len(EDGE_KINDS) else None


def edge_case(cell, ns, T, seed, ref=A):
    """draw(), with the target of every stream s with edge_kind(s):
        y         y itself, bit for bit: e = +0, dL/dy = +0, the loss stays the accumulator
        nan, +inf, -inf, zeros (+0 and -0 in turn)
        overflow  -+3e19 against y's sign: e * grad_scale is finite, e * e is not
        denormal  x and the state of the stream scaled by 2^-64 and target = 2 y, so e = -y and e * e = y * y lies below 2^-126 wherever y
                  follows the scale (a graph that adds a constant to its output, as generator_without_input does, cannot get there: the
                  difference of two float32 near 0.1 is 0 or at least 2^-27.  Such a stream takes y's neighbour, the smallest e there is)
    In the first round of kinds (s < 14) the value fills the stream; in later rounds it sits in every other (row + slot) only, so that
    finite and special terms meet in one accumulator.  Returns (the eight inputs, kind of every stream)"""
    p = GC.prog(cell)
    x, s0, par, tg, sb, ap, ac, al = draw(cell, ns, T, seed)
    kinds = [edge_kind(s) for s in range(ns)]
    den = np.array([k == "denormal" for k in kinds])
    x[:, den] *= TINY
    s0[:, den] *= TINY
    y, _ = ref.forward(p, x, s0, par)
    t, j = np.meshgrid(np.arange(T), np.arange(p.n_out), indexing="ij")
    for s, kind in enumerate(kinds):
        if kind is None:
            continue
        ys = y[:, s]
        with np.errstate(all="ignore"):
            v = {"y": ys, "nan": np.full_like(ys, np.nan), "+inf": np.full_like(ys, np.inf), "-inf": np.full_like(ys, -np.inf),
                 "zeros": np.where((t + j) % 4 < 2, F32(0.0), F32(-0.0)).astype(F32), "overflow": np.where(ys < 0, F32(3e19), F32(-3e19)).astype(F32),
                 "denormal": np.where(np.abs(ys) < F32(2.0 ** -40), ys + ys, np.nextafter(ys, F32(np.inf)))}[kind]
        m = np.ones((T, p.n_out), bool) if s < 2 * len(EDGE_KINDS) else (t + j) % 2 == 0
        tg[:, s][m] = v[m]
    return (x, s0, par, tg, sb, ap, ac, al), kinds


# ---- the kernels of the GPU tests --------------------------------------------------------------------------------------------------
def kernel_requests():
    """(program, checkpoint_rows, stream_major) of every loss kernel test_loss_grad_fuzz_gpu.py launches: the default stride of every
    cell and trig graph, strides 1 and 4 of grad_fuzz_cells.STRIDE_CELLS, stride 4 of the trig graphs"""
    import trig_cells as TC
    out = []
    for cell in GC.CELLS:
        out += [(GC.prog(cell), 0, sm) for sm in (False, True)]
    for cell in GC.STRIDE_CELLS:
        out += [(GC.prog(cell), c, sm) for c in (1, 4) for sm in (False, True)]
    for name in TC.GRAD_GRAPHS:
        out += [(TC.graph(name), c, sm) for c in TRIG_STRIDES for sm in (False, True)]
    return out


def record(path):
    """the raw manifest of kernel_requests(), written by a process that records (FLOWZ_HIP_MANIFEST); needs no GPU"""
    code = ("import sys\nsys.path[:0] = [%r, %r]\nimport loss_grad_fuzz as LF\n"
            "for p, c, sm in LF.kernel_requests():\n    p.loss_grad_resources(c, stream_major=sm)\n") % (os.path.dirname(HERE), HERE)
    subprocess.check_call([sys.executable, "-c", code], env=dict(os.environ, FLOWZ_HIP_MANIFEST=path))
    with open(path, "rb") as f:
        return f.read()


def records(raw):
    """{(P, U, block, flags, recipe)} of a raw manifest"""
    out, at = set(), 0
    while at < len(raw):
        m = re.compile(rb"FZM1 (\d+) (\d+) (\d+) (\d+) (\d+)\n").match(raw, at)
        assert m, raw[at:at + 40]
        n = int(m.group(5))
        out.add(tuple(int(g) for g in m.groups()[:4]) + (raw[m.end():m.end() + n],))
        at = m.end() + n
    return out


def record_manifest():
    """tests/golden/loss_grad_fuzz_kernels.fzm.gz.  build() replays every manifest under tests/golden/, so a GPU run finds these built"""
    from zignal_amd import flowz as F
    with tempfile.TemporaryDirectory() as td:
        raw = record(os.path.join(td, "manifest.fzm"))
    with open(MANIFEST, "wb") as out:
        out.write(gzip.compress(raw, 9, mtime=0))
    return F.manifest_build(MANIFEST)


if __name__ == "__main__":
    print("kernel manifest:", record_manifest())
