"""What the fuzz of the backward of a whole recording shares (fz_run_recording_grad, fz_run_recording_loss_grad and the two
block-start-states kernels behind them; test_recording_fuzz_host.py, test_recording_fuzz_gpu.py): the graphs, the shapes of every
graph as a committed rule over the graph's own strides, the draws, the restatement with a wrong chain that the inputs must tell from the
right one, the pins of the states kernels (tests/golden/recording_fuzz_pins.json) and the kernel manifest of everything the GPU test
launches that no other manifest holds (tests/golden/recording_fuzz_kernels.fzm.gz).  `PYTHONPATH=. python tests/recording_fuzz.py`
rewrites the pins and records the manifest, without a GPU.

Both states kernels are parametrised by the width of the input frame alone (fz_grad.cpp: states_unroll, states_sm_patch_rows): the
rows of an unrolled group U, and stream-major U = min(U, R) with R the rows of the LDS patch.  CLASSES is that table.  The 48 cells
of tests/grad_fuzz_cells.py reach n_in = 0 .. 3, and six crafted graphs with wide input frames (WIDE) reach the classes from four wires
on.  Of the sin / cos / log graphs of tests/trig_cells.py, all3's state passes through sin and cos, so its fz_adj::fwd has to give the
forward planner's bits through the argument reduction; pm's state is a phase that touches neither its input nor sin (its states kernels
fetch no x), and log lies on no state path of either graph: there the two only add node kinds to the block launches."""
import gzip
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

import adjoint_ref as A
import adjoint_ref_trig as AT
import grad_fuzz_cells as GC
import trig_cells as TC
from grad_harness import up4
from graphs import DEL, IN, add, chan, lit, mul
from zignal_amd import flowz as F

F32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
PINS_FILE = os.path.join(HERE, "golden", "recording_fuzz_pins.json")
MANIFEST = os.path.join(HERE, "golden", "recording_fuzz_kernels.fzm.gz")
K = 0.37                                                          # grad_scale of every loss launch: no power of two, so e * k rounds
BASE = 800                                                        # triple i of shapes(name) is drawn with seed BASE + i

# (n_in from, to (None: and beyond), time-major kernel, stream-major kernel) -- the states kernels by input frame width
CLASSES = [(0, 0, "u8", "u4r4"), (1, 1, "u8", "u8r32"), (2, 2, "u8", "u8r16"), (3, 3, "u4", "u4r16"), (4, 4, "u4", "u4r8"),
           (5, 7, "u2", "u2r8"), (8, 8, "u2", "u2r4"), (9, None, "u1", "u1r4")]

# name -> (n_in, n_out) of the crafted wide graphs
WIDE = {"wide5x1": (5, 1), "wide8x2": (8, 2), "wide9x1": (9, 1), "wide16x1": (16, 1), "wide4x4": (4, 4), "wide40x1": (40, 1)}
TIME_MAJOR_ONLY = ("wide40x1",)                                   # neither stream-major kernel's patch fits the LDS: refused
# name -> (ns, T, B, row0): one triple more, stream-major only.  B is the smallest block length above 4 that is no multiple of 4 and that
# the ABI takes (B n_in, B n_out, row0 n_in and row0 n_out are multiples of 4 floats), row0 the last row before 4 it takes: the block
# windows start at rows 3, 8, 13 and at rows 2, 8, 14, off the 4-row grid, and the last block is a short one
SM_ONLY = {"wide4x4": (65, 13, 5, 3), "wide8x2": (65, 15, 6, 2)}


def wide(n, n_out):
    """output o = sum_k c[o][k] * _k + d[o] * _1[_2] + sum_{k >= 2} g[o][k] * _k[_1], the outputs joined with chan(): n input wires, a
    delay line of depth 2 on wire 1 and one of depth 1 on every other wire, n + 1 state rows.  A states kernel runs fz_adj::fwd alone,
    which computes the next state and nothing of y: with the line of wire 1 only, every other wire would be dead code there -- no
    load of it, none of the U n_in frame registers that states_unroll bounds.  With a line on every wire the whole frame is live"""
    outs = []
    for o in range(n_out):
        e = mul(lit(0.3 - 0.05 * o), IN(1))
        for k in range(2, n + 1):
            e = add(e, mul(lit(0.1 + 0.01 * k + 0.02 * o), IN(k)))
        e = add(e, mul(lit(0.4 - 0.1 * o), DEL(1, 2)))
        for k in range(2, n + 1):
            e = add(e, mul(lit(0.05 + 0.002 * k + 0.01 * o), DEL(k, 1)))
        outs.append(e)
    return outs[0] if n_out == 1 else chan(*outs)


NAMES = list(GC.CELLS) + list(TC.GRAD_GRAPHS) + list(WIDE)
CRAFTED = list(TC.GRAD_GRAPHS) + list(WIDE)                       # what no test of the cells compiles a states kernel of
_progs = {}


def prog(name):
    if name not in _progs:
        _progs[name] = GC.prog(name) if name in GC.CELLS else TC.graph(name) if name in TC.GRAD_GRAPHS else F.compile(F.from_sexpr(wide(*WIDE[name])))
    return _progs[name]


def ref_of(name):
    """the module that restates the graph: sin, cos and log are tests/adjoint_ref_trig.py's"""
    return AT if name in TC.GRAD_GRAPHS else A


def wires_the_state_reads(p):
    """the input wires the next state depends on within a step (a delayed read is the state's own): what fz_adj::fwd keeps of x once
    the compiler has dropped the arithmetic of y"""
    L = A.Layout(p)
    seen, todo = set(), [src for src, _, _ in L.lines]
    while todo:
        k = todo.pop()
        if k in seen:
            continue
        seen.add(k)
        kind, a, b, _ = L.ir[k]
        if kind not in ("input", "const", "param", "delay"):
            todo += [a] if kind in A._UN else [a, b]
    return {L.ir[k][1] for k in seen if L.ir[k][0] == "input"}


def layouts(name):
    return (False,) if name in TIME_MAJOR_ONLY else (False, True)


# ---- what a graph resolves to -------------------------------------------------------------------------------------------------------
def symbols(name):
    """(time-major, stream-major) states symbol; None: refused"""
    p, out = prog(name), []
    for sm in (False, True):
        try:
            out.append(p.states_kernel_symbol(sm))
        except F.FlowzError:
            out.append(None)
    return tuple(out)


def strides(name):
    """dict u_tm, u_sm, r (the states kernels' unrolled groups and LDS patch rows), c, r_adj (the adjoint kernels' checkpoint stride and
    patch rows), read from the symbols.  Where the stream-major kernels are refused, u_sm is u_tm and both r and r_adj are max(4, c):
    the shapes still walk the same boundaries"""
    tm, sm = symbols(name)
    c, r_adj = GC.strides(prog(name))
    assert (sm is None) == (r_adj is None), f"{name}: one stream-major kernel is refused and the other is not: the shapes rule has no case for it"
    u_tm = int(re.fullmatch(r"fz_states_kernel_u(\d+)b256_g[0-9a-f]{8}", tm).group(1))
    if sm is None:
        return dict(u_tm=u_tm, u_sm=u_tm, r=max(4, c), c=c, r_adj=r_adj or max(4, c))
    m = re.fullmatch(r"fz_states_sm_kernel_u(\d+)r(\d+)b256_g[0-9a-f]{8}", sm)
    return dict(u_tm=u_tm, u_sm=int(m.group(1)), r=int(m.group(2)), c=c, r_adj=r_adj)


def resolved(name):
    """a graph's pin: the two states symbols up to the workgroup size (None: refused) and the program's sizes"""
    p = prog(name)
    tm, sm = (s and s[:s.index("b256") + 4] for s in symbols(name))
    return {"time_major": tm, "stream_major": sm, "sizes": [p.n_in, p.n_out, p.n_state, p.n_param, p.n_const]}


def load_pins():
    with open(PINS_FILE) as f:
        return json.load(f)


# ---- shapes -------------------------------------------------------------------------------------------------------------------------
def shapes(name):
    """[(ns, T, B)], at most eight, from the graph's own strides():
        (1, 1, 4)                 one row: the time-major prefetch of both groups clamps to row 0
        (65, 3, 4)                1 < T < U wherever U > 2: a first group that is not full
        (64, U + 1, 4)            a group and a row, of either layout's U; with U = 8 two block starts inside one group
        (321, R, up4(R) + 4)      a last patch that is exactly full, in one block (B >= T)
        (65, R + 1, 4)            a patch and a row, in blocks of 4: the last block has one row
        (321, 2 R_adj + 3, b)     two patches of the adjoint kernel and three rows; b = 12 where C > 4 (a multiple of 4 but not of C),
                                  else 4 (T >= 11: block starts at every fourth row, a last block of three)
        (64, 2 R_adj + 3, C)      where C > 4: blocks of whole checkpoint chunks
    1, 64 (a wave exactly full), 65 and 321 streams are spread over the triples, not multiplied out.  B is a multiple of 4 throughout:
    time-major blocks are pointer offsets that keep the 16-byte alignment (SM_ONLY has the others)"""
    s = strides(name)
    out = [(1, 1, 4), (65, 3, 4)]
    out += [(64, u + 1, 4) for u in sorted({s["u_tm"], s["u_sm"]}, reverse=True)]
    out += [(321, s["r"], up4(s["r"]) + 4), (65, s["r"] + 1, 4)]
    T = 2 * s["r_adj"] + 3
    out.append((321, T, 12 if s["c"] > 4 else 4))
    if s["c"] > 4:
        out.append((64, T, s["c"]))
    return out


def longest(name):
    """(index, triple) of the graph's longest triple (the first of them)"""
    sh = shapes(name)
    i = max(range(len(sh)), key=lambda j: (sh[j][1], -j))
    return i, sh[i]


def chain_triple(name):
    """(index, triple): blocks of 4 rows and the largest T -- the most block boundaries a gradient has to cross"""
    sh = shapes(name)
    i = max((j for j in range(len(sh)) if sh[j][2] == 4), key=lambda j: (sh[j][1], -j))
    return i, sh[i]


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
def draw(name, ns, T, seed):
    """x, state, params, target (also dL/dy), dL/d(state after) and three accumulators, none of them zero: grad_harness.make_inputs as
    test_recording_grad_gpu.draw calls it for a cell"""
    from grad_harness import make_inputs
    p = prog(name)
    x, s0, par, tg, sb, ap, ac = make_inputs(p, name, ns, T, seed, draw_params=GC.draw_params, ties=GC.has_ties(p), special_every=GC.SPECIAL_EVERY)
    al = np.random.default_rng(seed + 1).standard_normal(ns).astype(F32)
    return x, s0, par, tg, sb, ap, ac, al


def clean_streams(name, ns):
    """the streams without specials: all, or for a graph with ties those that are no SPECIAL_EVERY-th"""
    return np.arange(ns) % GC.SPECIAL_EVERY != 0 if GC.has_ties(prog(name)) else np.ones(ns, bool)


def restated(name, d, B, loss):
    """recording_ref.grad of a draw"""
    import recording_ref as RR
    x, s0, par, tg, sb, ap, ac, al = d
    kw = dict(target=tg, k=K, accum_loss=al) if loss else dict(out_grad=tg)
    return RR.grad(prog(name), x, B, state=s0, params=par, state_grad=sb, accum_params=ap, accum_consts=ac, ref=ref_of(name), **kw)


def single(name, d, loss):
    """the one call over all rows: adjoint_ref.grad or loss_grad_ref.loss_grad"""
    import loss_grad_ref as LR
    x, s0, par, tg, sb, ap, ac, al = d
    p, ref = prog(name), ref_of(name)
    return LR.loss_grad(p, x, tg, K, s0, par, sb, ap, ac, al, ref=ref) if loss else ref.grad(p, x, tg, s0, par, sb, ap, ac)


def wrong_chain(name, d, B):
    """the plain backward block by block as recording_ref.grad restates it, but for one thing: every block gets the CALLER's state
    gradient, not the one the block behind it wrote.  {x, state, params, consts}"""
    import recording_ref as RR
    x, s0, par, tg, sb, ap, ac, al = d
    p, ref = prog(name), ref_of(name)
    st, _ = RR.starts(p, x, B, s0, par, ref)
    gx, r = [None] * len(st), None
    for kb in range(len(st) - 1, -1, -1):
        rows = slice(kb * B, min((kb + 1) * B, x.shape[0]))
        r = ref.grad(p, x[rows], tg[rows], st[kb], par, sb, ap, ac)
        gx[kb], ap, ac = r["x"], r["params"], r["consts"]
    return dict(r, x=np.concatenate(gx))


# ---- the kernels of the GPU test ----------------------------------------------------------------------------------------------------
def resolve_kernels():
    """resolve every kernel test_recording_fuzz_gpu.py launches that no other manifest under tests/golden/ holds: the states kernels of
    every graph with state in both layouts, the adjoint and loss kernels of the wide graphs (the cells' are in grad_fuzz_kernels and
    loss_grad_fuzz_kernels, the sin / cos / log graphs' in trig_log_kernels and loss_grad_fuzz_kernels), and the forward kernel of every
    graph's longest triple, which state_out is compared with.  Returns how many calls resolved a kernel"""
    n = 0
    for name in NAMES:
        p = prog(name)
        for sm in layouts(name):
            if p.n_state:                                         # (a graph without delay lines launches no states kernel)
                p.states_resources(sm)
                n += 1
            if name in WIDE:
                p.grad_resources(0, stream_major=sm)
                p.loss_grad_resources(0, stream_major=sm)
                n += 2
        if p.n_state:
            ns, T, _ = longest(name)[1]
            p.build(None, ns, T)
            n += 1
    return n


def record(path=None):
    """resolve_kernels() in a process that records (FLOWZ_HIP_MANIFEST); needs no GPU.  Returns the raw manifest.  By hand:
        FLOWZ_HIP_MANIFEST=m.fzm python -c "import sys; sys.path.insert(0, 'tests'); import recording_fuzz as RF; RF.resolve_kernels()"; gzip -9n m.fzm"""
    code = "import sys\nsys.path[:0] = [%r, %r]\nimport recording_fuzz as RF\nRF.resolve_kernels()\n" % (os.path.dirname(HERE), HERE)
    with tempfile.TemporaryDirectory() as td:
        path = path or os.path.join(td, "manifest.fzm")
        subprocess.check_call([sys.executable, "-c", code], env=dict(os.environ, FLOWZ_HIP_MANIFEST=path))
        with open(path, "rb") as f:
            return f.read()


def records(raw):
    """{(P, U, block, flags, recipe)} of a raw manifest"""
    from loss_grad_fuzz import records as parse
    return parse(raw)


def record_manifest():
    """tests/golden/recording_fuzz_kernels.fzm.gz.  build() replays every manifest under tests/golden/, so a GPU run finds these built"""
    with open(MANIFEST, "wb") as out:
        out.write(gzip.compress(record(), 9, mtime=0))
    return F.manifest_build(MANIFEST)


if __name__ == "__main__":                         # rewrite the pins of the library as it is (review the diff), then the manifest
    pins = {name: resolved(name) for name in NAMES}
    with open(PINS_FILE, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in pins.items()) + "\n}\n")
    print("kernel manifest:", record_manifest())
