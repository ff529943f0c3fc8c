"""The graphs the two adjoint kernels are fuzzed on (fz_run_block_grad, fz_run_block_grad_stream_major): a fixed selection of seeded
random graphs (tests/randgraphs.py: make, make_cmp_grad, make_grad) and a few crafted ones, their inputs, and what they resolve to.

The named graphs of tests/grad_graphs.py leave most of what the kernel skeletons are parametrised over untouched: five (C, R) classes
of ten (C the checkpoint stride, R the rows of the stream-major kernel's LDS patch), no C = 1, no delay line deeper than 2, three frame
shapes, no output slot that is an input or a delayed read, no node without an adjoint.  SELECTED is what select() picks: walking the
seeds of the three generators in order, a seed is taken when it adds a (C, R) class, a structural feature (FEATURES) or a node kind that
is not yet held three times -- and only when the GPU test's inputs put a signal on every adjoint of it (signal_gaps).  (The frame
shape is no key of its own: nearly every seed has a (C, R, n_in, n_out) nobody else has, and
the budget would be spent on the first generator; the shapes the selection reaches are listed by the host test.)  The list is
committed, not recomputed: a planner change that moves a cell shows in the pins
(tests/golden/grad_fuzz_pins.json; `python tests/grad_fuzz_cells.py` rewrites them, prints what select() picks now and records the
kernel manifest of the cells, tests/golden/grad_fuzz_kernels.fzm.gz).

test_grad_fuzz_host.py checks pins, coverage, the restatement (tests/adjoint_ref.py) against float64 autograd and that both kernels of
every cell compile without scratch; test_grad_fuzz_gpu.py holds both kernels to the restatement bit for bit."""
import json
import os
import re

import numpy as np

import graphs as G
import randgraphs as RG
from graphs import DEL, IN, add, chan, fb, lit, mul, seq
from zignal_amd import flowz as F

F32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
PINS_FILE = os.path.join(HERE, "golden", "grad_fuzz_pins.json")
MANIFEST = os.path.join(HERE, "golden", "grad_fuzz_kernels.fzm.gz")
HELD, SEEDS = 3, 300                              # how often a class / feature is held, seeds walked per generator
SHARES = (("make", 13), ("cmp", 8), ("grad", 11))  # graphs per generator before its walk takes only what is not held at all: 43 selected, 48 cells with the crafted ones
FEATURES = ("out_is_input", "out_is_delay", "unreached", "line_from_input", "neg", "div_by_coef", "le", "ge", "eq", "ne", "depth8", "param", "out5")
STRIDE_CELLS = ("cascade9_depth8", "grad18")      # the C = 1 cell and one with a line of depth 8: also run at checkpoint_rows 1 and 4
GPU_SEED = 500                                    # test_grad_fuzz_gpu.py draws shape i of shapes(cell) with seed GPU_SEED + i
TIES = ("abs", "min", "max", "lt", "le", "gt", "ge", "eq", "ne")   # node kinds whose rule depends on a tie or a special value


# ---- crafted graphs -------------------------------------------------------------------------------------------------------------
def cascade9_depth8():
    """nine stages _1 + c*_1[_8]: 72 state rows, more than 64 -- the only way to the checkpoint stride C = 1"""
    cs = (0.4, -0.35, 0.3, -0.25, 0.2, 0.45, -0.15, 0.1, -0.3)
    return seq(*[add(IN(1), mul(lit(c), DEL(1, 8))) for c in cs])


def no_delay_line():
    """no state at all: the state pointers are null and the workspace is empty.  2 in / 2 out"""
    return chan(add(mul(lit(0.7), IN(1)), G.fn("tanh", mul(lit(-0.4), IN(2)))), mul(IN(1), IN(2)))


def passes_input_and_delayed_input():
    """the only outputs are an input wire and a delayed input wire: both output slots are nodes without arithmetic"""
    return chan(IN(1), DEL(1, 3))


def generator_without_input():
    """~(p0 * _1[_1] + 0.1): a feedback with no input wire, its coefficient a per-stream parameter"""
    return fb(add(mul(G.param(0), DEL(1, 1)), lit(0.1)))


def gated_by_a_wire_nothing_differentiates():
    """_1 * (0.3*_2 > 0.1) + 0.5*_1[_2]: wire 2, the product 0.3*_2 and both of its literals feed a comparison only.  No adjoint reaches
    them: dL/dx of wire 2 is +0.0 in every row and the coefficient accumulators of 0.3 and 0.1 stay what they were, also where _2 is
    infinite or NaN (an adjoint of -0.0 handed on through the product would turn them into -0.0 and NaN: no random cell tells)"""
    return add(mul(IN(1), G.cmp("gt", mul(lit(0.3), IN(2)), lit(0.1))), mul(lit(0.5), DEL(1, 2)))


CRAFTED = {
    "cascade9_depth8": cascade9_depth8,
    "no_delay_line": no_delay_line,
    "passes_input_and_delayed_input": passes_input_and_delayed_input,
    "generator_without_input": generator_without_input,
    "gated_by_a_wire_nothing_differentiates": gated_by_a_wire_nothing_differentiates,
}

GENERATORS = {
    "make": lambda seed: RG.make(seed)[0],
    "cmp": lambda seed: RG.make_cmp_grad(seed)[0],
    "grad": lambda seed: RG.make_grad(seed)[0],
}

# (generator, seed): what select() picked when the list was made
SELECTED = [
    ("make", 0), ("make", 1), ("make", 2), ("make", 3), ("make", 4), ("make", 5), ("make", 6), ("make", 8), ("make", 10), ("make", 11),
    ("make", 12), ("make", 18), ("make", 21), ("make", 25), ("make", 27), ("make", 29), ("make", 34), ("make", 94), ("make", 142),
    ("cmp", 21), ("cmp", 27), ("cmp", 31), ("cmp", 34), ("cmp", 42), ("cmp", 46), ("cmp", 53), ("cmp", 60),
    ("grad", 4), ("grad", 5), ("grad", 7), ("grad", 9), ("grad", 11), ("grad", 13), ("grad", 15), ("grad", 16), ("grad", 17), ("grad", 18),
    ("grad", 20), ("grad", 33), ("grad", 70), ("grad", 106), ("grad", 133), ("grad", 212),
]

CELLS = [f"{g}{s}" for g, s in SELECTED] + list(CRAFTED)


def sexpr(cell):
    if cell in CRAFTED:
        return CRAFTED[cell]()
    m = re.fullmatch(r"([a-z]+)(\d+)", cell)
    return GENERATORS[m.group(1)](int(m.group(2)))


_progs = {}


def prog(cell):
    if cell not in _progs:
        _progs[cell] = F.compile(F.from_sexpr(sexpr(cell)))
    return _progs[cell]


# ---- what a program resolves to ---------------------------------------------------------------------------------------------------
def strides(p, checkpoint_rows=0):
    """(C, R) by the kernels' symbols; R is None where the stream-major patch does not fit the LDS (the library refuses it)"""
    c = int(re.match(r"fz_adjoint_kernel_c(\d+)b", p.grad_kernel_symbol(checkpoint_rows)).group(1))
    try:
        m = re.match(r"fz_adjoint_sm_kernel_c(\d+)r(\d+)b", p.grad_kernel_symbol(checkpoint_rows, stream_major=True))
    except F.FlowzError:
        return c, None
    assert int(m.group(1)) == c
    return c, int(m.group(2))


def features(p):
    """the structural features (FEATURES) of a program the backward takes"""
    import adjoint_ref as A
    L = A.Layout(p)
    ir = L.ir
    f = set()
    for o in L.outs:
        if ir[o][0] == "input":
            f.add("out_is_input")
        if ir[o][0] == "delay":
            f.add("out_is_delay")
    if not all(L.has):
        f.add("unreached")
    if any(ir[src][0] == "input" for src, _, _ in L.lines):
        f.add("line_from_input")
    for kind, a, b, _ in ir:
        if kind in ("neg", "le", "ge", "eq", "ne"):
            f.add(kind)
        if kind == "div" and ir[b][0] == "const":
            f.add("div_by_coef")
    if any(depth == 8 for _, depth, _ in L.lines):
        f.add("depth8")
    if p.n_param:
        f.add("param")
    if p.n_out >= 5:
        f.add("out5")
    return f


def kinds(p):
    return {k for k, *_ in p.ir()}


def has_ties(p):
    return bool(kinds(p) & set(TIES))


def select(shares=SHARES, held=HELD, seeds=SEEDS):
    """the selection rule: [(generator, seed)].  Each generator has a share of the budget (walking all three in one go, the first
    generator's frame shapes alone use the budget up); once its share is used, its walk goes on for what is not held at all and for node kinds
    not held twice"""
    count, out = {}, []
    for gen, share in shares:
        n = 0
        for seed in range(seeds):
            try:
                p = F.compile(F.from_sexpr(GENERATORS[gen](seed)))
            except F.FlowzError:
                continue                                   # (a graph the lowering refuses: an algebraic loop)
            if not p.grad_supported() or signal_gaps(f"{gen}{seed}"):
                continue
            keys = [("CR",) + strides(p)] + sorted(features(p)) + [("kind", k) for k in sorted(kinds(p))]
            if any(count.get(k, 0) < (held if n < share else 2 if k[0] == "kind" else 1) for k in keys):
                out.append((gen, seed))
                n += 1
                for k in keys:
                    count[k] = count.get(k, 0) + 1
    return out


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def draw_params(p, ns, rng):
    """per-stream coefficients as randgraphs._coef draws the literals they replace: +-[0.05, 0.45]"""
    if not p.n_param:
        return None
    v = rng.uniform(0.05, 0.45, (p.n_param, ns))
    return (v * np.where(rng.random((p.n_param, ns)) < 0.5, 1.0, -1.0)).astype(F32)


def inputs(cell, ns, T, seed):
    """grad_harness.make_inputs for a cell: x, state, params, dL/dy, dL/d(state after), the two accumulators -- none of them zero; cells
    with ABS / MIN / MAX / comparisons get the ties and specials (+-0, NaN, +-inf, equal operands) in every third stream"""
    from grad_harness import make_inputs
    p = prog(cell)
    return make_inputs(p, cell, ns, T, seed, ties=has_ties(p), draw_params=draw_params, special_every=SPECIAL_EVERY)


def shapes(cell):
    """(ns, T): one stream, a wave and one, five waves and one; a chunk and one row, a patch and one, two patches and three"""
    c, r = strides(prog(cell))
    r = r or c
    return [(ns, T) for ns in (1, 65, 321) for T in sorted({c + 1, r + 1, 2 * r + 3})]


SPECIAL_EVERY = 3                                  # cells with ties: the specials (NaN, +-inf among them) go into every third stream


def signal_gaps(cell):
    """which adjoints the GPU test's inputs leave without a signal.  With the inputs test_grad_fuzz_gpu.py draws for the longest block of
    the cell at 65 and at 321 streams (its shapes, its seeds; zero accumulators here: what the block itself contributes), every input
    wire, parameter and coefficient an adjoint reaches (Layout.has) and every state row must get a FINITE adjoint that is not zero in
    every stream that holds no NaN or infinity -- all streams, but the every third one with specials of a cell with ties -- so that a
    dropped contribution changes bits (a NaN says nothing: the comparison takes any NaN for any other).
    Returns [(ns, what, index, streams without a signal)]; select() takes no cell with gaps"""
    import adjoint_ref as A
    p = prog(cell)
    L = A.Layout(p)
    sh = shapes(cell)
    gaps = []
    for ns in (65, 321):
        T = max(t for n, t in sh if n == ns)
        x, s0, par, yb, sb, ap, ac = inputs(cell, ns, T, GPU_SEED + sh.index((ns, T)))
        assert all(np.all(a != 0) for a in (yb, sb, ap, ac, s0) if a.size) and (par is None or np.all(par != 0))
        g = A.grad(p, x, yb, s0, par, sb)
        clean = np.ones(ns, bool) if not has_ties(p) else np.arange(ns) % SPECIAL_EVERY != 0
        assert np.all(np.isfinite(x[:, clean]))
        live = lambda v: np.isfinite(v) & (v != 0)                                          # noqa: E731
        rows = []
        for i, (kind, a, _, _) in enumerate(L.ir):
            if L.has[i] and kind == "input":
                rows.append(("x wire", a, np.any(live(g["x"][:, :, a]), axis=0)))
            elif L.has[i] and kind in ("param", "const"):
                rows.append((kind, a, live(g[kind + "s"][a])))
        rows += [("state row", r, live(g["state"][r])) for r in range(L.n_state)]
        gaps += [(ns, what, k, int((~ok & clean).sum())) for what, k, ok in rows if np.any(~ok & clean)]
    return gaps


# ---- pins -----------------------------------------------------------------------------------------------------------------------
def resolved(cell):
    """what a cell's pin holds but the spills: the two symbols (None: the stream-major patch is refused) and the program's sizes"""
    p = prog(cell)
    try:
        sm = p.grad_kernel_symbol(stream_major=True)
    except F.FlowzError:
        sm = None
    return {"time_major": p.grad_kernel_symbol(), "stream_major": sm, "sizes": [p.n_in, p.n_out, p.n_state, p.n_param, p.n_const]}


def spills(cell):
    """sgpr_spills of the two kernels (JIT for gfx950; None: refused)"""
    p = prog(cell)
    out = [p.grad_resources()["sgpr_spills"]]
    try:
        out.append(p.grad_resources(stream_major=True)["sgpr_spills"])
    except F.FlowzError:
        out.append(None)
    return out


def kernel_requests():
    """(program, checkpoint_rows, stream_major) of every adjoint kernel test_grad_fuzz_gpu.py, test_grad_gpu.py and
    test_grad_stream_major_gpu.py launch: the default kernels of every cell and named graph, strides 1 and 4 where a test asks for them"""
    import grad_graphs as GG
    out = []
    named = {n: F.compile(F.from_sexpr(b())) for n, b in GG.SUPPORTED.items()}
    for p in [prog(c) for c in CELLS] + list(named.values()):
        out += [(p, 0, False), (p, 0, True)]
    for p in [prog(c) for c in STRIDE_CELLS] + [named[n] for n in ("df1_cascade6", "moog_ladder", "envelope_follower", "div_sqrt_exp")]:
        out += [(p, c, sm) for c in (1, 4) for sm in (False, True)]
    return out


def record_manifest():
    """tests/golden/grad_fuzz_kernels.fzm.gz: resolve every kernel of kernel_requests() in a process that records (FLOWZ_HIP_MANIFEST);
    needs no GPU.  build() replays every manifest under tests/golden/, so a GPU run finds the adjoint kernels built"""
    import gzip
    import subprocess
    import sys
    import tempfile
    code = ("import sys\nsys.path[:0] = [%r, %r]\nimport grad_fuzz_cells as GC\nfrom zignal_amd import flowz as F\n"
            "for p, c, sm in GC.kernel_requests():\n    try:\n        p.grad_resources(c, stream_major=sm)\n"
            "    except F.FlowzError as e:\n        print('refused:', e)\n") % (os.path.dirname(HERE), HERE)
    with tempfile.TemporaryDirectory() as td:
        raw = os.path.join(td, "manifest.fzm")
        subprocess.check_call([sys.executable, "-c", code], env=dict(os.environ, FLOWZ_HIP_MANIFEST=raw))
        with open(raw, "rb") as f, open(MANIFEST, "wb") as out:
            out.write(gzip.compress(f.read(), 9, mtime=0))
    return F.manifest_build(MANIFEST)


def load_pins():
    with open(PINS_FILE) as f:
        return json.load(f)


if __name__ == "__main__":                         # python tests/grad_fuzz_cells.py: write the pins of the library as it is (review the diff)
    picked = select()
    print("select():", picked if picked != SELECTED else "the committed list")
    pins = {}
    for cell in CELLS:
        pins[cell] = dict(resolved(cell), sgpr_spills=spills(cell))
        print(cell, pins[cell])
    with open(PINS_FILE, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in pins.items()) + "\n}\n")
    print("kernel manifest:", record_manifest())
