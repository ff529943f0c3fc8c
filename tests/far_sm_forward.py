"""Graphs, geometry, shapes and kernels of the stream-major far FORWARD tests (fz_run_block_far_stream_major: graphs with delay lines
deeper than 256 samples, rings in HBM, on [batch, time] buffers as they lie): the graphs; the static rule that chooses the group
rows G, the patch rows R and the workgroup, restated; the shapes built from each graph's own D, R and G; the inputs, the oracle's
and the time-major kernel's answers, computed once; the random graphs; and the kernels the GPU tests launch
(tests/golden/far_sm_forward_kernels.fzm.gz)."""
import functools
import gzip
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

import delay_cells as DC
import far_grad_graphs as FG
import randgraphs as R
from grad_harness import up4
from grad_host_harness import LDS_BYTES
from graphs import DEL, IN, add, chan, cmp, fb, lit, mul
from oracle import flowz_oracle as O

F32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
MANIFEST = os.path.join(HERE, "golden", "far_sm_forward_kernels.fzm.gz")
FAR_SM = (1 << 18) | 1                                            # FZ_VF_FAR_SM (fz_internal.hpp)
SM = DC.SM


def two_out():
    """(_1 + 0.5*_1[_300], 0.25*_1): two output wires, one of which reads a far line"""
    return chan(add(IN(1), mul(lit(0.5), DEL(1, 300))), mul(lit(0.25), IN(1)))


def gated():
    """~(0.6*_1[_270]*(_1[_270] < 0.5) + _2): a comparison node gates the loop through a far line"""
    return fb(add(mul(mul(lit(0.6), DEL(1, 270)), cmp("lt", DEL(1, 270), lit(0.5))), IN(2)))


# name -> s-expression builder: the eight graphs of the far backward, three delay-cell templates, two outputs, a comparison
GRAPHS = dict(FG.FARS)
GRAPHS.update({"fb257": lambda: DC.sexpr("fb", (257,)), "taps257_128_9_3": lambda: DC.sexpr("taps", (257, 128, 9, 3)),
               "mixed3_40_300": lambda: DC.sexpr("mixed", (3, 40, 300)), "two_out": two_out, "gated": gated})
DEEPEST = dict(FG.DEEPEST, fb257=257, taps257_128_9_3=257, mixed3_40_300=300, two_out=300, gated=270)
NOT_IN_ORACLE = ("far_adjacent", "far_mixed")                     # a graph function (tanh), a uniform coefficient: oracle() says what holds them
AUTOGRAD = ("far257", 130, 300)                                   # autograd.run_far(stream_major=True): graph, streams, rows
PYTHON_CALL = ("far_comb", 65, 304)                               # the [n_streams, rows] call: graph, streams, rows
NO_FAR = ("fb", (40,))                                            # a graph without a far line at PYTHON_CALL's shape: delay_cells template, depths
RANDOM_SEEDS, RANDOM_SHAPE = range(9200, 9240), (136, 620)        # the make_deep seeds and the shape of test_delay_lines_gpu.py
RANDOM_KEPT = 12                                                  # of them: deepest delay beyond 256 and accepted (the host test counts)

_progs = {}


def prog(name):
    from zignal_amd import flowz as F
    if name not in _progs:
        _progs[name] = F.compile(F.from_sexpr(GRAPHS[name]()))
    return _progs[name]


# ---- the static rule, restated (zignal_amd/csrc/fz_far_sm.cpp: far_sm_group_rows, far_sm_geometry) -----------------------------------------
READ_REGS, MIN_ROWS = 64, 16


def far_reads(p):
    """the delays the kernel reads from rings in HBM (fr_n of the generated body)"""
    m = re.search(r"fr_n\[\d+\] = \{([^}]*)\}", p.far_stream_major_source())
    return [int(v.strip().rstrip("u")) for v in m.group(1).split(",")]


def lds_slots(p):
    return int(re.search(r"#define FZ_LDS_SLOTS (\d+)", p.far_stream_major_source()).group(1))


def lds_bytes(p, block, rows):
    """rings [slot][lane], then one patch per wave of 64 rows of [rows x n_in floats][rows x n_out floats][16 bytes]"""
    return 4 * lds_slots(p) * block + (block // 64) * 64 * (4 * rows * (p.n_in + p.n_out) + 16)


def rule(p):
    """(G, R, block) of the static rule, or (G, MIN_ROWS, 0) when nothing fits"""
    reads = far_reads(p)
    assert min(reads) >= 9
    cap, G = min(16, min(reads) // 2), 4
    while G * 2 <= cap:
        G *= 2
    while G > 4 and 2 * G * len(reads) > READ_REGS:
        G //= 2
    R0 = MIN_ROWS
    while R0 * max(p.n_in, p.n_out, 1) < 32:
        R0 *= 2
    for times in (2, 1):
        rows = R0
        while rows >= MIN_ROWS:
            for block in (256, 128, 64):
                if times * lds_bytes(p, block, rows) <= LDS_BYTES:
                    return G, rows, block
            rows //= 2
    return G, MIN_ROWS, 0


SYMBOL = re.compile(r"fz_far_sm_kernel_g(\d+)r(\d+)b(\d+)_g[0-9a-f]{8}$")


def geometry(p):
    """(G, R, block): the kernel symbol names them"""
    m = SYMBOL.match(p.far_stream_major_kernel_symbol())
    assert m, p.far_stream_major_kernel_symbol()
    return tuple(int(v) for v in m.groups())


# ---- shapes, from each graph's own D, R and G -------------------------------------------------------------------------------------------------
def streams_of(name):
    return (1, 63, 64, 65) if name == "far1031" else (1, 63, 64, 65, 257)


def rows_of(name):
    G, rows, _ = geometry(prog(name))
    D = DEEPEST[name]
    return sorted(T for T in {1, 3, G - 1, G, G + 1, rows - 1, rows, rows + 1, D - 1, D, D + 1, 2 * D + 3} if name != "far1031" or T <= D + 1)


def chain_rows(name):
    """the two window lengths of the chained test: up4(D - 2) rows, then D + 5"""
    return up4(DEEPEST[name] - 2), DEEPEST[name] + 5


def time_major_shapes(name):
    """(streams, rows) of every time-major run_block launch the GPU tests compare with"""
    D, (a, b) = DEEPEST[name], chain_rows(name)
    shapes = {(ns, D + 1) for ns in streams_of(name)} | {(65, T) for T in rows_of(name)} | {(65, a), (65, b), (65, a + b)}
    return sorted(shapes | {shape[1:] for shape in (AUTOGRAD, PYTHON_CALL) if shape[0] == name})


# ---- inputs and expected answers --------------------------------------------------------------------------------------------------------------
def params_of(p, ns, seed):
    return np.random.default_rng(seed + 1).uniform(0.3, 0.8, (p.n_param, ns)).astype(F32) if p.n_param else None


@functools.lru_cache(maxsize=8)
def _draw(name, ns, T, seed):
    p = prog(name)
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((T, ns, p.n_in)) * 0.5).astype(F32)
    s0 = (rng.standard_normal((p.n_state, ns)) * 0.1).astype(F32)
    for a in (x, s0):
        a.setflags(write=False)
    return x, s0, params_of(p, ns, seed)


def draw(name, ns, T, seed=5, p0=None, zero=False):
    """x [T, ns, n_in], the state before the block (random line rows, or zeros; every far line's phase row p0 modulo its depth, default
    D - 3: the ring wraps inside the first groups), params"""
    x, s0, par = _draw(name, ns, T, seed)
    s0 = np.zeros_like(s0) if zero else s0.copy()
    p0 = DEEPEST[name] - 3 if p0 is None else p0
    for _, d, pr in FG.far_rows(prog(name)):
        s0[pr] = F32(p0 % d)
    return x, s0, par


@functools.lru_cache(maxsize=8)
def oracle(name, ns, T, seed=5):
    """the oracle's output on draw()'s x from a zero state (what a state of zero slots gives at any phase), computed once.  The oracle
    has no spelling for the graph functions (far_adjacent's tanh) and for uniform coefficients (far_mixed's): such a graph is held to
    the IR evaluator with the functions' restatements, tests/fn_ref.py, as tests/test_graph_functions_gpu.py holds them"""
    x, _, par = _draw(name, ns, T, seed)
    try:
        want = O.compile(GRAPHS[name](), ns, params=par).run(x)
    except O.GraphError:
        import fn_ref
        assert name in NOT_IN_ORACLE, name
        want = fn_ref.run_ir(prog(name), x, par)[0]
    want.setflags(write=False)
    return want


# ---- the random graphs ---------------------------------------------------------------------------------------------------------------------------
def random_graphs():
    """(seed, s-expression, n_in, n_out) of the make_deep graphs of RANDOM_SEEDS the oracle takes whose deepest delay passes 256 and
    which the new call accepts; no other seed is left out"""
    from zignal_amd import flowz as F
    out = []
    for seed in RANDOM_SEEDS:
        g, n_in, n_out = R.make_deep(seed)
        try:
            if O.input_arity(g) != n_in or O.output_arity(g) != n_out:
                continue
            O.compile(g, 1)
        except O.GraphError:
            continue
        p = F.compile(F.from_sexpr(g))
        if p.max_delay > DC.LDS_MAX and p.far_stream_major_supported():
            out.append((seed, g, n_in, n_out))
    return out


# ---- the kernels the GPU tests launch: tests/golden/far_sm_forward_kernels.fzm.gz -----------------------------------------------------------
def resolve():
    """what a recording process calls (FLOWZ_HIP_MANIFEST set): the far stream-major kernel of every graph and of every random graph,
    and the time-major forward kernels they are compared with"""
    from zignal_amd import flowz as F
    for n in sorted(GRAPHS):
        prog(n).far_stream_major_resources()
        for ns, rows in time_major_shapes(n):
            prog(n).build(None, ns, rows)
    for _, g, _, _ in random_graphs():
        F.compile(F.from_sexpr(g)).far_stream_major_resources()
    F.compile(F.from_sexpr(DC.sexpr(*NO_FAR))).build(F.make_variant(0, 0, 0, SM), PYTHON_CALL[1], PYTHON_CALL[2])


def record_manifest():
    """record the manifest with the library as it is; needs no GPU.  build() replays every manifest under tests/golden/, so a GPU run
    finds them built.  By hand: PYTHONPATH=. python tests/far_sm_forward.py"""
    from zignal_amd import flowz as F
    code = "import sys\nsys.path[:0] = [%r, %r]\nimport far_sm_forward as FF\nFF.resolve()\n" % (os.path.dirname(HERE), HERE)
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


if __name__ == "__main__":                         # record the kernel manifest of the library as it is
    print("kernel manifest:", record_manifest())
