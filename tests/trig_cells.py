"""sin, cos and log on the kernel bodies: the graphs, the cells (graph, layout, variant, shape, the kernel name the library resolves),
their inputs, the hand-written recurrences of the three workloads, and the kernel manifest of everything the GPU tests launch.

test_trig_log_host.py checks every cell's kernel name without a GPU; test_trig_log_gpu.py runs every cell against fn_ref.run_ir with the
functions of tests/fn_ref_trig.py registered."""
import gzip
import os
import subprocess
import sys
import tempfile

import numpy as np

import fn_ref as R
import fn_ref_trig as RT
from fn_bodies import GS, L, NSP, OUT64, P3, PLAIN, SML, SMS, variant   # noqa: F401
from zignal_amd import flowz as F
from zignal_amd import workloads as W

F32, F64 = np.float32, np.float64
HERE = os.path.dirname(os.path.abspath(__file__))
MANIFEST = os.path.join(HERE, "golden", "trig_log_kernels.fzm.gz")
PINS_FILE = os.path.join(HERE, "golden", "trig_log_pins.json")
SEED = 20261018
FEED_FORWARD = ("bank", "f64lit")
OUT_F64 = ("f64lit",)
WORKLOADS = ("pm", "fold", "comp")


def all_three():
    """the crafted graph of the backward tests: a feedback through sin and cos, log behind it (its operand stays >= 0.7):
        ~( 0.5*sin(_1[_1] + _2) + 0.3*cos(2*_1[_1]) ) |= log(1.5 + _1)"""
    y1 = W.DEL(1, 1)
    loop = W.add(W.mul(W.lit(0.5), W.fn("sin", W.add(y1, W.IN(2)))), W.mul(W.lit(0.3), W.fn("cos", W.mul(W.lit(2.0), y1))))
    return W.seq(W.fb(loop), W.fn("log", W.add(W.lit(1.5), W.IN(1))))


def expr(name):
    _1, _2 = F.placeholder(1), F.placeholder(2)
    return {"bank": lambda: F.chan(F.sin(_1), F.cos(_1), F.log(_1), F.log(abs(_2)), F.sin(_1) * F.cos(_2)),
            "pm": lambda: F.from_sexpr(W.pm_operator()),
            "fold": lambda: F.from_sexpr(W.wavefolder()),
            "comp": lambda: F.from_sexpr(W.log_compressor()),
            "lds": lambda: F.seq(F.sin(_1 + 0.5 * _1[40]), ~F.log(1.5 + 0.3 * _1[23] * _1[23] + _2 * _2)),
            "pairsin": lambda: ~F.sin(0.5 * _1[1] + _2),
            "pairlog": lambda: F.seq(F.log(1.5 + _1 * _1), ~(0.5 * _1[1] + _2)),
            "f64lit": lambda: F.log(F.lit64(0.5) * (_1 + _1[3])),
            "all3": lambda: F.from_sexpr(all_three())}[name]()


_PROGS = {}


def graph(name):
    if name not in _PROGS:
        _PROGS[name] = F.compile(expr(name))
    return _PROGS[name]


# a cell: (id, graph, layout, variant, n_streams, n_samples, tile_streams, kernel name, cut, variant of the block after the cut)
_K = "fz_block_kernel_"
CELLS = []
for _g in ("bank",) + WORKLOADS:
    # time-major, one, two and four streams per lane, a ragged last lane, the second block after a cut at 37
    CELLS += [(f"{_g}-p1", _g, "rows", (1, 16, 256, 0), 1027, 77, 0, _K + "p1u16b256f0M", 37, PLAIN),
              (f"{_g}-p2", _g, "rows", (2, 2, 1024, L | GS), 1027, 77, 0, _K + "p2u2b1024f8912896RM", 37, PLAIN),
              (f"{_g}-p4", _g, "rows", (4, 1, 256, L | GS | P3), 1027, 77, 0, _K + "p4u1b256f8912928RM", 37, PLAIN),
              # lockstep, with and without the XCD step
              (f"{_g}-L", _g, "rows", (2, 2, 1024, L), 2048, 64, 0, _K + "p2u2b1024f524288", 37, PLAIN),
              (f"{_g}-LG", _g, "rows", (2, 2, 1024, L | GS), 2048, 64, 0, _K + "p2u2b1024f8912896", 37, PLAIN),
              (f"{_g}-tiles", _g, "tiles", (2, 16, 256, 0), 4096, 40, 2048, _K + "p2u16b256f0", 17, PLAIN),
              # (the bank's five output wires halve the short body's chunk)
              (f"{_g}-sm-short", _g, "sm", (1, 0, 0, SMS), 334, 300, 0, _K + ("p1u16b256f128" if _g == "bank" else "p1u32b256f128"), 132,
               (1, 8, 0, SMS) if _g == "bank" else (1, 16, 0, SMS))]
for _g in WORKLOADS:                                       # (the long-run bodies take 1-in / 1-out graphs)
    CELLS += [(f"{_g}-sm-long{U}-{ns}", _g, "sm", (1, U, 0, SML), ns, T, 0, _K + f"p1u{U}b64f384", 132, (0, 0, 0, SMS))
              for U in (64, 128) for ns, T in ((334, 300), (2, 388))]
# the pair long-run body keeps 256 staging registers next to the graph's: with the three workloads its kernel would spill, and the library
# runs the one-stream long-run body instead (fz_plan.cpp: settle_variant) -- the cells above.  Two smaller graphs reach it:
CELLS += [(f"{_g}-sm-pair{ns}", _g, "sm", (2, 64, 0, SML), ns, T, 0, _K + "p2u64b64f384", 132, (0, 0, 0, SMS))
          for _g in ("pairsin", "pairlog") for ns, T in ((334, 300), (1026, 200))]
CELLS += [("lds-free", "lds", "rows", (1, 32, 256, 0), 2048, 150, 0, _K + "p1u32b256f0", 37, PLAIN),
          ("lds-L", "lds", "rows", (1, 16, 256, L | GS), 2048, 150, 0, _K + "p1u16b256f8912896", 37, PLAIN),
          ("f64lit-p4", "f64lit", "rows", (4, 8, 256, OUT64), 2048, 64, 0, _K + "p4u8b256f64L", 37, (1, 8, 256, NSP | OUT64))]


def cell_name(prog, c):
    _, _, layout, v, ns, T, tile, *_ = c
    return prog.kernel_name(variant(v, layout), ns, T, tile)


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def edge_values():
    """+-0, subnormals, 1 and its neighbours, powers of two, +-inf, NaN, negatives (for log), |a| just below and at 2^20, the neighbours
    of multiples of pi/2"""
    one = F32(1)
    ev = [0.0, -0.0, np.finfo(F32).smallest_subnormal, -np.finfo(F32).smallest_subnormal, F32(1e-40), np.finfo(F32).tiny,
          np.nextafter(np.finfo(F32).tiny, F32(0)), one, np.nextafter(one, F32(0)), np.nextafter(one, F32(2)), -one, 0.5, 2.0, 4.0,
          F32(2.0 ** -126), F32(2.0 ** -100), F32(2.0 ** 100), F32(2.0 ** 127), np.finfo(F32).max, np.inf, -np.inf, np.nan, -2.5, -1e-30,
          F32(2.0 ** 20), np.nextafter(F32(2.0 ** 20), F32(0)), -F32(2.0 ** 20), -np.nextafter(F32(2.0 ** 20), F32(0)), F32(2.0 ** 21), F32(1e-5),
          F32(np.sqrt(0.5)), np.nextafter(F32(np.sqrt(0.5)), F32(1)), F32(np.sqrt(2.0)), np.nextafter(F32(np.sqrt(2.0)), F32(1))]
    for k in (1, 2, 3, 4, 5, 8, 100, 1001, 333333):
        m = F32(k * (np.pi / 2))
        ev += [m, np.nextafter(m, F32(0)), np.nextafter(m, F32(np.inf)), -m]
    return np.asarray(ev, F32)


def accuracy_sample(n=1 << 18, seed=SEED):
    """the committed sample of the accuracy test: n random values -- a third random bit patterns, a third in [-2^20, 2^20], a third in
    [-8, 8] -- and the edge values"""
    rng = np.random.default_rng(seed)
    k = n // 3
    bits = rng.integers(0, 1 << 32, k, dtype=np.uint64).astype(np.uint32).view(F32)
    wide = rng.uniform(-2.0 ** 20, 2.0 ** 20, k).astype(F32)
    near = rng.uniform(-8, 8, n - 2 * k).astype(F32)
    return np.concatenate([bits, wide, near, edge_values()])


def mixed_edges(T, ns, w, seed):
    """feed-forward graphs: random bit patterns and values in sin's domain, the edge values in the first and the last 256 streams"""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 1 << 32, (T, ns, w), dtype=np.uint64).astype(np.uint32).view(F32)
    dom = rng.random((T, ns, w)) < 0.6
    x = np.where(dom, rng.uniform(-40, 40, (T, ns, w)).astype(F32), x)
    ev = edge_values()
    for lo in (0, max(ns - 256, 0)):
        n = min(256, ns - lo)
        t, s, k = np.meshgrid(np.arange(T), np.arange(n), np.arange(w), indexing="ij")
        x[:, lo:lo + n] = ev[(t * 7 + s * 3 + k * 11) % len(ev)]
    return x


def frames(name, prog, ns, T):
    """(float32 frames [T, ns, slots], params [n_param, ns] or None) of one graph at one shape; the recursive graphs get finite inputs
    that keep their state finite"""
    seed = SEED + 1000 * ns + T + sum(map(ord, name))
    if name in FEED_FORWARD:
        return mixed_edges(T, ns, prog.n_in, seed), None
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((T, ns, max(prog.n_in, 1))) * 0.7).astype(F32)
    params = rng.uniform(0.001, 0.8, (prog.n_param, ns)).astype(F32) if prog.n_param else None
    return x, params


# ---- the workloads from their equations -------------------------------------------------------------------------------------------
def pm_operator_ref(x, inc, index=W.PM_INDEX):
    x, inc = np.asarray(x, F32), np.asarray(inc, F32)
    ph = np.zeros(x.shape[1], F32)
    out = np.empty_like(x)
    for t in range(x.shape[0]):
        p = ph + inc
        ph = p - W.PM_TWO_PI * np.where(p >= W.PM_PI, F32(1), F32(0))
        out[t] = RT.sin(ph + F32(index) * x[t])
    return out


def wavefolder_ref(x, a=W.FOLD_POLE, g=W.FOLD_GAIN):
    x = np.asarray(x, F32)
    e = np.zeros(x.shape[1], F32)
    out = np.empty_like(x)
    for t in range(x.shape[0]):
        e = e + F32(a) * (x[t] - e)
        out[t] = RT.sin(F32(g) * e)
    return out


def log_compressor_ref(x, slope=W.COMP_SLOPE, threshold=W.COMP_THRESHOLD, eps=W.COMP_EPS):
    x = np.asarray(x, F32)
    env = R.envelope_follower_ref(x, W.ENV_ATTACK, W.ENV_RELEASE)
    with np.errstate(all="ignore"):
        return R.exp(R.fmin(np.zeros_like(x), F32(slope) * (F32(threshold) - RT.log(env + F32(eps))))) * x


def recurrence(name, x, params):
    x = x[..., 0]
    if name == "pm":
        return pm_operator_ref(x, params[0])
    return wavefolder_ref(x) if name == "fold" else log_compressor_ref(x)


# ---- the kernels of the GPU tests --------------------------------------------------------------------------------------------
GRAD_GRAPHS = ("all3", "pm")
PCM_SHAPES = {"rows": (1027, 40), "sm": (66, 136, 8)}


def resolve_kernels():
    """resolve (build or find in the cache) every kernel test_trig_log_gpu.py launches; needs no GPU"""
    for c in CELLS:
        _, name, layout, v, ns, T, tile, _, cut, after = c
        p = graph(name)
        for vv in (v, after, PLAIN if name not in OUT_F64 else (1, 8, 256, NSP | OUT64)):
            lay = layout if vv is not PLAIN and vv[3] & NSP == 0 else "rows"
            for rows in (T, cut, T - cut):
                p.build(variant(vv, lay), ns, rows, tile if lay == "tiles" else 0)
    fold = graph("fold")
    for out in ("int16", "float32"):
        fold.pcm16_resources("int16", out, PCM_SHAPES["rows"][0])
    fold.pcm16_stream_major_resources("int16", "int16")
    fold.build(F.make_variant(*PLAIN), PCM_SHAPES["rows"][0], PCM_SHAPES["rows"][1])
    fold.build(variant((0, 0, 0, 0), "sm"), PCM_SHAPES["sm"][0], PCM_SHAPES["sm"][1] - PCM_SHAPES["sm"][2])
    for name in GRAD_GRAPHS:
        p = graph(name)
        p.build(F.make_variant(*PLAIN), 130, 37)
        for c in (0, 4):
            for sm in (False, True):
                p.grad_resources(c, stream_major=sm)


def record_manifest():
    """tests/golden/trig_log_kernels.fzm.gz: resolve_kernels() in a process that records (FLOWZ_HIP_MANIFEST).  build() replays every
    manifest under tests/golden/, so a GPU run finds these kernels built"""
    code = "import sys\nsys.path[:0] = [%r, %r]\nimport trig_cells as TC\nTC.resolve_kernels()\n" % (os.path.dirname(HERE), HERE)
    with tempfile.TemporaryDirectory() as td:
        raw = os.path.join(td, "manifest.fzm")
        subprocess.check_call([sys.executable, "-c", code], env=dict(os.environ, FLOWZ_HIP_MANIFEST=raw))
        with open(raw, "rb") as f, open(MANIFEST, "wb") as out:
            out.write(gzip.compress(f.read(), 9, mtime=0))
    return F.manifest_build(MANIFEST)


if __name__ == "__main__":                         # PYTHONPATH=. python tests/trig_cells.py: the kernel names as resolved now, then the manifest
    for c in CELLS:
        got = cell_name(graph(c[1]), c)
        print(("ok   " if got == c[7] else "DIFF ") + c[0], got)
    print(record_manifest())
