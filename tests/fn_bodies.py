"""The graph-function body matrix: function graphs, the kernel bodies explicit variants reach with them, and the inputs they run on.

CELLS names, for every cell, the graph, the frame layout, the variant, the shape and the kernel name the library resolves for it, and the
body that continues the block after the cut (the second of two chained blocks).  test_graph_functions_host.py checks every name without a
GPU (so a planner change that moves a cell to another body fails on a CPU), test_graph_functions_bodies_gpu.py runs every cell against
the IR evaluator of tests/fn_ref.py.  DEFAULT_BODIES: the body the library picks by itself for these graphs at full size."""
import numpy as np

import fn_ref as R
from oracle import flowz_oracle as O
from test_graph_functions_gpu import edge_values, random_bits
from zignal_amd import flowz as F
from zignal_amd import workloads as W

F32, F64 = np.float32, np.float64
C = F.C
L, GS, P3, NSP = C.FZ_VF_LOCKSTEP, C.FZ_VF_GRID_SYNC, C.FZ_VF_PREFETCH3, C.FZ_VF_NO_STAGE_PACK
SM, SML, SMS, OUT64 = C.FZ_VF_STREAM_MAJOR, C.FZ_VF_SM_LONG, C.FZ_VF_SM_SHORT, C.FZ_VF_OUT_F64
PLAIN = (1, 8, 256, NSP)                       # the kernel every cell's state is compared with
SEED = 20241015


FEED_FORWARD = ("two", "four", "bank", "f64lit")          # (no loop: every class of input value can go in, none sticks)
OUT_F64 = ("f64lit",)                                      # (run with float64 output frames)


def graph(name):
    """the program of a matrix graph"""
    _1, _2 = F.placeholder(1), F.placeholder(2)
    moog = F.from_sexpr(W.moog_ladder())
    e = {"moog": lambda: moog,
         "soft": lambda: F.from_sexpr(W.soft_clip_cascade(4)),
         "env": lambda: F.from_sexpr(W.envelope_follower()),
         "two": lambda: F.par(F.tanh(1.5 * _1), F.sqrt(abs(_1 + _1[2]))),
         "four": lambda: F.par(F.tanh(_1), F.tanh(0.5 * _1 + _1[1]), F.tanh(F.tanh(2.0 * _1) - _1[2]), F.tanh(_1 * _1[1])),
         "bank": lambda: F.chan(F.abs(_1), F.sqrt(_1), F.exp(_1), F.tanh(_1), F.min(_1, _2), F.max(_1, _2)),
         "lds": lambda: F.seq(F.tanh(_1 + 0.5 * _1[40]), ~F.tanh(0.7 * _1[23] + _2)),
         "ldscomb": lambda: F.from_sexpr(W.lds_ring_comb()),
         "far": lambda: F.seq(moog, _1 + 0.5 * _1[300]),
         "mod": lambda: ~F.tanh(F.modulator(0) * _1[1] + _2),
         "f64lit": lambda: F.tanh(F.lit64(0.5) * (_1 + _1[3])),
         "typed": lambda: ~F.tanh(0.9 * _1[1] + _2)}[name]()
    prog = F.compile(e, in_dtypes=["f64"]) if name == "typed" else F.compile(e)
    return prog


# a cell: (id, graph, layout, variant, n_streams, n_samples, tile_streams, kernel name, cut, variant of the block after the cut)
#   layouts: "rows" (time-major [T, ns, w]), "tiles" (stream-tiled), "sm" (stream-major [ns, T, w]: the variant without FZ_VF_STREAM_MAJOR)
_K = "fz_block_kernel_"
CELLS = [
    # the lockstep frame kernel: two streams per lane with the XCD step, four with a third buffer, the library's own four-stream body
    ("moog-p2L", "moog", "rows", (2, 2, 1024, L | GS), 2048, 300, 0, _K + "p2u2b1024f8912896", 37, PLAIN),
    ("soft-p2L", "soft", "rows", (2, 2, 1024, L | GS), 2048, 300, 0, _K + "p2u2b1024f8912896", 37, PLAIN),
    ("env-p2L", "env", "rows", (2, 2, 1024, L | GS), 2048, 300, 0, _K + "p2u2b1024f8912896", 37, PLAIN),
    ("moog-p4Lp3", "moog", "rows", (4, 1, 256, L | P3), 2048, 300, 0, _K + "p4u1b256f524320", 37, PLAIN),
    ("soft-p4Lp3", "soft", "rows", (4, 1, 256, L | P3), 2048, 300, 0, _K + "p4u1b256f524320", 37, PLAIN),
    ("env-p4Lp3", "env", "rows", (4, 1, 256, L | P3), 2048, 300, 0, _K + "p4u1b256f524320", 37, PLAIN),
    ("moog-p4LGp3", "moog", "rows", (4, 1, 1024, L | GS | P3), 2048, 300, 0, _K + "p4u1b1024f8912928", 37, PLAIN),
    # ragged stream counts: the last lane's streams run past the end of the rows
    ("moog-ragged", "moog", "rows", (4, 1, 256, L | GS | P3), 1027, 300, 0, _K + "p4u1b256f8912928RM", 37, PLAIN),
    ("soft-ragged", "soft", "rows", (2, 2, 1024, L | GS), 1027, 300, 0, _K + "p2u2b1024f8912896RM", 37, PLAIN),
    ("env-ragged", "env", "rows", (4, 1, 1024, L | GS | P3), 1027, 300, 0, _K + "p4u1b1024f8912928RM", 37, PLAIN),
    # a sample-rate modulator inside tanh
    ("mod-p4LGp3", "mod", "rows", (4, 1, 1024, L | GS | P3), 2048, 300, 0, _K + "p4u1b1024f8912928", 37, PLAIN),
    ("mod-p2", "mod", "rows", (2, 16, 256, 0), 2048, 300, 0, _K + "p2u16b256f0", 37, PLAIN),
    # stream tiles: free-running and in lockstep
    ("moog-tiles", "moog", "tiles", (2, 16, 256, 0), 4096, 160, 2048, _K + "p2u16b256f0", 37, PLAIN),
    ("moog-tilesL", "moog", "tiles", (2, 2, 1024, L | GS), 4096, 160, 2048, _K + "p2u2b1024f8912896", 37, PLAIN),
    ("soft-tilesL", "soft", "tiles", (2, 2, 1024, L | GS), 4096, 160, 2048, _K + "p2u2b1024f8912896", 37, PLAIN),
    ("env-tilesL", "env", "tiles", (2, 2, 1024, L | GS), 4096, 160, 2048, _K + "p2u2b1024f8912896", 37, PLAIN),
    # lane groups: pairs (2-wire frames, four streams per lane), singles (4-wire frames, two streams per lane); wide lockstep
    ("two-pairs", "two", "rows", (4, 8, 256, 0), 2048, 300, 0, _K + "p4u8b256f0L", 37, PLAIN),
    ("two-pairsL", "two", "rows", (4, 1, 1024, L | GS | P3), 2048, 300, 0, _K + "p4u1b1024f8912928L", 37, PLAIN),
    ("typed-pairs", "typed", "rows", (4, 8, 256, 0), 2048, 300, 0, _K + "p4u8b256f0L", 37, PLAIN),
    ("typed-pairsL", "typed", "rows", (4, 1, 1024, L | GS | P3), 2048, 300, 0, _K + "p4u1b1024f8912928L", 37, PLAIN),
    ("f64lit-pairs", "f64lit", "rows", (4, 8, 256, OUT64), 2048, 300, 0, _K + "p4u8b256f64L", 37, (1, 8, 256, NSP | OUT64)),
    ("f64lit-pairsL", "f64lit", "rows", (4, 1, 1024, L | GS | P3 | OUT64), 2048, 300, 0, _K + "p4u1b1024f8912992L", 37, (1, 8, 256, NSP | OUT64)),
    ("four-singles", "four", "rows", (2, 8, 256, 0), 2048, 300, 0, _K + "p2u8b256f0S", 37, PLAIN),
    ("four-wide", "four", "rows", (1, 3, 1024, L | GS), 2048, 300, 0, _K + "p1u3b1024f8912896", 37, PLAIN),
    ("bank-p2L", "bank", "rows", (2, 2, 1024, L | GS), 2048, 300, 0, _K + "p2u2b1024f8912896", 37, PLAIN),
    ("bank-p4Lp3", "bank", "rows", (4, 1, 256, L | GS | P3), 2048, 300, 0, _K + "p4u1b256f8912928", 37, PLAIN),
    ("bank-p4", "bank", "rows", (4, 8, 256, 0), 2048, 300, 0, _K + "p4u8b256f0", 37, PLAIN),
    # LDS rings: free-running, in lockstep, and the lockstep step-down (one row per chunk, three buffers)
    ("lds-free", "lds", "rows", (1, 32, 256, 0), 2048, 300, 0, _K + "p1u32b256f0", 37, PLAIN),
    ("lds-L", "lds", "rows", (1, 16, 256, L | GS), 2048, 300, 0, _K + "p1u16b256f8912896", 37, PLAIN),
    ("lds-Lp3", "lds", "rows", (1, 1, 256, L | GS | P3), 2048, 300, 0, _K + "p1u1b256f8912928", 37, PLAIN),
    ("ldscomb-Lp3", "ldscomb", "rows", (1, 1, 256, L | GS | P3), 2048, 300, 0, _K + "p1u1b256f8912928", 37, PLAIN),
    # an HBM ring behind the ladder: free-running at every lane packing, and in lockstep
    ("far-p1", "far", "rows", (1, 16, 256, 0), 2048, 600, 0, _K + "p1u16b256f0", 37, PLAIN),
    ("far-p2", "far", "rows", (2, 16, 256, 0), 2048, 600, 0, _K + "p2u16b256f0", 37, PLAIN),
    ("far-p4", "far", "rows", (4, 8, 256, 0), 2048, 600, 0, _K + "p4u8b256f0", 37, PLAIN),
    ("far-p4L", "far", "rows", (4, 2, 1024, L | GS), 2048, 600, 0, _K + "p4u2b1024f8912896", 37, PLAIN),
    # stream-major buffers: the short-chunk body, the one-stream long-run body, the pair long-run body (tails off the 128-sample phases)
    ("moog-sm-short", "moog", "sm", (1, 0, 0, SMS), 334, 300, 0, _K + "p1u32b256f128", 132, (0, 0, 0, SML)),
    ("typed-sm-short", "typed", "sm", (1, 0, 0, SMS), 334, 300, 0, _K + "p1u32b256f128", 132, (1, 16, 0, SMS)),
] + [
    (f"{g}-sm-long{U}", g, "sm", (1, U, 0, SML), ns, T, 0, _K + f"p1u{U}b64f384", 132, (0, 0, 0, SMS))
    for g in ("moog", "soft", "env") for U, ns, T in ((64, 334, 300), (128, 2, 388))
] + [
    (f"{g}-sm-pair{ns}", g, "sm", (2, 64, 0, SML), ns, T, 0, _K + "p2u64b64f384", 132, (0, 0, 0, SMS))
    for g in ("moog", "soft", "env") for ns, T in ((334, 300), (2, 388), (1026, 200))
]

# the library's own choice (no variant) for these graphs: (graph, n_streams, n_samples, tile_streams, stream-major, kernel name)
DEFAULT_BODIES = [
    ("moog", 1 << 19, 4096, 0, True, _K + "p2u64b64f384"),
    ("moog", 1 << 20, 4096, 0, True, _K + "p2u64b64f384"),
    ("soft", 1 << 20, 4096, 0, True, _K + "p2u64b64f384"),
    ("moog", 1 << 20, 128, 0, True, _K + "p1u32b256f128"),
    ("env", 1 << 20, 128, 0, True, _K + "p1u32b256f128"),
    ("moog", 1 << 19, 4096, 0, False, _K + "p2u2b1024f8912896"),
    ("soft", 1 << 19, 4096, 0, False, _K + "p2u2b1024f8912896"),
    ("env", 1 << 19, 4096, 0, False, _K + "p2u2b1024f8912896"),
    ("moog", 1 << 20, 4096, 8192, False, _K + "p2u2b1024f8912896"),
    ("soft", 1 << 20, 4096, 8192, False, _K + "p2u2b1024f8912896"),
    ("env", 1 << 20, 4096, 8192, False, _K + "p2u2b1024f8912896"),
    ("moog", (1 << 20) + 1, 4096, 0, False, _K + "p4u1b1024f8912928M"),
    ("soft", (1 << 20) + 1, 4096, 0, False, _K + "p4u1b1024f8912928M"),
    ("env", (1 << 20) + 1, 4096, 0, False, _K + "p4u1b1024f8912928M"),
    ("lds", 1 << 20, 4096, 0, False, _K + "p1u16b256f8912896"),
    ("lds", 1 << 27, 4096, 0, False, _K + "p1u1b256f8912928"),
    ("ldscomb", 1 << 27, 4096, 0, False, _K + "p1u1b256f8912928"),
    ("far", 1 << 20, 4096, 0, False, _K + "p4u2b1024f8912896"),
    ("two", 1 << 20, 4096, 0, False, _K + "p4u1b1024f8912928L"),
    ("four", 1 << 20, 4096, 0, False, _K + "p1u3b1024f8912896"),
    ("four", 1 << 20, 4096, 0, True, _K + "p1u32b256f128"),
    ("typed", 1 << 20, 4096, 0, False, _K + "p4u1b1024f8912928L"),
    ("typed", 1 << 20, 4096, 0, True, _K + "p1u32b256f128"),
    ("mod", 1 << 20, 4096, 0, False, _K + "p4u1b1024f8912928"),
]


def variant(v, layout="rows"):
    return F.make_variant(v[0], v[1], v[2], v[3] | (SM if layout == "sm" else 0))


def cell_name(prog, c):
    _, _, layout, v, ns, T, tile, *_ = c
    return prog.kernel_name(variant(v, layout), ns, T, tile)


def default_name(prog, ns, T, tile, sm, out_f64=False):
    return prog.kernel_name(F.make_variant(0, 0, 0, (SM if sm else 0) | (OUT64 if out_f64 else 0)), ns, T, tile)


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def cutoffs(ns, seed):
    return (0.05 + 0.6 * np.random.default_rng(seed).random(ns)).astype(F32)


def mixed_edges(T, ns, w, seed):
    """feed-forward graphs: bit patterns over the whole range (random_bits), and in the first and the last 256 streams every class of edge
    value -- NaN, +-inf, +-0, subnormals, tanh's switch point and its neighbours, exp's overflow thresholds -- placed so that the streams
    (and wires) of one lane, pair or quad carry different classes at every sample"""
    x = random_bits(F32, (T, ns, w), seed)
    ev = edge_values(F32)
    sw = F32(0.55)
    ev = np.concatenate([ev, [np.nextafter(sw, F32(0)), np.nextafter(sw, F32(1)), -np.nextafter(sw, F32(1)), F32(R.TANH_C[F32]["sw"]),
                              np.nextafter(F32(R.TANH_C[F32]["sw"]), F32(0)), F32(R.EXP_C[F32]["xmax"]), np.nextafter(F32(R.EXP_C[F32]["xmax"]), F32(np.inf))]]).astype(F32)
    rng = np.random.default_rng(seed + 1)
    for lo in (0, max(ns - 256, 0)):
        n = min(256, ns - lo)
        t, s, k = np.meshgrid(np.arange(T), np.arange(n), np.arange(w), indexing="ij")
        cls = (t * 7 + s * 3 + k * 11) % len(ev)
        v = ev[cls]
        finite = rng.random((T, n, w)) < 0.3                  # ... and finite, in-range values in between
        v = np.where(finite & (s % 2 == 1), (rng.standard_normal((T, n, w)) * 2).astype(F32), v)
        x[:, lo:lo + n] = v
    return x


def stateful_input(name, T, ns, w, seed):
    """recursive graphs: synthetic noise x 3 (the ladder and the clipper driven into saturation) with edge values in a few streams -- a NaN
    next to a finite stream of the same lane, an infinity, -0 and subnormals -- at a sample inside the first chunk"""
    x = (O.synth_input(seed, np.arange(ns), T, n_wires=w) * 3).astype(F32)
    if name == "typed":
        return x
    row = min(5, T - 1)
    for s, v in zip((5, 9, 10, 13, 14, 17), (np.nan, np.inf, -np.inf, -0.0, np.finfo(F32).smallest_subnormal, 0.55)):
        if s < ns:
            x[row, s, 0] = v
    return x


def frames(name, prog, ns, T):
    """(float32 frames [T, ns, slots], params [n_param, ns] or None, modulator rows [n_mod, T] or None) of one graph at one shape"""
    seed = SEED + 1000 * ns + T + sum(map(ord, name))
    if name == "typed":                                        # a double wire whose values are no float32 values
        a = stateful_input(name, T, ns, 1, seed)[..., 0].astype(F64)
        a *= 1 + np.ldexp(np.random.default_rng(seed).random((T, ns)), -30)
        a[3, 5], a[4, 6], a[7, 9] = np.nan, np.inf, -0.0
        x = F.pack_typed([a], ["f64"])
    elif name in FEED_FORWARD:
        x = mixed_edges(T, ns, prog.n_in, seed)
    else:
        x = stateful_input(name, T, ns, max(prog.n_in, 1), seed)
    params = cutoffs(ns, seed)[None] if prog.n_param else None
    mod = np.random.default_rng(seed + 2).uniform(-0.95, 0.95, (prog.n_mod, T)).astype(F32) if prog.n_mod else None
    return x, params, mod
