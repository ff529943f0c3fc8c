"""The random-graph body matrix: the seeded graphs of tests/randgraphs.py on every body of the forward block kernel.

A cell is one random graph (family, seed) on one kernel body (frame layout, variant, shape).  The cells are not written down: select() walks
each family's seed range in order, per body, and keeps the first K seeds that the oracle compiles, whose inputs can tell a wrong kernel from
a right one (discriminates()), and that the library resolves and builds without refusal.  tests/golden/fuzz_bodies_pins.json holds what that
walk gave -- family, seed, layout, variant, shape, tile, the kernel name, the row of the cut and the body after it -- and CELLS is read
from it; test_fuzz_bodies_host.py reruns the walk and every name without a GPU (so a planner change that moves a cell to another body
fails on a CPU), test_fuzz_bodies_gpu.py runs every cell against oracle.flowz_oracle bit for bit.  UNREACHABLE names every (family, body)
the planner refuses outright.  `PYTHONPATH=. python tests/fuzz_bodies.py` rewrites the pins of the library as it is (review the diff) and
records tests/golden/fuzz_bodies_kernels.fzm.gz, without a GPU.  tools/fuzz_gpu.py draws its variants from BODIES."""
import gzip
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

import randgraphs as R
from oracle import flowz_oracle as O
from zignal_amd import flowz as F

F32, F64 = np.float32, np.float64
C = F.C
L, GS, P3, NSP = C.FZ_VF_LOCKSTEP, C.FZ_VF_GRID_SYNC, C.FZ_VF_PREFETCH3, C.FZ_VF_NO_STAGE_PACK
SM, SML, SMS, OUT64 = C.FZ_VF_STREAM_MAJOR, C.FZ_VF_SM_LONG, C.FZ_VF_SM_SHORT, C.FZ_VF_OUT_F64
PLAIN = (1, 8, 256, NSP)                       # the kernel every cell's state is compared with, and the body behind the cut of a rows cell
HERE = os.path.dirname(os.path.abspath(__file__))
PINS_FILE = os.path.join(HERE, "golden", "fuzz_bodies_pins.json")
MANIFEST = os.path.join(HERE, "golden", "fuzz_bodies_kernels.fzm.gz")
REG_MAX, LDS_MAX = 8, 256                      # kRegMaxDepth, kLdsMaxDepth (fz_internal.hpp)
MAX_LDS_BYTES = 160 * 1024

# family -> (generator, first seed).  Ranges of WALK seeds, apart from one another and from what test_fuzz_graphs.py (0 .. 7059) and
# test_delay_lines_*.py (9000 .. 9239) use.  "tin": the typed graphs once more, compiled with input types (fz_compile_typed)
FAMILIES = {"plain": (R.make, 20000), "cmp": (R.make_cmp, 22000), "typed": (R.make_typed, 24000), "deep": (R.make_deep, 26000),
            "tin": (R.make_typed, 28000)}
TABLE_FAMILIES = ("plain", "cmp", "typed", "deep")
WALK = 400                                     # seeds of a family's range
K_ROWS, K_SM = 4, 3                            # cells per (family, body): time-major and tiled bodies, stream-major bodies
CUT_ROWS, CUT_SM = 37, 133                     # the row a chained run cuts the block at (odd; off every chunk and phase boundary)
# (family, body) -> K where a condition of the matrix needs more cells than the body's K: the first complex graph of the typed range is its tenth
# usable seed, and the typed cells have to hold a double, a complex and a cdouble graph
K_MORE = {("typed", "free-p2"): 10}
COMPARISONS = ("lt", "le", "gt", "ge", "eq", "ne", "and", "or", "not")

# a body: name -> (layout, variant (P, U, block, flags) or None: the library's own choice, n_streams, n_samples, tile_streams, K).  Layouts: "rows" (time-major [T, ns, w]), "tiles" (stream-tiled), "sm" (stream-major [ns, T, w]: the variant
# without FZ_VF_STREAM_MAJOR).  Lockstep bodies in 64- and 128-lane workgroups: four workgroups at least, so that arrival counters and barriers
# do something; one body in the 1024-lane geometry the library picks by itself
BODIES = {
    "free-p2": ("rows", (2, 8, 256, 0), 2048, 300, 0, K_ROWS),
    "free-p4": ("rows", (4, 8, 256, 0), 2048, 300, 0, K_ROWS),
    "lock-p2": ("rows", (2, 2, 128, L | GS), 2048, 300, 0, K_ROWS),
    "third-p4": ("rows", (4, 1, 64, L | P3), 2048, 300, 0, K_ROWS),
    "third-xcd-p4": ("rows", (4, 1, 128, L | GS | P3), 2048, 300, 0, K_ROWS),
    "wide": ("rows", (1, 3, 1024, L | GS), 2048, 300, 0, K_ROWS),
    "lock-p2-b1024": ("rows", (2, 2, 1024, L | GS), 2048, 300, 0, 2),      # (two: one per family gives two frame widths, the matrix wants three per body)
    "ragged-p2": ("rows", (2, 2, 128, L | GS), 1027, 300, 0, K_ROWS),
    "ragged-p4": ("rows", (4, 1, 64, L | GS | P3), 1027, 300, 0, K_ROWS),
    "tiles-free": ("tiles", (2, 16, 256, 0), 4096, 160, 2048, K_ROWS),
    "tiles-lock": ("tiles", (2, 2, 1024, L | GS), 4096, 160, 2048, K_ROWS),
    "sm-short-p1": ("sm", (1, 0, 0, SMS), 334, 300, 0, K_SM),
    "sm-short-p2": ("sm", (2, 8, 0, SMS), 334, 300, 0, K_SM),
    "sm-short-1x1": ("sm", (1, 0, 0, SMS), 334, 300, 0, 1),                # (a 1 in / 1 out graph: the block behind the cut runs the long body)
    "sm-long64": ("sm", (1, 64, 0, SML), 334, 300, 0, K_SM),
    "sm-long64x2": ("sm", (1, 64, 0, SML), 2, 388, 0, K_SM),
    "sm-long128": ("sm", (1, 128, 0, SML), 2, 388, 0, K_SM),
    "sm-long128x334": ("sm", (1, 128, 0, SML), 334, 300, 0, K_SM),
    "sm-pair334": ("sm", (2, 64, 0, SML), 334, 300, 0, K_SM),
    "sm-pair2": ("sm", (2, 64, 0, SML), 2, 388, 0, K_SM),
    "sm-pair1026": ("sm", (2, 64, 0, SML), 1026, 200, 0, K_SM),
    "auto-rows": ("rows", None, 2048, 300, 0, K_ROWS),
    "auto-ragged": ("rows", None, 1027, 300, 0, K_ROWS),
    "auto-tiles": ("tiles", None, 4096, 160, 2048, K_ROWS),
    "auto-sm": ("sm", None, 334, 300, 0, K_SM),
    "auto-sm2": ("sm", None, 2, 388, 0, K_SM),
}
LONG_BODIES = tuple(b for b, v in BODIES.items() if v[1] and v[1][3] & SML)
LONG1_BODIES = tuple(b for b in LONG_BODIES if BODIES[b][1][0] == 1)
PAIR_BODIES = tuple(b for b in LONG_BODIES if BODIES[b][1][0] == 2)
P4_BODIES = tuple(b for b, v in BODIES.items() if v[0] == "rows" and v[1] and v[1][0] == 4)     # (lane pairs: names ending in L)
P2_BODIES = tuple(b for b, v in BODIES.items() if v[0] == "rows" and v[1] and v[1][0] == 2)     # (lane singles: names ending in S)
# float64 output frames: per typed graph of the rows cells that has a double result, a free-running and a lockstep cell
OUT64_BODIES = {"f64-free-p2": ("rows", (2, 8, 256, OUT64), 2048, 300, 0, 0),
                "f64-lock-p2": ("rows", (2, 2, 128, L | GS | OUT64), 2048, 300, 0, 0)}
# fz_compile_typed with input types drawn per seed (float or double per wire, from a stream of the seed's own): a double wire is two frame
# slots, so a graph with one double input has a 2-wire input frame and four streams per lane run as lane pairs (kernel names ending in L) --
# one pair cell free-running and one in lockstep, and one cell each of a graph that mixes float and double inputs
TIN_BODIES = {"tin-pairs": ("rows", (4, 8, 256, 0), 2048, 300, 0, 1),
              "tin-pairs-lock": ("rows", (4, 1, 128, L | GS | P3), 2048, 300, 0, 1),
              "tin-mixed": ("rows", (4, 8, 256, 0), 2048, 300, 0, 1),
              "tin-mixed-lock": ("rows", (4, 1, 128, L | GS | P3), 2048, 300, 0, 1)}
ALL_BODIES = {**BODIES, **OUT64_BODIES, **TIN_BODIES}
# body -> what a seed has to be for it, beyond its family ("pairs": its kernel on this body is a lane-pair kernel; "mixed": float and double
# inputs; "1x1": 1 in / 1 out without LDS slots).  Other seeds are passed over without being walked
WANTS = {"tin-pairs": "pairs", "tin-pairs-lock": "pairs", "tin-mixed": "mixed", "tin-mixed-lock": "mixed", "sm-short-1x1": "1x1"}
# what tools/fuzz_gpu.py draws from: every distinct explicit variant of BODIES under the name of its first body, and the variants no cell
# pins -- one stream per lane free-running, the plain kernel, a cap on the workgroups per CU, lockstep without the XCD step
TOOL_EXTRA = {"free-p1": (1, 16, 256, 0), "plain": PLAIN, "free-p2-wg2": (2, 8, 256, C.FZ_VF_MAX_WG(2)), "lock-p2-alone": (2, 2, 128, L)}


def tool_bodies(sm):
    """{name: variant} of the distinct explicit variants: the stream-major ones, or the time-major and tiled ones with TOOL_EXTRA"""
    out = {}
    for b, v in list(BODIES.items()) + ([] if sm else list(TOOL_EXTRA.items())):
        var = v[1] if b in BODIES else v
        if var is not None and (b not in BODIES or (v[0] == "sm") == sm) and var not in out.values():
            out[b] = var
    return out


# what the planner refuses outright: (family, class of graph, bodies, status, the head of the message).  No seed of such a class is walked for
# such a body, none is a cell; test_fuzz_bodies_host.py asserts every entry on the family's first seeds of the class by calling the library.
# Classes (classes_of): "any"; "far": a delay line in an HBM ring; "not 1x1": all but the 1 in / 1 out graphs without LDS slots, which
# the long-run and pair bodies take (a deep graph they would take has its deep line in an HBM ring); "no room": the LDS
# rings of the body's workgroup -- its lanes x streams per lane x the graph's ring slots -- pass the 160 KiB of a CU.  The first entry that holds counts
EVERY = ("plain", "cmp", "typed", "deep")
UNREACHABLE = [
    (("deep",), "far", ("third-p4", "third-xcd-p4"), C.FZ_E_INVALID, "FZ_VF_PREFETCH3 is not available with delays beyond LDS"),
    (("deep",), "far", ("sm-short-p1", "sm-short-p2", "sm-short-1x1", "auto-sm", "auto-sm2"), C.FZ_E_UNSUPPORTED, "stream-major frames: delay lines beyond 256 samples are not supported"),
    (("deep",), "any", ("ragged-p2", "ragged-p4"), C.FZ_E_INVALID, "n_streams must be a multiple of streams_per_lane"),      # (LDS rings too: a ring per lane slot)
    (("deep",), "far", LONG_BODIES, C.FZ_E_INVALID, "graphs with delays beyond LDS need unroll <= 16"),
    (("deep",), "no room", tuple(b for b, v in ALL_BODIES.items() if v[1] and v[1][2] and v[2] != 1027), C.FZ_E_UNSUPPORTED, "delay lines too long for the LDS ring buffers"),
    (EVERY, "not 1x1", LONG1_BODIES, C.FZ_E_UNSUPPORTED, "FZ_VF_SM_LONG: needs a 1-in/1-out graph"),
    (EVERY, "not 1x1", PAIR_BODIES, C.FZ_E_UNSUPPORTED, "FZ_VF_SM_LONG with two streams per lane: needs a 1-in/1-out float graph"),
]


def unreachable(family, G, body):
    """the entry of UNREACHABLE that holds (family, graph, body), or None"""
    cl = classes_of(G)
    v = ALL_BODIES[body][1]
    if v and G["prog"].n_lds_slots * v[2] * v[0] * 4 > MAX_LDS_BYTES:
        cl.add("no room")
    for u in UNREACHABLE:
        if family in u[0] and u[1] in cl and body in u[2]:
            return u
    return None


# ---- graphs -------------------------------------------------------------------------------------------------------------------------
def _walk(e):
    yield e
    for c in e:
        if isinstance(c, tuple):
            yield from _walk(c)


def delays(g):
    return [e[2] for e in _walk(g) if e[0] == "del"]


def in_dtypes(family, seed, n_in):
    """the input types of a "tin" graph: float / double per wire, one double at least -- from a stream of the seed's own, apart from the one
    randgraphs draws the graph (and its n_in) from: the types say nothing about the graph"""
    if family != "tin":
        return None
    rng = np.random.default_rng(seed + 88000)
    dts = [str(rng.choice(["f32", "f64"])) for _ in range(n_in)]
    return dts if "f64" in dts else None


_graphs = {}


def graph(family, seed):
    """dict g, n_in, n_out, kind, dts, prog of a seed -- or None: the oracle or the library does not take it, or it is not of its family (a
    cmp graph without a comparison, a deep one without a delay beyond the registers, a typed one without a double or complex node, a graph
    without state)"""
    key = (family, seed)
    if key in _graphs:
        return _graphs[key]
    out = _graphs[key] = None
    r = FAMILIES[family][0](seed)
    g, n_in, n_out = r[:3]
    kind = r[3] if len(r) > 3 else None
    dts = in_dtypes(family, seed, n_in)
    try:
        if O.input_arity(g) != n_in or O.output_arity(g) != n_out or (family == "tin" and dts is None):
            return None
        O.compile(g, 1, typed=True, in_dtypes=dts) if dts else O.compile(g, 1)
        prog = F.compile(F.from_sexpr(g), in_dtypes=dts) if dts else F.compile(F.from_sexpr(g))
    except (O.GraphError, F.FlowzError):
        return None
    nodes = {e[0] for e in _walk(g)}
    if family == "cmp" and not nodes & set(COMPARISONS):
        return None
    if family == "deep" and max(delays(g) + [0]) <= REG_MAX:
        return None
    if family in ("typed", "tin") and kind == "double" and not prog.n_const64:
        return None
    if not prog.n_state:
        return None
    out = _graphs[key] = dict(g=g, n_in=n_in, n_out=n_out, kind=kind, dts=dts, prog=prog, nodes=nodes,
                              rings={"lds" if d <= LDS_MAX else "far" for d in delays(g) if d > REG_MAX})
    return out


def classes_of(G):
    p = G["prog"]
    one = (p.n_in, p.n_out) == (1, 1) and p.n_lds_slots == 0
    return {"any", "1x1" if one else "not 1x1"} | ({"far"} if "far" in G["rings"] else set())


def wanted(G, body):
    """whether a graph is what WANTS asks of the body's seeds"""
    w = WANTS.get(body)
    if w == "mixed":
        return {"f32", "f64"} <= set(G["dts"])
    if w == "1x1":
        return "1x1" in classes_of(G)
    if w == "pairs":
        layout, v, ns, T, tile, _ = ALL_BODIES[body]
        try:
            return G["prog"].kernel_name(variant(v, layout), ns, T, tile).endswith("L")
        except F.FlowzError:
            return False
    return True


def compares_in_double(g):
    """a comparison whose first operand randgraphs widened by a double literal: made in double"""
    return any(e[0] in COMPARISONS[:6] and isinstance(e[1], tuple) and e[1][0] == "mul" and e[1][1][0] == "lit64" for e in _walk(g))


def has_double_result(G):
    return any(t in ("f64", "cf64") for t in G["prog"].output_dtypes())


# ---- inputs and the oracle ----------------------------------------------------------------------------------------------------------
def frames(family, seed, streams, T):
    """(float32 frames [T, len(streams), slots], the typed wires or None) of a seed: O.synth_input(seed, ...) as the one-body fuzz draws it;
    a double input wire gets low-order bits no float has"""
    G = graph(family, seed)
    x = O.synth_input(seed, np.asarray(streams), T, n_wires=G["n_in"])
    if not G["dts"]:
        return x, None
    wires = [x[:, :, i].astype(F64) * (1.0 + 1e-9) if dt == "f64" else x[:, :, i] for i, dt in enumerate(G["dts"])]
    return F.pack_typed(wires, G["dts"]), wires


_SLOT = {"float64": "f64", "complex64": "cf32", "float32": "f32", "complex128": "cf64"}


def oracle_run(family, seed, x, wires, out_f64=False, T=None, zero_wire=None):
    """(the oracle's output frames as the kernels write them, the oracle) on rows [0, T) of x; zero_wire: that input wire held at zero"""
    G = graph(family, seed)
    ns = x.shape[1]
    T = x.shape[0] if T is None else T
    if G["dts"]:
        orc = O.compile(G["g"], ns, typed=True, in_dtypes=G["dts"])
        ws = [np.zeros_like(w[:T]) if i == zero_wire else w[:T] for i, w in enumerate(wires)]
        outs = O.run_typed(orc, ws, T=T)
        return F.pack_typed(outs, [_SLOT[str(o.dtype)] for o in outs]), orc
    orc = O.compile(G["g"], ns, out_f64=out_f64)
    xx = x[:T]
    if zero_wire is not None:
        xx = xx.copy()
        xx[:, :, zero_wire] = 0
    return orc.run(xx), orc


def oracle_state(orc):
    """the delay lines of an oracle as one byte string"""
    out = []
    for w in orc._delayed:
        for v in w.fifo:
            out.append(np.ascontiguousarray(v.re).tobytes() + np.ascontiguousarray(v.im).tobytes() if hasattr(v, "re") else np.ascontiguousarray(v).tobytes())
    return b"".join(out)


def out_wires(G, y):
    """the output frames as one array per wire (a typed program's in the wire's own type: a double is two frame slots), or per slot"""
    if G["dts"]:
        return F.unpack_typed(np.ascontiguousarray(y), G["prog"].output_dtypes())
    return [y[..., j] for j in range(y.shape[-1])]


def all_finite(G, y):
    return all(bool(np.isfinite(w).all()) for w in out_wires(G, y))


def slice_streams(ns):
    """the first and the last 3 streams"""
    return np.unique(np.concatenate([np.arange(min(3, ns)), np.arange(max(ns - 3, 0), ns)]))


def ndiff(a, b):
    """words that differ, NaNs of any payload equal"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    u = np.uint32 if a.dtype == F32 else np.uint64
    return int(((a.view(u) != b.view(u)) & ~(np.isnan(a) & np.isnan(b))).sum())


_disc = {}


def discriminates(family, seed, ns, T, cut):
    """None where the cell's inputs can tell a wrong kernel from a right one, else what they cannot tell -- on the oracle alone, over the
    first and the last 3 streams: the output stays finite, no output wire is constant over the block, zeroing any one input wire changes the
    output, the delay lines after `cut` rows differ from those after cut + 1"""
    key = (family, seed, ns, T, cut)
    if key not in _disc:
        _disc[key] = _discriminates(*key)
    return _disc[key]


def _discriminates(family, seed, ns, T, cut):
    G = graph(family, seed)
    x, wires = frames(family, seed, slice_streams(ns), T)
    want, _ = oracle_run(family, seed, x, wires)
    if not all_finite(G, want):
        return "the output does not stay finite"
    if any((w == w[:1]).all() for w in out_wires(G, want)):
        return "an output wire is constant over the block"
    for i in range(G["n_in"]):
        if ndiff(oracle_run(family, seed, x, wires, zero_wire=i)[0], want) == 0:
            return f"input wire {i + 1} does not reach the output"
    a, b = oracle_run(family, seed, x, wires, T=cut)[1], oracle_run(family, seed, x, wires, T=cut + 1)[1]
    if oracle_state(a) == oracle_state(b):
        return "the state after the cut is the state one row later"
    return None


# ---- what a cell resolves to ----------------------------------------------------------------------------------------------------------
def variant(v, layout="rows"):
    if v is None:
        return F.make_variant(0, 0, 0, SM) if layout == "sm" else None
    return F.make_variant(v[0], v[1], v[2], v[3] | (SM if layout == "sm" else 0))


def cut_of(layout):
    return CUT_SM if layout == "sm" else CUT_ROWS


def plain_of(G, ns, T, out_f64=False, other_than=None):
    """PLAIN -- for a deep graph its chunk within what the HBM rings take (half the youngest ring read), and the workgroup left to the
    planner where 256 lanes of LDS rings do not fit.  other_than: a kernel name it must not resolve to (the library's own choice for a
    deep graph at these shapes can be the plain kernel itself: the block behind the cut then takes a shorter chunk)"""
    for U, block in ((8, 256), (4, 256), (2, 256), (1, 256), (8, 0), (4, 0), (2, 0), (1, 0)):
        v = (1, U, block, NSP | (OUT64 if out_f64 else 0))
        try:
            if G["prog"].kernel_name(variant(v), ns, T, 0) != other_than:
                return v
        except F.FlowzError:
            pass
    raise AssertionError("no plain kernel")


def after_of(G, layout, v, ns, T, tile, name):
    """the body behind the cut: rows and tiles continue on the plain kernel; stream-major short on long where the graph and the rest of the
    block allow it, else on short with another chunk; long and pair on short.  Another kernel than the cell's own in every case"""
    if layout != "sm":
        return plain_of(G, ns, T, bool(v and v[3] & OUT64), other_than=name)
    n = T - CUT_SM
    own_long = v is not None and v[3] & SML
    for cand in ([] if own_long else [(0, 0, 0, SML)]) + [(1, 16, 0, SMS), (1, 4, 0, SMS)]:
        try:
            if G["prog"].kernel_name(variant(cand, "sm"), ns, n, 0) != name:
                return cand
        except F.FlowzError:
            pass
    raise AssertionError("no other stream-major body")


def refusal(G, body):
    """None, or (status, message) of the library's refusal of a graph on a body: by kernel_name, and for an explicit lockstep variant by
    the build (a lockstep kernel that needs scratch is refused when it is built, not when it is planned)"""
    layout, v, ns, T, tile, _ = ALL_BODIES[body]
    try:
        G["prog"].kernel_name(variant(v, layout), ns, T, tile)
        if v is not None and v[3] & L:
            G["prog"].build(variant(v, layout), ns, T, tile)
    except F.FlowzError as e:
        return e.code, str(e)
    return None


def resolve(family, seed, body):
    """the pin of a cell"""
    G = graph(family, seed)
    layout, v, ns, T, tile, _ = ALL_BODIES[body]
    name = G["prog"].kernel_name(variant(v, layout), ns, T, tile)
    after = after_of(G, layout, v, ns, T, tile, name)
    return {"family": family, "seed": seed, "body": body, "layout": layout, "variant": None if v is None else list(v), "shape": [ns, T], "tile": tile,
            "kind": G["kind"], "in_dtypes": G["dts"], "frame": [G["prog"].n_in, G["prog"].n_out], "kernel": name, "cut": cut_of(layout), "after": list(after)}


def select_body(family, body, seeds=None, K=None):
    """(the seeds kept, {seed: (status, message)} of the seeds refused, the seeds walked) of one (family, body): the family's range in order
    until K seeds are kept"""
    layout, v, ns, T, tile, k = ALL_BODIES[body]
    K = K_MORE.get((family, body), k) if K is None else K
    first = FAMILIES[family][1]
    kept, refused, walked = [], {}, 0
    for seed in (range(first, first + WALK) if seeds is None else seeds):
        if len(kept) >= K:
            break
        G = graph(family, seed)
        if G is None:
            continue
        if unreachable(family, G, body) or not wanted(G, body):
            continue
        if discriminates(family, seed, ns, T, cut_of(layout)) is not None:
            continue
        walked += 1
        r = refusal(G, body)
        if r is not None:
            refused[seed] = r
        else:
            kept.append(seed)
    return kept, refused, walked


def select():
    """(pins {cell id: pin} in the order the GPU test runs them, walk {(family, body): (kept, refused, walked)})"""
    pins, walk = {}, {}
    for family in TABLE_FAMILIES:
        for body in BODIES:
            walk[family, body] = select_body(family, body)
            for seed in walk[family, body][0]:
                pins[f"{family}{seed}-{body}"] = resolve(family, seed, body)
    # float64 output frames: every typed graph of the cells above at 2048 x 300 that has a double result
    seeds = sorted({p["seed"] for p in pins.values() if p["family"] == "typed" and p["shape"] == [2048, 300] and has_double_result(graph("typed", p["seed"]))})
    for body in OUT64_BODIES:
        walk["typed", body] = select_body("typed", body, seeds, len(seeds))
        for seed in walk["typed", body][0]:
            pins[f"typed{seed}-{body}"] = resolve("typed", seed, body)
    for body in TIN_BODIES:
        walk["tin", body] = select_body("tin", body)
        for seed in walk["tin", body][0]:
            pins[f"tin{seed}-{body}"] = resolve("tin", seed, body)
    # one oracle run per (graph, shape): the cells that share one follow one another
    order = sorted(pins, key=lambda k: (list(FAMILIES).index(pins[k]["family"]), pins[k]["seed"], pins[k]["shape"], "f64" in pins[k]["body"]))
    return {k: pins[k] for k in order}, walk


def dump(pins):
    return "{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in pins.items()) + "\n}\n"


def load_pins():
    with open(PINS_FILE) as f:
        return json.load(f)


CELLS = load_pins() if os.path.exists(PINS_FILE) else {}


def out_f64(pin):
    return bool(pin["variant"] and pin["variant"][3] & OUT64)


# ---- the kernels of the GPU test ----------------------------------------------------------------------------------------------------
def kernel_requests():
    """(family, seed, layout, variant, n_streams, n_samples, tile_streams) of every kernel test_fuzz_bodies_gpu.py launches: each cell's
    own, the whole block and the rows up to the cut; the body behind the cut; the plain kernel; for a stream-major cell the rows kernel
    it is compared with"""
    out = []
    for pin in CELLS.values():
        fam, seed, layout, (ns, T), tile, cut = pin["family"], pin["seed"], pin["layout"], pin["shape"], pin["tile"], pin["cut"]
        v = None if pin["variant"] is None else tuple(pin["variant"])
        plain = plain_of(graph(fam, seed), ns, T, out_f64(pin))
        out += [(fam, seed, layout, v, ns, T, tile), (fam, seed, layout, v, ns, cut, tile), (fam, seed, layout, tuple(pin["after"]), ns, T - cut, tile),
                (fam, seed, "rows", plain, ns, T, 0)]
    return list(dict.fromkeys(out))


def resolve_kernels():
    """build every kernel of kernel_requests(); returns how many"""
    n = 0
    for fam, seed, layout, v, ns, T, tile in kernel_requests():
        graph(fam, seed)["prog"].build(variant(v, layout), ns, T, tile)
        n += 1
    return n


def record(path=None):
    """resolve_kernels() in a process that records (FLOWZ_HIP_MANIFEST); needs no GPU.  Returns the raw manifest"""
    code = "import sys\nsys.path[:0] = [%r, %r]\nimport fuzz_bodies as FB\nFB.resolve_kernels()\n" % (os.path.dirname(HERE), HERE)
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
    """tests/golden/fuzz_bodies_kernels.fzm.gz.  build() replays every manifest under tests/golden/, so a GPU run finds these built"""
    with open(MANIFEST, "wb") as out:
        out.write(gzip.compress(record(), 9, mtime=0))
    return F.manifest_build(MANIFEST)


if __name__ == "__main__":                         # rewrite the pins of the library as it is (review the diff), then the manifest
    pins, walk = select()
    with open(PINS_FILE, "w") as f:
        f.write(dump(pins))
    for (family, body), (kept, refused, walked) in walk.items():
        print(f"{family:6} {body:16} kept {kept}, refused {sorted(refused)} of {walked} walked")
    print(len(pins), "cells")
    print("kernel manifest:", record_manifest())                 # (its recording process reads the pins just written)
