"""The delay-line matrix: graphs whose delays sweep every storage class (registers up to 8 samples, LDS rings up to 256, HBM rings beyond)
and every way the code generator reads an LDS ring (vectorised in time, fetched up front per chunk, in place), the kernel bodies they run
on, and their inputs.

CELLS names, for every cell, the graph template and its depths, the frame layout, the variant, the shape, and (PINS) the kernel name and
ring plan the library resolves for it.  test_delay_lines_host.py checks every pin and the coverage of the matrix without a GPU (so a planner
or code generator change that moves a cell fails on a CPU first); test_delay_lines_gpu.py runs every cell against oracle.flowz_oracle."""
import json
import os
import re

import numpy as np

from graphs import DEL, IN, add, chan, fb, lit, mul, par, seq
from oracle import flowz_oracle as O
from zignal_amd import flowz as F

F32, F64 = np.float32, np.float64
C = F.C
L, GS, P3, NSP = C.FZ_VF_LOCKSTEP, C.FZ_VF_GRID_SYNC, C.FZ_VF_PREFETCH3, C.FZ_VF_NO_STAGE_PACK
SM, SMS = C.FZ_VF_STREAM_MAJOR, C.FZ_VF_SM_SHORT
SEED = 20261016
REG_MAX, LDS_MAX = 8, 256                     # kRegMaxDepth, kLdsMaxDepth (fz_internal.hpp)
MAX_LDS_BYTES = 160 * 1024

LDS_DEPTHS = (9, 10, 11, 12, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256)
FAR_DEPTHS = (257, 258, 259, 260, 511, 512, 513)
DEPTHS = (8,) + LDS_DEPTHS + FAR_DEPTHS


# ---- graph templates (s-expressions: the same one drives the oracle and the library) ------------------------------------------
def ff(d):
    """_1 + c * _1[d]: feed-forward comb"""
    return add(IN(1), mul(lit(0.5), DEL(1, d)))


def fbk(d):
    """~(c * _1[d] + _2): a loop through the line -- a read of step t depends on a push of the same chunk whenever d < U"""
    return fb(add(mul(lit(0.6), DEL(1, d)), IN(2)))


def taps(*ds):
    """one fed-back line read at several distances (the deepest is the line's depth); loop gain 0.8"""
    cs = (0.3, -0.2, 0.2, 0.1)
    e = mul(lit(cs[0]), DEL(1, ds[0]))
    for c, d in zip(cs[1:], ds[1:]):
        e = add(e, mul(lit(c), DEL(1, d)))
    return fb(add(e, IN(2)))


def mixed(dr, dl, df=0):
    """a comb over a register line, then a loop over an LDS line, then (df) a loop over an HBM line"""
    g = seq(add(IN(1), mul(lit(0.4), DEL(1, dr))), fb(add(mul(lit(0.5), DEL(1, dl)), IN(2))))
    return seq(g, fb(add(mul(lit(-0.5), DEL(1, df)), IN(2)))) if df else g


def mixed2(dr, dl, df=0):
    """2 in / 2 out: a loop over an LDS line next to a comb over a line read dr and (df: an HBM line with a shadow register) df samples
    back, then both wires mixed, the second with itself two samples back"""
    right = add(IN(1), mul(lit(0.4), DEL(1, dr)))
    if df:
        right = add(right, mul(lit(0.3), DEL(1, df)))
    return seq(par(fb(add(mul(lit(0.5), DEL(1, dl)), IN(2))), right), chan(add(IN(1), mul(lit(0.25), IN(2))), add(IN(2), mul(lit(-0.25), DEL(1, 2)))))


def many(k, d, nt):
    """k feed-forward stages in series, each with a line of depth d read at nt distances d, d - 1, ..."""
    cs = (0.3, -0.2, 0.2, 0.1, -0.1)
    g = None
    for _ in range(k):
        e = IN(1)
        for j in range(nt):
            e = add(e, mul(lit(cs[j]), DEL(1, d - j)))
        g = e if g is None else seq(g, e)
    return g


TEMPLATES = {"ff": ff, "fb": fbk, "taps": taps, "mixed": mixed, "mixed2": mixed2, "many": many}
FEED_FORWARD = ("ff", "many")                      # (no loop: every class of input value can go in, none sticks)


def sexpr(tmpl, args):
    return TEMPLATES[tmpl](*args)


def graph_depths(tmpl, args):
    """the depths of the lines of a graph, in the library's line order"""
    if tmpl in ("ff", "fb"):
        return [args[0]]
    if tmpl == "taps":
        return [max(args)]
    if tmpl == "many":
        return [args[1]] * args[0]
    dr, dl, df = (tuple(args) + (0,))[:3]
    if tmpl == "mixed":
        return [dr, dl] + ([df] if df else [])
    return [dl, max(dr, df)]                       # (mixed2: the loop's line is also read 2 back, the comb's dr and df back)


def reads(tmpl, args):
    """every (depth of the line, distance read) of a graph"""
    if tmpl in ("ff", "fb"):
        return [(args[0], args[0])]
    if tmpl == "taps":
        return [(max(args), d) for d in args]
    if tmpl == "many":
        return [(args[1], args[1] - j) for _ in range(args[0]) for j in range(args[2])]
    dr, dl, df = (tuple(args) + (0,))[:3]
    if tmpl == "mixed":
        return [(dr, dr), (dl, dl)] + ([(df, df)] if df else [])
    return [(dl, dl), (dl, 2), (max(dr, df), dr)] + ([(df, df)] if df else [])


def neighbours(tmpl, args):
    """the graphs with one read moved by one sample (each tap of `taps` in turn): what a kernel wrong by one slot would compute"""
    out = []
    if tmpl in ("ff", "fb"):
        out = [(args[0] - 1,), (args[0] + 1,)]
    elif tmpl == "taps":
        for i in range(len(args)):
            for s in (-1, 1):
                a = list(args)
                a[i] += s
                if a[i] >= 1 and len(set(a)) == len(a):
                    out.append(tuple(a))
    elif tmpl == "many":
        out = [(args[0], args[1] - 1, args[2]), (args[0], args[1] + 1, args[2])]
    else:
        for i in range(len(args)):
            for s in (-1, 1):
                a = list(args)
                if a[i]:
                    a[i] += s
                    out.append(tuple(a))
    return out


def compile_cell(c):
    e = F.from_sexpr(sexpr(c["tmpl"], c["args"]))
    return F.compile(e, in_dtypes=[c["dtype"]]) if c["dtype"] else F.compile(e)


def storage(d):
    return "reg" if d <= REG_MAX else "lds" if d <= LDS_MAX else "far"


def ring_size(d):
    return 1 << (d - 1).bit_length()


# ---- cells --------------------------------------------------------------------------------------------------------------------
def block_length(d, U):
    """samples of a cell: room for the chained pieces 1, G - 1, d - 1, d, d + 1 and a long one; odd and no multiple of the chunk, so that
    neither T % U nor T % G is 0"""
    T = 3 * d + 3 * max(U, 16) + 37
    while T % 2 == 0 or (U > 1 and T % U == 0):
        T += 1
    return T


def _cell(cid, tmpl, args, layout, v, ns, T=None, tile=0, dtype=None, other=None):
    d = max(a for a in (args[1:2] if tmpl == "many" else args))
    U = v[1] if v else 16
    T = T if T is not None else block_length(d, U or 16)
    return {"id": cid, "tmpl": tmpl, "args": tuple(args), "layout": layout, "v": v, "ns": ns, "T": T, "tile": tile, "dtype": dtype, "d": d, "other": other,
            # a block no longer than the line says nothing about its depth by itself: d + 2 more samples follow it in the chained run
            "tail": d + 2 if T < d + 2 else 0}


def _cells():
    cs = []
    # 1. every depth, the free-running block kernel: the loop with one stream per lane and 16-row chunks, the comb with two and 8-row chunks
    #    (block 0: the planner shrinks the workgroup where 256 lanes of rings do not fit the LDS)
    for d in DEPTHS:
        cs.append(_cell(f"fb{d}-p1u16", "fb", (d,), "rows", (1, 16, 0, 0), 512))
        cs.append(_cell(f"ff{d}-p2u8", "ff", (d,), "rows", (2, 8, 0, 0), 334))
    # 2. four streams per lane: LDS rings up to 128 samples (deeper ones do not fit: refusals below), every HBM depth
    #    (fb31-p4u8 does not run the chunk it asks for: its 8-row kernel uses scratch -- alone among these depths; 17, 32 and 63 do not -- and the
    #     launch steps down to 2-row chunks, G = 2.  That pin, like the double loops that ask for 16 rows and settle at 8, follows the compiler's
    #     register allocation and moves with a compiler update; the cell then still runs, on the other chunk length)
    for d in DEPTHS:
        if d <= 128 or d > LDS_MAX:
            cs.append(_cell(f"fb{d}-p4u8", "fb", (d,), "rows", (4, 8, 0, 0), 512))
    # 3. the chunk length: every unroll, at depths around the first ring sizes
    for P, ds, Us in ((1, (9, 16, 17, 33), (1, 2, 3, 4, 8, 12, 32)), (2, (10, 32), (2, 3, 4, 12, 32)), (4, (11, 32), (1, 2, 3, 12, 16))):
        for d in ds:
            for U in Us:
                cs.append(_cell(f"fb{d}-p{P}u{U}", "fb", (d,), "rows", (P, U, 256, 0), 512))
    for d, U in ((9, 12), (12, 32), (15, 4), (31, 12), (63, 3), (127, 32), (128, 12)):
        cs.append(_cell(f"ff{d}-p1u{U}", "ff", (d,), "rows", (1, U, 256, 0), 512))
    # 4. several taps on one line: the deepest, one in the middle, 9, and one within the registers' range (on a far line: a shadow register)
    for k, (ts, P, U) in enumerate((((12, 10, 9, 2), 1, 16), ((16, 12, 9, 3), 2, 8), ((16, 13, 9, 2), 4, 8), ((40, 20, 9, 5), 1, 16), ((64, 33, 9, 8), 2, 16),
                                    ((65, 32, 9), 1, 32), ((128, 64, 9, 4), 4, 4), ((256, 100, 9, 7), 1, 8), ((33, 17), 1, 32), ((64, 48, 32), 4, 32),
                                    ((257, 128, 9, 3), 1, 4), ((300, 150, 9, 8), 2, 4), ((512, 256, 9, 1), 4, 4), ((513, 257, 32), 2, 16), ((260, 40, 33, 6), 1, 16))):
        cs.append(_cell("taps" + "_".join(map(str, ts)) + f"-p{P}u{U}", "taps", ts, "rows", (P, U, 0, 0), 512))
    # 5. the lockstep frame kernel: workgroups of 256 and 1024 lanes, its step-down to one row per chunk with three buffers; far lines in
    #    lockstep take chunks of at least two rows and no third buffer
    for d in (9, 16, 17, 32):
        cs.append(_cell(f"fb{d}-L256", "fb", (d,), "rows", (1, 16, 256, L | GS), 512))
        cs.append(_cell(f"ff{d}-L1024", "ff", (d,), "rows", (1, 4, 1024, L | GS), 2048))
        cs.append(_cell(f"fb{d}-Lp3", "fb", (d,), "rows", (1, 1, 256, L | GS | P3), 512))
    for d in (10, 16):
        cs.append(_cell(f"fb{d}-p2L1024", "fb", (d,), "rows", (2, 2, 1024, L | GS), 2048))
    for d in (64, 65, 128, 255, 256):
        cs.append(_cell(f"fb{d}-L", "fb", (d,), "rows", (1, 16, 0, L | GS), 512))
        cs.append(_cell(f"ff{d}-Lp3", "ff", (d,), "rows", (1, 1, 0, L | GS | P3), 512))
    for d in (257, 260, 512):
        cs.append(_cell(f"fb{d}-L256", "fb", (d,), "rows", (1, 8, 256, L | GS), 512))
        cs.append(_cell(f"ff{d}-p2L1024", "ff", (d,), "rows", (2, 2, 1024, L | GS), 2048))
    cs.append(_cell("fb257-p4L1024", "fb", (257,), "rows", (4, 2, 1024, L | GS), 4096))
    # 6. stream tiles, free-running and in lockstep
    for d in (9, 16, 33, 255, 256, 257, 511):
        cs.append(_cell(f"fb{d}-tiles", "fb", (d,), "tiles", (1, 16, 0, 0), 1024, tile=256))
        cs.append(_cell(f"ff{d}-tilesL", "ff", (d,), "tiles", (1, 8, 0, L | GS), 1024, tile=256))
    cs.append(_cell("fb16-tiles-p2L1024", "fb", (16,), "tiles", (2, 2, 1024, L | GS), 4096, tile=2048))
    # 7. stream-major buffers, the short body: every LDS depth with one stream per lane (the loop) and with two (the comb), a ragged count
    for d in (8,) + LDS_DEPTHS:
        cs.append(_cell(f"fb{d}-sm1", "fb", (d,), "sm", (1, 0, 0, SMS), 334))
        cs.append(_cell(f"ff{d}-sm2", "ff", (d,), "sm", (2, 0, 0, SMS), 334))
    # 8. the library's own choice at the test's shape
    for d in (9, 64, 256, 257, 513):
        cs.append(_cell(f"fb{d}-auto", "fb", (d,), "rows", None, 2048))
        cs.append(_cell(f"ff{d}-auto-tiles", "ff", (d,), "tiles", None, 1024, tile=256))
    for d in (12, 128):
        cs.append(_cell(f"ff{d}-auto-sm", "ff", (d,), "sm", (0, 0, 0, 0), 334))
    # 9. a register line, an LDS line and an HBM line in one graph; 2 in / 2 out: four streams per lane run as lane groups
    for P, U, flags, ns in ((1, 16, 0, 512), (2, 8, 0, 512), (4, 4, 0, 512), (2, 2, 256, 2048)):
        cs.append(_cell(f"mixed3_40_300-p{P}u{U}" + ("L" if flags else ""), "mixed", (3, 40, 300), "rows", (P, U, flags, flags and (L | GS)), ns))
        cs.append(_cell(f"mixed2_5_16_257-p{P}u{U}" + ("L" if flags else ""), "mixed2", (5, 16, 257), "rows", (P, U, flags, flags and (L | GS)), max(ns, 2048)))
    cs.append(_cell("mixed2_8_9-p4u8", "mixed2", (8, 9), "rows", (4, 8, 256, 0), 2048))
    cs.append(_cell("mixed2_8_9-p4Lp3", "mixed2", (8, 9), "rows", (4, 1, 256, L | GS | P3), 2048))
    for P in (1, 2):
        cs.append(_cell(f"mixed3_40-sm{P}", "mixed", (3, 40), "sm", (P, 0, 0, SMS), 334))
        cs.append(_cell(f"mixed2_5_16-sm{P}", "mixed2", (5, 16), "sm", (P, 0, 0, SMS), 334))
    # 10. many lines with several taps each: the register estimate of the vectorised plan passes 200 (G halved; given up), the rings of 256 lanes
    #     pass the LDS (the workgroup shrinks)
    cs.append(_cell("many4_16_3-p1u16", "many", (4, 16, 3), "rows", (1, 16, 0, 0), 512))
    cs.append(_cell("many6_16_4-p4u8", "many", (6, 16, 4), "rows", (4, 8, 0, 0), 512))
    cs.append(_cell("many10_16_4-p1u16", "many", (10, 16, 4), "rows", (1, 16, 0, 0), 512))
    cs.append(_cell("many4_128_2-p1u16", "many", (4, 128, 2), "rows", (1, 16, 0, 0), 512))
    cs.append(_cell("many5_128_2-p1u1", "many", (5, 128, 2), "rows", (1, 1, 0, L | GS | P3), 512, other=(1, 1, 0, NSP)))   # (vectorised, the padded rings would not fit)
    # 11. typed programs: the loop on a double wire (two float rows per slot: every LDS depth) and on a std::complex<float> wire (two lines)
    for k, d in enumerate((8,) + LDS_DEPTHS):
        P, U = ((1, 16), (2, 8), (4, 4))[k % 3] if d <= 64 else ((1, 16), (2, 8))[k % 2] if d <= 128 else (1, 16)
        cs.append(_cell(f"fb{d}-f64-p{P}u{U}", "fb", (d,), "rows", (P, U, 0, 0), 512, dtype="f64"))
    for d in (9, 33, 128, 256):
        cs.append(_cell(f"fb{d}-f64-sm", "fb", (d,), "sm", (1, 0, 0, SMS), 332, dtype="f64"))
        cs.append(_cell(f"fb{d}-f64-Lp3", "fb", (d,), "rows", (1, 1, 0, L | GS | P3), 512, dtype="f64"))
    for d, P, U in ((9, 1, 16), (16, 2, 8), (17, 4, 8), (33, 1, 12), (64, 2, 4), (128, 1, 32), (255, 1, 16), (256, 1, 8)):
        cs.append(_cell(f"fb{d}-cf32-p{P}u{U}", "fb", (d,), "rows", (P, U, 0, 0), 512, dtype="cf32"))
    for d, P, U in ((257, 1, 8), (260, 2, 4)):                       # (a complex wire beyond the LDS: two float rings in HBM)
        cs.append(_cell(f"fb{d}-cf32-p{P}u{U}", "fb", (d,), "rows", (P, U, 0, 0), 512, dtype="cf32"))
    # 12. blocks no longer than the line (d + 2 more samples follow in the chained run)
    for d, v in ((16, (1, 16, 0, 0)), (40, (1, 16, 0, 0)), (256, (1, 16, 0, 0)), (257, (1, 16, 0, 0)), (512, (4, 8, 0, 0))):
        for T, tag in ((d - 3, "lt"), (d, "eq"), (d + 1, "gt")):
            cs.append(_cell(f"fb{d}-T{tag}-p{v[0]}", "fb", (d,), "rows", v, 512, T=T))
    cs.append(_cell("ff33-Teq-sm1", "ff", (33,), "sm", (1, 0, 0, SMS), 334, T=33))
    ids = [c["id"] for c in cs]
    assert len(set(ids)) == len(ids), [i for i in ids if ids.count(i) > 1]
    return cs


CELLS = _cells()

# what the planner refuses: (template, args, dtype, variant, stream-major, status, a piece of the message)
REFUSALS = [
    ("fb", (129,), None, (4, 8, 0, 0), False, C.FZ_E_UNSUPPORTED, "delay lines too long for the LDS ring buffers"),
    ("fb", (256,), None, (4, 8, 0, 0), False, C.FZ_E_UNSUPPORTED, "delay lines too long for the LDS ring buffers"),
    ("fb", (256,), None, (1, 16, 256, 0), False, C.FZ_E_UNSUPPORTED, "delay lines too long for the LDS ring buffers"),      # (a block the caller fixed)
    ("many", (6, 128, 2), None, (1, 16, 0, 0), False, C.FZ_E_UNSUPPORTED, "delay lines too long for the LDS ring buffers"),  # one more line than many5_128_2
    ("fb", (257,), None, (1, 0, 0, SMS), True, C.FZ_E_UNSUPPORTED, "delay lines beyond 256 samples are not supported"),
    ("mixed", (3, 40, 300), None, (2, 0, 0, SMS), True, C.FZ_E_UNSUPPORTED, "delay lines beyond 256 samples are not supported"),
    ("fb", (257,), None, (1, 32, 0, 0), False, C.FZ_E_INVALID, "need unroll <= 16"),
    ("taps", (257, 128, 9, 3), None, (1, 8, 0, 0), False, C.FZ_E_INVALID, "need unroll <= 4"),
    ("fb", (257,), None, (1, 1, 256, L | GS | P3), False, C.FZ_E_INVALID, "FZ_VF_PREFETCH3 is not available with delays beyond LDS"),
]


def variant(c):
    v = c["v"]
    if v is None:
        return None
    return F.make_variant(v[0], v[1], v[2], v[3] | (SM if c["layout"] == "sm" else 0))


def cell_name(prog, c):
    return prog.kernel_name(variant(c), c["ns"], c["T"], c["tile"])


_NAME = re.compile(r"fz_block_kernel_p(\d+)u(\d+)b(\d+)(?:s\d+(?:a\d+)?)?(?:w\d(?:io2?)?)?f(\d+)([RMLS]*)$")


def resolved(prog, c):
    """(kernel name, P, U, block, FZ_RING_G, FZ_LDS_SLOTS, how the LDS rings are read) of a cell: the name of its launch, the rest from the
    configuration and the graph body generated for the explicit variant the name spells"""
    name = cell_name(prog, c)
    m = _NAME.match(name)
    assert m, name
    P, U, B, flags = (int(x) for x in m.groups()[:4])
    flags |= SMS if c["layout"] == "sm" else 0     # (the letters behind the flags: internal bits of the launch, no part of the ring plan)
    src = prog.source(F.make_variant(P, U, B, flags))
    defs = {k: int(re.search(r"#define %s (\d+)" % k, src).group(1)) for k in ("FZ_RING_G", "FZ_LDS_SLOTS", "FZ_U", "FZ_BLOCK", "FZ_P")}
    assert (defs["FZ_P"], defs["FZ_U"], defs["FZ_BLOCK"]) == (P, U, B), (name, defs)
    body = src.split("// ==== fz_graph_body.h ====")[1].split("// ==== ")[0]
    how = "none" if not defs["FZ_LDS_SLOTS"] else "vec" if defs["FZ_RING_G"] else "front" if re.search(r"\bV lr\d+\[FZ_U\];", body) else "place"
    return name, P, U, B, defs["FZ_RING_G"], defs["FZ_LDS_SLOTS"], how


def other_body(c):
    """the variant of the pieces of a chained run that the cell's own variant does not run: a plain free-running kernel, its chunk within the
    far lines' cap (half the youngest read of an HBM ring)"""
    if c.get("other"):
        return c["other"]
    far_reads = [r for dl, r in reads(c["tmpl"], c["args"]) if dl > LDS_MAX and r > REG_MAX]
    U = min([8] + [r // 2 for r in far_reads])
    v = (1, U, 0, NSP)
    if c["layout"] == "rows" and c.get("plain") is None and (c["v"] is None or (c["v"][0] == 1 and not (c["v"][3] & L))):
        v = (1, 2 if c["v"] and c["v"][1] == 4 else min(U, 4), 0, NSP)          # (one stream per lane again: a chunk of another length)
    return v


def plain(c):
    """the kernel every cell's state is compared with"""
    return other_body(dict(c, plain=True))


def pieces(c, G, U):
    """lengths of the chained blocks of a cell: 1, G - 1 (U - 1 where the rings are not vectorised), d - 1, d, d + 1 and what is left as one
    long piece; behind a block no longer than the line, that block first"""
    d, total = c["d"], c["T"] + c["tail"]
    want = ([c["T"]] if c["tail"] else []) + [1, (G or U) - 1, d - 1, d, d + 1]
    out, left = [], total
    for n in want:
        n = min(n, left)
        if n > 0:
            out.append(n)
            left -= n
    if left:
        out.append(left)
    assert sum(out) == total
    return out


# ---- inputs -------------------------------------------------------------------------------------------------------------------
EDGES = ((4, 5, np.nan), (6, 5, np.inf), (129, 6, -0.0), (130, 6, float(np.finfo(F32).smallest_subnormal)), (7, 3, -np.inf))   # (stream, row, value)


def n_wires(c):
    return O.input_arity(sexpr(c["tmpl"], c["args"]))


def frames(c):
    """noise over the whole block (every sample differs from its neighbours); in the feed-forward graphs -0, a subnormal, infinities and a
    NaN in streams of lanes 1 and 32 (a value moved to the wrong stream of a packed lane or lane group shows).  Typed cells: the wire in its
    own type, a double whose low word is not zero.  Returns (float32 frames [T + tail, ns, slots], the wires for oracle.run_typed or None)"""
    T, ns = c["T"] + c["tail"], c["ns"]
    seed = SEED + 1000 * ns + T + sum(map(ord, c["tmpl"])) + sum(c["args"])
    if c["dtype"] == "f64":
        a = O.synth_input(seed, np.arange(ns), T)[..., 0].astype(F64)
        a *= 1 + np.ldexp(np.random.default_rng(seed).random((T, ns)), -30)
        return F.pack_typed([a], ["f64"]), [a]
    if c["dtype"] == "cf32":
        a = O.synth_input(seed, np.arange(ns), T, n_wires=2)
        z = (a[..., 0] + 1j * a[..., 1]).astype(np.complex64)
        return F.pack_typed([z], ["cf32"]), [z]
    x = O.synth_input(seed, np.arange(ns), T, n_wires=n_wires(c))
    if c["tmpl"] in FEED_FORWARD:
        for s, t, v in EDGES:
            if s < ns and t < T:
                x[t, s, 0] = v
    return x, None


def all_finite(c, y):
    """frames of a double wire hold its two words: finite as doubles"""
    return bool(np.isfinite(np.ascontiguousarray(y).view(F64) if c["dtype"] == "f64" else y).all())


def edge_streams(c):
    return sorted({s for s, t, _ in EDGES if s < c["ns"] and t < c["T"] + c["tail"]}) if c["tmpl"] in FEED_FORWARD and not c["dtype"] else []


def oracle_run(c, args=None, x=None, wires=None, streams=None):
    """the oracle's output frames (float32 slots, as the kernels write them) of the cell's graph -- or of the same template with other
    depths -- on the cell's input; streams: a subset of them"""
    g = sexpr(c["tmpl"], args if args is not None else c["args"])
    if x is None:
        x, wires = frames(c)
    sel = slice(None) if streams is None else np.asarray(streams)
    ns = c["ns"] if streams is None else len(streams)
    if c["dtype"]:
        orc = O.compile(g, ns, typed=True, in_dtypes=[c["dtype"]])
        outs = O.run_typed(orc, [w[:, sel] for w in wires])
        return F.pack_typed(outs, [{"float64": "f64", "complex64": "cf32", "float32": "f32"}[str(o.dtype)] for o in outs])
    return O.compile(g, ns).run(x[:, sel])


# ---- pins ---------------------------------------------------------------------------------------------------------------------
PINS_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "delay_line_pins.json")


def load_pins():
    """cell id -> [kernel name, P, U, block, FZ_RING_G, FZ_LDS_SLOTS, how the rings are read ("vec", "front", "place"; "none": no LDS ring)]"""
    with open(PINS_FILE) as f:
        return json.load(f)


if __name__ == "__main__":                         # python tests/delay_cells.py: write the pins of the library as it is (review the diff)
    pins = {}
    for c in CELLS:
        try:
            pins[c["id"]] = list(resolved(compile_cell(c), c))
        except F.FlowzError as e:
            print("REFUSED", c["id"], e)
    with open(PINS_FILE, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in pins.items()) + "\n}\n")
    print(len(pins), "cells,", len({(c["tmpl"], c["args"], c["dtype"], tuple(pins[c["id"]][:4])) for c in CELLS if c["id"] in pins}), "kernels")
