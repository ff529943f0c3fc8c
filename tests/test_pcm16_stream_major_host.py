"""16-bit PCM on stream-major buffers without a GPU (fz_run_block_pcm16_stream_major): the exported symbols, the refusals (those of the
time-major PCM call, word for word), every argument check on fake addresses -- each fails before a device is needed --, the kernel's
JIT for gfx950 with its chunk rows and LDS bytes pinned (tests/golden/pcm16_sm_pins.json), and what a manifest replay does with
records no launch could have made."""
import ctypes
import json
import os
import re

import pytest

import grad_graphs as GG
import graphs as G
from zignal_amd import _capi as C
from zignal_amd import flowz as F

I16, FLT = C.FZ_FRAMES_I16, C.FZ_FRAMES_F32
PINS = os.path.join(os.path.dirname(__file__), "golden", "pcm16_sm_pins.json")
SYMBOLS = ("fz_run_block_pcm16_stream_major", "fz_program_pcm16_stream_major_resources", "fz_program_pcm16_stream_major_kernel_symbol",
           "fz_program_pcm16_stream_major_source", "fz_bank_process_pcm16_stream_major", "fz_bank_process_host_pcm16_stream_major")


def prog_of(name):
    return F.compile(F.from_sexpr(GG.SUPPORTED[name]()))


def test_the_c_abi_exports_the_six_symbols_and_capi_binds_them():
    raw = ctypes.CDLL(C.lib._name)
    for s in SYMBOLS:
        assert hasattr(raw, s), s
        assert getattr(C.lib, s).argtypes is not None, s
    for m in ("run_block_pcm16_stream_major", "pcm16_stream_major_resources", "pcm16_stream_major_kernel_symbol", "pcm16_stream_major_source"):
        assert callable(getattr(F.Program, m))
    for m in ("process_pcm16_stream_major", "process_host_pcm16_stream_major"):
        assert callable(getattr(F.Bank, m))


@pytest.mark.parametrize("name", sorted(GG.REFUSED))
def test_refusals_are_those_of_the_time_major_call_word_for_word(name):
    build, typed, word = GG.REFUSED[name]
    p = F.compile(F.from_sexpr(build()), typed=typed)
    assert C.lib.fz_run_block_pcm16(p._h, None, None, None, None, 64, 16, I16, I16, None) == C.FZ_E_UNSUPPORTED
    tm = C.last_error()
    assert C.lib.fz_run_block_pcm16_stream_major(p._h, None, None, None, None, 64, 16, 0, 16, I16, I16, None) == C.FZ_E_UNSUPPORTED
    assert C.last_error() == tm and word.lower() in tm.lower()
    for call in (p.pcm16_stream_major_kernel_symbol, p.pcm16_stream_major_resources, p.pcm16_stream_major_source):
        with pytest.raises(F.FlowzError) as ei:
            call()
        assert ei.value.code == C.FZ_E_UNSUPPORTED and str(tm) in str(ei.value)


# ---- argument checks: every one fails before the device is needed ------------------------------------------------------------------
class FakeBufs:
    """distinct, 16-byte aligned, never dereferenced addresses for the buffers of a call (none of these calls reaches a launch)"""

    def __init__(self, p, ns=1000, rows=64, row0=8, n=40):
        self.p, self.ns, self.rows, self.row0, self.n = p, ns, rows, row0, n
        self.in_, self.out, self.state, self.params = (1 << 40) + 0, (1 << 40) + (1 << 36), (1 << 40) + (2 << 36), (1 << 40) + (3 << 36)

    def run(self, it=I16, ot=I16, **over):
        a = {"in_": self.in_ if self.p.n_in else None, "out": self.out, "state": self.state if self.p.n_state else None,
             "params": self.params if self.p.n_param else None, "ns": self.ns, "rows": self.rows, "row0": self.row0, "n": self.n}
        a.update(over)
        return C.lib.fz_run_block_pcm16_stream_major(self.p._h, a["in_"], a["out"], a["state"], a["params"], a["ns"], a["rows"], a["row0"],
                                                     a["n"], it, ot, None)


def test_argument_checks():
    p = prog_of("df1_cascade_params6")                      # 1 in, 1 out, state and per-stream coefficients
    b = FakeBufs(p)
    for it, ot in ((2, I16), (I16, 2), (7, 7), (0xFFFFFFFF, I16)):
        assert b.run(it, ot) == C.FZ_E_INVALID and "frame type" in C.last_error()
    assert b.run(FLT, FLT) == C.FZ_E_INVALID and "fz_run_block" in C.last_error()           # float32 on both sides
    assert C.lib.fz_run_block_pcm16_stream_major(None, b.in_, b.out, b.state, b.params, 64, 16, 0, 16, I16, I16, None) == C.FZ_E_INVALID
    # an empty block is FZ_OK and touches nothing: not a pointer, not the window, not the grid is looked at
    assert b.run(n=0) == C.FZ_OK and b.run(ns=0) == C.FZ_OK
    assert b.run(n=0, in_=None, out=None, state=None, params=None, rows=3, row0=77) == C.FZ_OK
    # a window past rows_total
    assert b.run(row0=32, n=33) == C.FZ_E_INVALID and "rows_total" in C.last_error()
    assert b.run(row0=0xFFFFFFF8, n=16, rows=0xFFFFFFF8) == C.FZ_E_INVALID and "rows_total" in C.last_error()
    # the 16-byte grid of the pieces: multiples of 8 on an int16 side, of 4 on a float32 side, named with the side
    for kw in (dict(rows=68), dict(row0=4), dict(rows=60, row0=12)):
        assert b.run(I16, I16, **kw) == C.FZ_E_INVALID and "multiples of 8" in C.last_error() and "int16" in C.last_error(), kw
        assert C.last_error().startswith("in:")
    # int16 in and float32 out in ONE call: rows on the float grid but off the int16 grid fail on `in`, with 8; the other way round on `out`
    assert b.run(I16, FLT, rows=68, row0=4, n=8) == C.FZ_E_INVALID and "in:" in C.last_error() and "multiples of 8" in C.last_error()
    assert b.run(FLT, I16, rows=68, row0=4, n=8) == C.FZ_E_INVALID and "out:" in C.last_error() and "multiples of 8" in C.last_error()
    assert b.run(FLT, I16, rows=66, row0=0, n=8) == C.FZ_E_INVALID and "in:" in C.last_error() and "multiples of 4" in C.last_error() and "float32" in C.last_error()
    # pointers
    for over in ({"in_": b.in_ + 2}, {"in_": b.in_ + 8}, {"out": b.out + 4}, {"state": b.state + 4}, {"params": b.params + 8}):
        assert b.run(**over) == C.FZ_E_INVALID and "aligned" in C.last_error(), over
    for over in ({"in_": None}, {"out": None}, {"state": None}, {"params": None}):
        assert b.run(**over) == C.FZ_E_INVALID and "null" in C.last_error(), over
    # 2^30 streams or more
    few = dict(rows=8, row0=0, n=8)                          # (buffers of 2^30 streams that stay apart at the fake addresses)
    assert b.run(ns=1 << 30, **few) == C.FZ_E_UNSUPPORTED and "2^30" in C.last_error()
    assert b.run(ns=1 << 31, it=I16, ot=FLT, **few) == C.FZ_E_UNSUPPORTED
    # the order: the window is checked before the grid, the grid before the pointers, the pointers before the stream count
    assert b.run(rows=68, row0=60, n=40) == C.FZ_E_INVALID and "rows_total" in C.last_error()
    assert b.run(rows=68, in_=b.in_ + 2) == C.FZ_E_INVALID and "multiples of 8" in C.last_error()
    assert b.run(ns=1 << 30, in_=b.in_ + 2, **few) == C.FZ_E_INVALID and "aligned" in C.last_error()


def test_a_side_without_wires_takes_a_null_pointer_only():
    """a pointer is NULL iff its width is 0: the other direction, on a graph without input wires"""
    p = F.compile(F.from_sexpr(G.lit(0.5)))                  # no input, one output
    assert (p.n_in, p.n_out) == (0, 1)
    b = FakeBufs(p)
    assert b.run(I16, I16, in_=b.in_) == C.FZ_E_INVALID and "in must be null" in C.last_error()
    assert b.run(FLT, I16, in_=b.in_) == C.FZ_E_INVALID and "in must be null" in C.last_error()
    assert b.run(I16, I16, out=None) == C.FZ_E_INVALID and "out is null" in C.last_error()
    # (no wires on `in`: its type puts no rule on the rows -- rows on the int16 grid of `out` only)
    assert b.run(FLT, I16, rows=64, row0=8, in_=b.in_ + 4) == C.FZ_E_INVALID and "in must be null" in C.last_error()


def test_four_wires_need_no_multiple_of_eight_rows():
    """the rule is on rows x wires: four int16 wires are on the grid at every even row"""
    q = prog_of("par4_sum")                                  # 4 in, 1 out
    b = FakeBufs(q, rows=64, row0=8, n=8)
    assert b.run(I16, FLT, rows=66, row0=2, n=8) == C.FZ_E_INVALID and "out:" in C.last_error() and "multiples of 4" in C.last_error()
    assert b.run(I16, I16, rows=66, row0=2, n=8) == C.FZ_E_INVALID and "out:" in C.last_error() and "multiples of 8" in C.last_error()
    assert b.run(I16, I16, rows=65, row0=0, n=8) == C.FZ_E_INVALID and "in:" in C.last_error()


def test_in_place_allowed_and_refused():
    p = prog_of("df1_cascade6")                             # n_in == n_out == 1
    b = FakeBufs(p)
    i16_bytes, f32_bytes = 64 * 1000 * 2, 64 * 1000 * 4
    bad = [
        dict(it=I16, ot=I16, out=b.in_ + 16),                # shifted: not in place
        dict(it=I16, ot=I16, out=b.in_ + i16_bytes - 16),    # the tail of in (the WHOLE buffers count, not the window)
        dict(it=I16, ot=I16, out=b.in_ - i16_bytes + 16),
        dict(it=I16, ot=FLT, out=b.in_),                     # the same buffer, but the sides differ in type
        dict(it=FLT, ot=I16, out=b.in_),
        dict(it=FLT, ot=I16, out=b.in_ + f32_bytes - 16),
        dict(it=I16, ot=FLT, out=b.in_ - f32_bytes + 16),
    ]
    for kw in bad:
        assert b.run(**kw) == C.FZ_E_INVALID and "overlap" in C.last_error(), kw
    q = prog_of("par4_sum")                                  # four wires in, one out: never in place
    bq = FakeBufs(q)
    assert bq.run(out=bq.in_) == C.FZ_E_INVALID and "overlap" in C.last_error()
    # allowed: int16 both sides, n_in == n_out, in == out -- the call gets past every check and stops where it needs the device (or,
    # on a machine with one, is not made: the addresses are fake)
    if C.lib.fz_device_count() == 0:
        rc = b.run(out=b.in_)
        assert rc == C.FZ_E_NO_DEVICE, (rc, C.last_error())
        assert b.run(out=b.in_ + i16_bytes) == C.FZ_E_NO_DEVICE                # buffers that touch but do not overlap


# ---- the kernel JITs for gfx950 without a device ---------------------------------------------------------------------------------
SYMBOL = re.compile(r"^fz_pcm16_sm_kernel_i([01])o([01])u(8|16|32|64)b64_g([0-9a-f]{8})$")
TYPES = {"int16": 1, "float32": 0}
JIT_GRAPHS = ["integrator", "df1_cascade6", "par4_sum", "cross_wire"]
JIT_PAIRS = [("int16", "int16"), ("int16", "float32"), ("float32", "int16")]


def lds_formula(p, it, ot, U):
    """64 patch rows of [U x n_in samples][U x n_out samples][16 bytes]"""
    return 64 * (U * (p.n_in * (2 if it == "int16" else 4) + p.n_out * (2 if ot == "int16" else 4)) + 16)


@pytest.mark.parametrize("name", JIT_GRAPHS)
@pytest.mark.parametrize("it,ot", JIT_PAIRS)
def test_kernel_jits_without_spills_and_with_the_pinned_chunk(name, it, ot):
    p = prog_of(name)
    r = p.pcm16_stream_major_resources(it, ot)
    assert r["scratch_bytes"] == 0 and r["vgpr_spills"] == 0, r
    U = r["unroll"]
    assert r["lds_bytes"] == lds_formula(p, it, ot, U), r
    assert 4 * r["lds_bytes"] <= 160 * 1024                                      # four waves fit a CU's LDS
    s = p.pcm16_stream_major_kernel_symbol(it, ot)
    m = SYMBOL.match(s)
    assert m, s
    assert (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (TYPES[it], TYPES[ot], U)
    assert m.group(4) == p.kernel_symbol().split("_g")[-1]
    src = p.pcm16_stream_major_source(it, ot)
    assert f"#define FZ_KERNEL {s}\n" in src and "fz_pcm16_sm_kernel -- hand-written gfx950" in src and "struct fz_graph" in src
    assert "fz_pcm16_kernel -- hand-written gfx950" not in src                    # a text of its own
    pin = json.load(open(PINS))[f"{name}:{it}:{ot}"]
    assert pin == {"symbol": s, "chunk_rows": U, "lds_bytes": r["lds_bytes"]}, (pin, s, r)


def test_a_graph_that_spills_at_every_chunk_length_still_gets_a_kernel():
    """the halving of the chunk stops at 8 rows, one int16 piece: a heavy graph runs that kernel with its spills, as it does on the
    time-major PCM kernel and on the float32 stream-major kernel -- it is not a compile error"""
    p = F.compile(F.from_sexpr(G.df1_cascade_params(48)))
    assert p.pcm16_supported()
    for it, ot in JIT_PAIRS:
        r = p.pcm16_stream_major_resources(it, ot)
        s = p.pcm16_stream_major_kernel_symbol(it, ot)
        m = SYMBOL.match(s)
        assert m and int(m.group(3)) == r["unroll"] and r["unroll"] >= 8 and r["unroll"] % 8 == 0, (s, r)
        assert r["lds_bytes"] == lds_formula(p, it, ot, r["unroll"])
        assert r["unroll"] == 8 or r["scratch_bytes"] == 0, r                      # (halved as far as it goes before spills are accepted)
        assert f"#define FZ_KERNEL {s}\n" in p.pcm16_stream_major_source(it, ot)


def test_the_chunk_rule_on_the_pinned_graphs():
    """64 rows for one int16 wire, 32 for two, 16 for four -- the narrowest int16 side decides --, halved until four patches fit 160 KB"""
    pins = json.load(open(PINS))
    want = {"integrator": (64, 64, 64), "df1_cascade6": (64, 64, 64),
            "par4_sum": (32, 16, 32),         # i16 -> i16: the one-wire out-run asks for 64 rows, 42 KB a wave: halved once; i16 -> f32: four wires, 16 rows
            "cross_wire": (64, 32, 32)}       # i16 -> f32: 64 rows are 41 KB a wave: halved once; f32 -> i16: two int16 wires, 32 rows
    for name, us in want.items():
        for (it, ot), U in zip(JIT_PAIRS, us):
            assert pins[f"{name}:{it}:{ot}"]["chunk_rows"] == U, (name, it, ot)


def test_float32_on_both_sides_and_bad_types_have_no_kernel():
    p = prog_of("integrator")
    with pytest.raises(F.FlowzError) as ei:
        p.pcm16_stream_major_kernel_symbol("float32", "float32")
    assert ei.value.code == C.FZ_E_INVALID
    buf = ctypes.create_string_buffer(160)
    assert C.lib.fz_program_pcm16_stream_major_kernel_symbol(p._h, 3, 1, buf, 160) == C.FZ_E_INVALID
    assert C.lib.fz_program_pcm16_stream_major_kernel_symbol(None, 1, 1, buf, 160) == C.FZ_E_INVALID


PCM, PCM_SM = 1 << 12, 1 << 13


def test_a_callers_variant_still_cannot_name_the_kernel():
    p = prog_of("integrator")
    for flags in (PCM_SM, PCM | PCM_SM | 1 | 2, PCM | 1 | 2 | 128):
        with pytest.raises(F.FlowzError) as ei:
            p.kernel_symbol(F.make_variant(1, 64, 64, flags), 4096, 64)
        assert ei.value.code == C.FZ_E_INVALID


def test_manifest_replay_asks_whether_a_stream_major_pcm_record_fits(tmp_path):
    """a manifest is data from elsewhere: records no fz_run_block_pcm16_stream_major launch could have made are counted as failed"""
    def record(prog_expr, typed, P, U, block, flags):
        buf = ctypes.create_string_buffer(1 << 16)
        n = C.lib.fz_expr_recipe(prog_expr._h, buf, 1 << 16)
        recipe = f"typed {typed}\n".encode() + buf.raw[:n]
        return f"FZM1 {P} {U} {block} {flags} {len(recipe)}\n".encode() + recipe
    good = F.from_sexpr(GG.SUPPORTED["integrator"]())
    ring = F.from_sexpr(GG.REFUSED["lds_ring_comb"][0]())
    K = PCM | PCM_SM
    recs = [
        record(good, 0, 1, 64, 64, K | 1 | 2),                # what a launch makes: at hand or built
        record(good, 0, 1, 128, 64, K | 1 | 2),               # chunks longer than the rule's
        record(good, 0, 1, 48, 64, K | 1 | 2),                # no power of two
        record(good, 0, 1, 64, 256, K | 1 | 2),               # another workgroup
        record(good, 0, 1, 64, 64, K),                        # float32 on both sides
        record(good, 0, 2, 64, 64, K | 1 | 2),                # two streams per lane
        record(good, 0, 1, 64, 64, K | 1 | 2 | 4),            # the 2-byte bit of the time-major kernel next to it
        record(ring, 0, 1, 64, 64, K | 1 | 2),                # a graph the PCM kernels refuse
    ]
    path = tmp_path / "m.fzm"
    path.write_bytes(b"".join(recs))
    r = F.manifest_build(str(path))
    assert r["records"] == 8 and r["failed"] == 7 and r["at_hand"] + r["built"] == 1, r
