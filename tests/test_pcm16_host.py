"""16-bit PCM frames without a GPU: the support matrix, argument checks (each fails before a device is needed), the PCM kernel's JIT
for gfx950 -- registers, scratch, symbol -- and tests/pcm16_ref.py, the numpy statement of the conversion rule the GPU tests hold the
kernel to, on hand-written cases.  (That every existing kernel keeps its source and code id is what tests/test_plan_pins_host.py,
test_delay_lines_host.py, test_graph_functions_host.py and test_grad_stream_major_host.py assert; they pass unchanged.)"""
import ctypes
import re

import numpy as np
import pytest

import grad_graphs as GG
import graphs as G
import pcm16_ref as R
from zignal_amd import _capi as C
from zignal_amd import flowz as F

F32 = np.float32
I16, FLT = C.FZ_FRAMES_I16, C.FZ_FRAMES_F32


def prog_of(name):
    return F.compile(F.from_sexpr(GG.SUPPORTED[name]()))


# ---- the support matrix ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(GG.SUPPORTED))
def test_supported_graphs_pass_the_check(name):
    p = prog_of(name)
    assert C.lib.fz_program_pcm16_check(p._h) == C.FZ_OK, C.last_error()
    assert p.pcm16_supported() and p.pcm16_unsupported_reason() == ""


@pytest.mark.parametrize("name", sorted(GG.REFUSED))
def test_refusals_name_their_reason(name):
    build, typed, word = GG.REFUSED[name]
    p = F.compile(F.from_sexpr(build()), typed=typed)
    assert C.lib.fz_program_pcm16_check(p._h) == C.FZ_E_UNSUPPORTED
    assert word.lower() in C.last_error().lower(), C.last_error()
    assert not p.pcm16_supported() and word.lower() in p.pcm16_unsupported_reason().lower()
    for call in (p.pcm16_kernel_symbol, p.pcm16_resources, p.pcm16_source):
        with pytest.raises(F.FlowzError) as ei:
            call()
        assert ei.value.code == C.FZ_E_UNSUPPORTED
    # the launch refuses it too, before it looks at a pointer or a device
    assert C.lib.fz_run_block_pcm16(p._h, None, None, None, None, 64, 16, I16, I16, None) == C.FZ_E_UNSUPPORTED


# ---- argument checks: every one fails before the device is needed ------------------------------------------------------------------
class FakeBufs:
    """distinct, 16-byte aligned, never dereferenced addresses for the buffers of a call (none of these calls reaches a launch)"""

    def __init__(self, p, ns, T):
        self.p, self.ns, self.T = p, ns, T
        self.in_, self.out, self.state, self.params = (1 << 40) + 0, (1 << 40) + (1 << 36), (1 << 40) + (2 << 36), (1 << 40) + (3 << 36)

    def run(self, it=I16, ot=I16, ns=None, T=None, **over):
        a = {"in_": self.in_ if self.p.n_in else None, "out": self.out, "state": self.state if self.p.n_state else None,
             "params": self.params if self.p.n_param else None}
        a.update(over)
        return C.lib.fz_run_block_pcm16(self.p._h, a["in_"], a["out"], a["state"], a["params"], self.ns if ns is None else ns,
                                        self.T if T is None else T, it, ot, None)


def test_argument_checks():
    p = prog_of("df1_cascade_params6")                      # 1 in, 1 out, state and per-stream coefficients
    b = FakeBufs(p, 1000, 40)
    for it, ot in ((2, I16), (I16, 2), (7, 7), (0xFFFFFFFF, I16)):
        assert b.run(it, ot) == C.FZ_E_INVALID and "frame type" in C.last_error()
    assert b.run(FLT, FLT) == C.FZ_E_INVALID and "fz_run_block" in C.last_error()
    for over in ({"in_": b.in_ + 2}, {"in_": b.in_ + 8}, {"out": b.out + 4}, {"state": b.state + 4}, {"params": b.params + 8}):
        assert b.run(**over) == C.FZ_E_INVALID and "aligned" in C.last_error(), over
    for over in ({"in_": None}, {"out": None}, {"state": None}, {"params": None}):
        assert b.run(**over) == C.FZ_E_INVALID and "null" in C.last_error(), over
    assert C.lib.fz_run_block_pcm16(None, b.in_, b.out, b.state, b.params, 64, 16, I16, I16, None) == C.FZ_E_INVALID
    # an empty block is FZ_OK and touches nothing (not a pointer is looked at)
    assert b.run(T=0) == C.FZ_OK and b.run(ns=0) == C.FZ_OK
    assert b.run(T=0, in_=None, out=None, state=None, params=None) == C.FZ_OK
    assert b.run(T=0xFFFFFFFF) == C.FZ_E_INVALID


def test_forbidden_overlaps():
    p = prog_of("df1_cascade6")                             # n_in == n_out == 1
    b = FakeBufs(p, 1000, 40)
    i16_bytes, f32_bytes = 40 * 1000 * 2, 40 * 1000 * 4
    bad = [
        dict(it=I16, ot=I16, out=b.in_ + 16),                # shifted: not in place
        dict(it=I16, ot=I16, out=b.in_ + i16_bytes - 16),    # the tail of in
        dict(it=I16, ot=I16, out=b.in_ - i16_bytes + 16),    # out's tail reaches into in
        dict(it=I16, ot=FLT, out=b.in_),                     # the same buffer, but the sides differ in type
        dict(it=FLT, ot=I16, out=b.in_),
        dict(it=FLT, ot=I16, out=b.in_ + f32_bytes - 16),
        dict(it=I16, ot=FLT, out=b.in_ - f32_bytes + 16),
    ]
    for kw in bad:
        assert b.run(**kw) == C.FZ_E_INVALID and "overlap" in C.last_error(), kw
    q = prog_of("par4_sum")                                  # four wires in, one out: never in place
    bq = FakeBufs(q, 1000, 40)
    assert bq.run(out=bq.in_) == C.FZ_E_INVALID and "overlap" in C.last_error()


def test_rows_of_4_gib_are_unsupported():
    q = prog_of("par4_sum")                                  # an int16 input row of 2^29 streams x 4 wires x 2 bytes
    assert FakeBufs(q, 1 << 29, 4).run() == C.FZ_E_UNSUPPORTED and "4 GiB" in C.last_error()
    assert FakeBufs(q, 1 << 29, 4).run(FLT, I16) == C.FZ_E_UNSUPPORTED and "4 GiB" in C.last_error()
    p = prog_of("df1_cascade6")
    assert FakeBufs(p, 1 << 30, 4).run(I16, FLT) == C.FZ_E_UNSUPPORTED
    assert FakeBufs(p, 1 << 31, 4).run() == C.FZ_E_UNSUPPORTED


# ---- the kernel JITs for gfx950 without a device ---------------------------------------------------------------------------------
SYMBOL = re.compile(r"^fz_pcm16_kernel_i([01])o([01])p([24])u([1248])b256(h?)(m?)_g([0-9a-f]{8})$")
TYPES = {"int16": 1, "float32": 0}


@pytest.mark.parametrize("name", ["integrator", "df1_cascade6", "par4_sum", "cross_wire"])
@pytest.mark.parametrize("it,ot", [("int16", "int16"), ("int16", "float32"), ("float32", "int16")])
def test_kernel_jits_without_spills_on_and_off_the_dword_grid(name, it, ot):
    p = prog_of(name)
    syms = []
    for ns in (1048576, 1000001):
        r = p.pcm16_resources(it, ot, ns)
        assert r["scratch_bytes"] == 0 and r["vgpr_spills"] == 0, (ns, r)
        assert r["lds_bytes"] == 0 and 0 < r["vgprs"] <= 256
        s = p.pcm16_kernel_symbol(it, ot, ns)
        m = SYMBOL.match(s)
        assert m, s
        assert (int(m.group(1)), int(m.group(2))) == (TYPES[it], TYPES[ot])
        assert int(m.group(4)) == r["unroll"]
        assert m.group(7) == p.kernel_symbol().split("_g")[-1]
        # off the dword grid: streams x wires odd on an int16 side -> 2-byte accesses, two streams per lane
        off = (it == "int16" and (ns * p.n_in) % 2 == 1) or (ot == "int16" and (ns * p.n_out) % 2 == 1)
        assert (m.group(5) == "h") == off, s
        assert int(m.group(3)) == (2 if off or max(p.n_in, p.n_out) > 2 else 4), s
        src = p.pcm16_source(it, ot, ns)
        assert f"#define FZ_KERNEL {s}\n" in src and "fz_pcm16_kernel -- hand-written gfx950" in src and "struct fz_graph" in src
        syms.append(s)
    # the two stream counts run different kernels: 1 000 001 streams are off the 64-byte store grid on every side (m), and off the
    # dword grid (h) wherever an int16 side has an odd number of wires
    assert syms[0] != syms[1] and syms[0].endswith("b256_g" + syms[0][-8:]) and syms[1].split("_g")[0].endswith("m")


def test_float32_on_both_sides_and_bad_types_have_no_kernel():
    p = prog_of("integrator")
    with pytest.raises(F.FlowzError) as ei:
        p.pcm16_kernel_symbol("float32", "float32")
    assert ei.value.code == C.FZ_E_INVALID
    buf = ctypes.create_string_buffer(160)
    assert C.lib.fz_program_pcm16_kernel_symbol(p._h, 3, 1, 64, buf, 160) == C.FZ_E_INVALID


def test_a_callers_variant_cannot_name_the_pcm_kernel():
    """the flag bits that name it stay reserved for callers"""
    p = prog_of("integrator")
    for flags in (1 << 12, (1 << 12) | 1 | 2):
        with pytest.raises(F.FlowzError) as ei:
            p.kernel_symbol(F.make_variant(2, 8, 256, flags), 4096, 64)
        assert ei.value.code == C.FZ_E_INVALID


def test_manifest_replay_asks_whether_a_pcm_record_fits(tmp_path):
    """a manifest is data from elsewhere: records no fz_run_block_pcm16 launch could have made are counted as failed, not built"""
    def record(prog_expr, typed, P, U, block, flags):
        buf = ctypes.create_string_buffer(1 << 16)
        n = C.lib.fz_expr_recipe(prog_expr._h, buf, 1 << 16)
        recipe = f"typed {typed}\n".encode() + buf.raw[:n]
        return f"FZM1 {P} {U} {block} {flags} {len(recipe)}\n".encode() + recipe
    PCM = 1 << 12
    good = F.from_sexpr(GG.SUPPORTED["integrator"]())
    ring = F.from_sexpr(GG.REFUSED["lds_ring_comb"][0]())
    recs = [
        record(good, 0, 4, 8, 256, PCM | 1 | 2),              # what a launch makes: at hand or built
        record(good, 0, 2, 8, 256, PCM | 1 | 2),              # two streams per lane on the grid: no plan of this graph
        record(good, 0, 4, 16, 256, PCM | 1 | 2),             # chunks longer than the plan's
        record(good, 0, 4, 8, 128, PCM | 1),                  # another workgroup
        record(good, 0, 4, 8, 256, PCM),                      # float32 on both sides
        record(good, 0, 4, 8, 256, PCM | 1 | 2 | 64),         # a forward flag next to it
        record(ring, 0, 4, 8, 256, PCM | 1 | 2),              # a graph the PCM kernel refuses
    ]
    path = tmp_path / "m.fzm"
    path.write_bytes(b"".join(recs))
    r = F.manifest_build(str(path))
    assert r["records"] == 7 and r["failed"] == 6 and r["at_hand"] + r["built"] == 1, r


# ---- the conversion rule as a numpy function ------------------------------------------------------------------------------------
def test_input_conversion_is_exact():
    q = np.arange(-32768, 32768, dtype=np.int16)
    x = R.to_float(q)
    assert x.dtype == F32 and x[0] == F32(-1.0) and x[-1] == F32(32767 / 32768)
    assert np.array_equal(x.astype(np.float64) * 32768, q.astype(np.float64))     # no rounding anywhere
    assert np.array_equal(R.from_float(x), q)                                      # and the rule inverts it


def test_output_rule_on_hand_written_cases():
    s = F32(1.0) / F32(32768)
    cases = [
        (0.5, 0), (-0.5, 0), (1.5, 2), (2.5, 2), (-1.5, -2), (-2.5, -2), (3.5, 4),            # ties go to even
        (32766.5, 32766), (32767.5, 32767), (-32768.5, -32768), (32767.0, 32767), (-32768.0, -32768),
        (32766.49, 32766), (-32767.5, -32768), (40000.0, 32767), (-40000.0, -32768),
    ]
    for v, want in cases:
        y = F32(v) * s                                                                       # (exact: a power of two)
        assert float(y) * 32768 == float(F32(v))
        assert R.from_float(np.array([y], F32))[0] == want, (v, want)
    special = np.array([np.inf, -np.inf, np.nan, -np.nan, 1e-45, -1e-45, 1e-39, -0.0, 0.0, 3.4e38, -3.4e38], F32)
    assert R.from_float(special).tolist() == [32767, -32768, 0, 0, 0, 0, 0, 0, 0, 32767, -32768]
    assert R.from_float(special).dtype == np.int16
