"""16-bit PCM on stream-major buffers on the MI355X (fz_run_block_pcm16_stream_major): every bit against the oracle's float32 forward
on pcm16_ref.to_float(q) and the output rule of tests/pcm16_ref.py, as tests/test_pcm16_gpu.py gets its expected values.  No tolerance
anywhere.

Shapes are the smallest at which this kernel can go wrong: one lane, a short last wave, a full wave, a wave of one lane, several
waves; blocks below one chunk (the row-by-row tail only), one row short of a chunk, a whole chunk, one row more, and two chunks plus
three rows (the held pieces of the prefetch and the tail); a window that is the whole buffer and one inside a longer buffer.  U, the
rows of a chunk, is asked of the library per graph and type pair.  The cells are a cross, not the full product (CELLS below, with the
coverage asserted).
"""
import functools

import numpy as np
import pytest

import grad_graphs as GG
import graphs as G
import pcm16_ref as R
from oracle import flowz_oracle as O

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

F32 = np.float32
STREAMS = (1, 63, 64, 65, 257)
LENGTHS = ("tail", "U-1", "U", "U+1", "2U+3")
WINDOWS = ("whole", "inside")
# 1-in / 1-out twice, 2-in / 1-out, 4-in / 1-out, two outputs, per-stream coefficients
GRAPHS = ("integrator", "df1_cascade6", "two_wire_mix", "par4_sum", "cross_wire", "df1_cascade_params6")
PAIRS = (("int16", "int16"), ("int16", "float32"), ("float32", "int16"))
# Input amplitude in int16 counts per graph, so that the expected int16 output is neither constant nor pinned to the rails (asserted per
# cell: under 10 % of samples at a saturation value, at least half non-zero).  The integrator sums its input: a small amplitude; the
# sum of four band-passes and the cascades stay inside the range at a quarter of full scale; the cascade with per-stream coefficients
# runs with b0 near a half (params_of) and an eighth.  Checked on the CPU with the oracle.
AMPLITUDE = {"integrator": 40, "df1_cascade6": 8000, "two_wire_mix": 8000, "par4_sum": 4000, "cross_wire": 8000, "df1_cascade_params6": 4000}


def two_wire_mix():
    """2-in / 1-out with a delay line: 0.5 * _1[_1] + 0.25 * _2"""
    return G.add(G.mul(G.lit(0.5), G.DEL(1, 1)), G.mul(G.lit(0.25), G.IN(2)))


SEXPR = dict(GG.SUPPORTED, two_wire_mix=two_wire_mix)

# the cross: cell i of a type pair takes graph i, and walks the other axes at different strides, so that every value of every axis
# meets every type pair
CELLS = [(GRAPHS[i], pair, STREAMS[(i + k) % 5], LENGTHS[(2 * i + k) % 5], WINDOWS[(i + k) % 2])
         for k, pair in enumerate(PAIRS) for i in range(len(GRAPHS))]


def test_the_cross_covers_every_axis_value_with_every_type_pair():
    for pair in PAIRS:
        mine = [c for c in CELLS if c[1] == pair]
        assert {c[0] for c in mine} == set(GRAPHS)
        assert {c[2] for c in mine} == set(STREAMS)
        assert {c[3] for c in mine} == set(LENGTHS)
        assert {c[4] for c in mine} == set(WINDOWS)


@pytest.fixture(scope="module")
def F():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    torch.cuda.set_device(0)
    from zignal_amd import flowz
    return flowz


_progs = {}


def prog(F, name, sexpr=None):
    if name not in _progs:
        _progs[name] = F.compile(F.from_sexpr(sexpr if sexpr is not None else SEXPR[name]()))
    return _progs[name]


def dev(a):
    return torch.from_numpy(np.array(a)).cuda() if a is not None else None     # (a copy: the shared references are read-only)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.uint32), b.view(np.uint32)))


def tdtype(name):
    return torch.int16 if name == "int16" else torch.float32


def chunk_rows(p, pair):
    return p.pcm16_stream_major_resources(*pair)["unroll"]


def length_of(kind, U):
    return {"tail": 3, "U-1": U - 1, "U": U, "U+1": U + 1, "2U+3": 2 * U + 3}[kind]


def window_of(kind, n, row0_inside=8):
    """(rows_total, row0): the whole buffer (n rounded up to the grid of 8 rows), or a window inside a longer one"""
    n8 = (n + 7) // 8 * 8
    return (n8, 0) if kind == "whole" else (row0_inside + n8 + 8, row0_inside)


def params_of(p, ns, seed):
    if not p.n_param:
        return None
    rng = np.random.default_rng(seed)
    par = np.empty((p.n_param, ns), F32)
    for j in range(p.n_param // 5):
        par[5 * j:5 * j + 5] = np.asarray(G.STABLE, F32)[:, None] * rng.uniform(0.9, 1.0, (5, ns)).astype(F32)
        # (b0 near a half: with the 0.05 of STABLE six stages in a row give a block of three rows nothing but zeros)
        par[5 * j] = rng.uniform(0.4, 0.5, ns).astype(F32)
    return par


@functools.lru_cache(maxsize=None)
def reference(name, ns, rows, seed=0):
    """(q [ns, rows, n_in] int16, params, the oracle's float32 output [rows, ns, n_out] when rows [0, rows) are ONE block): computed
    once per shape, shared, never changed"""
    from zignal_amd import flowz
    p = prog(flowz, name)
    a = AMPLITUDE[name]
    q = np.random.default_rng(1000 + ns + 7 * rows + seed).integers(-a, a + 1, (ns, rows, p.n_in), dtype=np.int16)
    par = params_of(p, ns, 7 + ns)
    want = O.compile(SEXPR[name](), ns, params=par).run(np.ascontiguousarray(R.to_float(q).transpose(1, 0, 2)))
    want = np.ascontiguousarray(want, F32)
    for a_ in (q, want):
        a_.setflags(write=False)
    return q, par, want


def assert_not_constant(want16):
    """the condition on the inputs: no cell compares constants"""
    sat = np.mean((want16 == 32767) | (want16 == -32768))
    assert sat < 0.10 and np.mean(want16 != 0) >= 0.5, (float(sat), float(np.mean(want16 != 0)))


SENTINEL = {"int16": 0x5A5A, "float32": 12345.0}
PAD = 64


def padded_out(ns, rows, n_out, odt):
    """out [ns, rows, n_out] full of sentinels inside an allocation with 64 more sentinels on either side"""
    n = ns * rows * n_out
    big = torch.full((PAD + n + PAD,), SENTINEL[odt], dtype=tdtype(odt), device="cuda")
    out = big[PAD:PAD + n].view(ns, rows, n_out)
    assert out.data_ptr() % 16 == 0
    return big, out


# ---- 1, 2, 7: bits, untouched rows, inputs that are no constants ------------------------------------------------------------------------
@pytest.mark.parametrize("name,pair,ns,length,window", CELLS)
def test_parity_with_the_oracle_the_float_path_and_the_time_major_state(F, name, pair, ns, length, window):
    p = prog(F, name)
    it, ot = pair
    U = chunk_rows(p, pair)
    n = length_of(length, U)
    rows, row0 = window_of(window, n, 8 if ns % 2 else 16)
    q, par, want = reference(name, ns, n)                                        # the window's rows as one block from zero state
    want_sm = np.ascontiguousarray(want.transpose(1, 0, 2))                       # [ns, n, n_out]
    want16 = R.from_float(want_sm)
    assert_not_constant(want16)
    # the buffers: the window's rows hold q, the rows around it other samples
    qbuf = np.random.default_rng(5 + ns).integers(-30000, 30000, (ns, rows, p.n_in), dtype=np.int16)
    qbuf[:, row0:row0 + n] = q
    x = dev(qbuf) if it == "int16" else dev(R.to_float(qbuf))
    big, out = padded_out(ns, rows, p.n_out, ot)
    y, st = p.run_block_pcm16_stream_major(x, params=dev(par), out=out, out_dtype=tdtype(ot), row0=row0, n_samples=n)
    assert y.data_ptr() == out.data_ptr()
    b = host(big)
    got = b[PAD:-PAD].reshape(ns, rows, p.n_out)
    if ot == "int16":
        assert np.array_equal(got[:, row0:row0 + n], want16), int((got[:, row0:row0 + n] != want16).sum())
    else:
        assert same_bits(got[:, row0:row0 + n], want_sm)
        # ... and fz_run_block_stream_major on the converted input, on the device
        y32, _ = p.run_block_stream_major(dev(R.to_float(qbuf)), params=dev(par), row0=row0, n_samples=n)
        assert same_bits(host(y32)[:, row0:row0 + n], got[:, row0:row0 + n])
    # rows outside the window and what lies around the buffer keep the sentinel
    s = SENTINEL[ot]
    assert (got[:, :row0] == s).all() and (got[:, row0 + n:] == s).all(), "a row outside the window was written"
    assert (b[:PAD] == s).all() and (b[-PAD:] == s).all(), "a sentinel next to out has changed"
    # the state after the block: that of the time-major PCM kernel on the transposed frames, the same bits
    xt = np.ascontiguousarray(q.transpose(1, 0, 2))
    _, st_tm = p.run_block_pcm16(dev(xt) if it == "int16" else dev(R.to_float(xt)), params=dev(par), out_dtype=tdtype(ot))
    assert same_bits(host(st)[:p.n_state], host(st_tm)[:p.n_state])


# ---- 3: chaining with the time-major PCM kernel on one state buffer ---------------------------------------------------------------------
@pytest.mark.parametrize("name,ns", (("df1_cascade6", 65), ("cross_wire", 63)))
def test_windows_chain_with_time_major_pcm_blocks_on_one_state(F, name, ns):
    p = prog(F, name)
    U = chunk_rows(p, ("int16", "int16"))
    n = 2 * U + 8
    q, par, want = reference(name, ns, n, seed=3)
    want16 = R.from_float(np.ascontiguousarray(want.transpose(1, 0, 2)))
    x = dev(q)
    out = torch.full((ns, n, p.n_out), 0x5A5A, dtype=torch.int16, device="cuda")
    # one block, for its state
    _, st_one = p.run_block_pcm16_stream_major(x)
    # rows [0, 1) stream-major, rows [1, U) time-major on the transposed piece (row 1 is off the stream-major grid), rows [U, n) stream-major
    _, st = p.run_block_pcm16_stream_major(x, out=out, row0=0, n_samples=1)
    piece = dev(np.ascontiguousarray(q[:, 1:U].transpose(1, 0, 2)))
    ymid, st = p.run_block_pcm16(piece, state=st)
    _, st = p.run_block_pcm16_stream_major(x, state=st, out=out, row0=U, n_samples=n - U)
    got = host(out)
    assert np.array_equal(got[:, :1], want16[:, :1]) and np.array_equal(got[:, U:], want16[:, U:])
    assert np.array_equal(host(ymid).transpose(1, 0, 2), want16[:, 1:U])
    assert (got[:, 1:U] == 0x5A5A).all()
    assert same_bits(host(st)[:p.n_state], host(st_one)[:p.n_state])


# ---- 4: in place ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns", (65, 257))
def test_in_place_equals_out_of_place(F, ns):
    p = prog(F, "df1_cascade6")                                                   # int16 both sides, n_in == n_out
    U = chunk_rows(p, ("int16", "int16"))
    n = 2 * U + 3
    rows, row0 = window_of("inside", n)
    q, _, want = reference("df1_cascade6", ns, n, seed=4)
    qbuf = np.random.default_rng(6 + ns).integers(-30000, 30000, (ns, rows, 1), dtype=np.int16)
    qbuf[:, row0:row0 + n] = q
    y, st = p.run_block_pcm16_stream_major(dev(qbuf), row0=row0, n_samples=n)
    buf = dev(qbuf)
    y2, st2 = p.run_block_pcm16_stream_major(buf, out=buf, row0=row0, n_samples=n)
    assert y2.data_ptr() == buf.data_ptr()
    got, inp = host(y), host(buf)
    assert np.array_equal(inp[:, row0:row0 + n], got[:, row0:row0 + n])
    assert np.array_equal(inp[:, row0:row0 + n], R.from_float(np.ascontiguousarray(want.transpose(1, 0, 2))))
    assert np.array_equal(inp[:, :row0], qbuf[:, :row0]) and np.array_equal(inp[:, row0 + n:], qbuf[:, row0 + n:])
    assert same_bits(host(st), host(st2))


# ---- 5: the rule's edges through the kernel ---------------------------------------------------------------------------------------------
def test_the_edges_of_the_output_rule_through_the_kernel(F):
    p = prog(F, "gain_one", G.mul(G.IN(1), G.lit(1.0)))
    U = chunk_rows(p, ("float32", "int16"))
    s = F32(1.0) / F32(32768)
    values = np.array([np.nan, np.inf, -np.inf, F32(32767.5) * s, F32(-32767.5) * s, F32(0.5) * s, F32(1.5) * s, F32(2.5) * s,
                       F32(-0.5) * s, F32(-1.5) * s, F32(-2.5) * s, -1.0, np.nextafter(F32(1.0), F32(0.0)), 1.0, 0.0, -0.0], F32)
    by_hand = np.array([0, 32767, -32768, 32767, -32768, 0, 2, 2, 0, -2, -2, -32768, 32767, 32767, 0, 0], np.int16)
    assert np.array_equal(R.from_float(values), by_hand)                          # the numpy rule agrees with the hand-written answers
    ns, n = 65, U + 5                                                             # a whole chunk through the pieces, five rows through the tail
    rows = (n + 7) // 8 * 8
    # every stream starts at another value: each value meets the chunk path and the tail path
    idx = (np.arange(ns)[:, None] + np.arange(rows)[None, :]) % len(values)
    x = values[idx][:, :, None]
    y, _ = p.run_block_pcm16_stream_major(dev(x), out_dtype=torch.int16, n_samples=n)
    got = host(y)[:, :n, 0]
    assert np.array_equal(got, by_hand[idx][:, :n]), int((got != by_hand[idx][:, :n]).sum())
    assert np.array_equal(got, R.from_float(x[:, :n, 0]))


# ---- 6: the host path ---------------------------------------------------------------------------------------------------------------------
class DeviceFloats:
    """a bank's state rows as torch sees them (fz_bank_state_device is a raw device pointer)"""

    def __init__(self, ptr, shape):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": "<f4", "data": (int(ptr), False), "version": 2}


def bank_state(F, bank):
    p = bank.prog
    ptr = F.C.lib.fz_bank_state_device(bank._h)
    return host(torch.as_tensor(DeviceFloats(ptr, (p.n_state, bank.n_streams)), device="cuda").clone())


# fz_bank.cpp: time chunks of 32 MiB on the wider side, whole multiples of 32 rows -- a second chunk would take 64 MiB each way at any
# stream count.  FLOWZ_HIP_HOST_CHUNK_BYTES (read at every call) sets another chunk size: with 16 KiB, eight streams of one int16 wire
# are 16 bytes a row and 1024 rows a chunk; two chunks and 13 rows (no multiple of 8) are 33 KB each way, three trips of the pipeline.
HOST_NS, HOST_CHUNK_BYTES = 8, 16 << 10
HOST_ROWS = 2 * (HOST_CHUNK_BYTES // (HOST_NS * 2) // 32 * 32) + 13


@pytest.mark.parametrize("memory", ("pageable numpy", "pinned torch"))
def test_host_path_over_several_time_chunks(F, monkeypatch, memory):
    ns, n = HOST_NS, HOST_ROWS
    assert n % 8 and n > 2 * 1024
    monkeypatch.setenv("FLOWZ_HIP_HOST_CHUNK_BYTES", str(HOST_CHUNK_BYTES))
    p = prog(F, "df1_cascade6")
    q, _, want = reference("df1_cascade6", ns, n, seed=8)
    want16 = R.from_float(np.ascontiguousarray(want.transpose(1, 0, 2)))
    assert_not_constant(want16)
    a, b = p.bank(ns), p.bank(ns)
    if memory == "pinned torch":
        got = a.process_host_pcm16_stream_major(torch.from_numpy(np.array(q)).pin_memory())
        assert got.dtype == torch.int16 and got.is_pinned()
        got = got.numpy()
    else:
        got = a.process_host_pcm16_stream_major(np.array(q))
        assert got.dtype == np.int16
    assert got.shape == (ns, n, 1)
    tm = b.process_host_pcm16(np.ascontiguousarray(q.transpose(1, 0, 2)))
    assert np.array_equal(got, tm.transpose(1, 0, 2))
    assert np.array_equal(got, want16)
    assert same_bits(bank_state(F, a), bank_state(F, b))
    # a second call goes on from the state the first left, chunked the same way
    got2 = a.process_host_pcm16_stream_major(np.array(q[:, :45]))
    tm2 = b.process_host_pcm16(np.ascontiguousarray(q[:, :45].transpose(1, 0, 2)))
    assert np.array_equal(got2, tm2.transpose(1, 0, 2))
    assert same_bits(bank_state(F, a), bank_state(F, b))


def test_host_path_on_pinned_torch_tensors(F):
    ns, n = 257, 45
    p = prog(F, "cross_wire")
    q, _, want = reference("cross_wire", ns, n, seed=6)
    a, b = p.bank(ns), p.bank(ns)
    got = a.process_host_pcm16_stream_major(torch.from_numpy(np.array(q)).pin_memory())
    assert got.dtype == torch.int16 and got.is_pinned()
    assert np.array_equal(got.numpy(), R.from_float(np.ascontiguousarray(want.transpose(1, 0, 2))))
    tm = b.process_host_pcm16(np.ascontiguousarray(q.transpose(1, 0, 2)))
    assert np.array_equal(got.numpy(), tm.transpose(1, 0, 2))
    assert same_bits(bank_state(F, a), bank_state(F, b))
    # the device entry point on the bank's state: the same block again from where the host call left the state
    c = p.bank(ns)
    rows = (n + 7) // 8 * 8
    qbuf = np.zeros((ns, rows, 1), np.int16)
    qbuf[:, :n] = q
    y = c.process_pcm16_stream_major(dev(qbuf), n_samples=n)
    assert np.array_equal(host(y)[:, :n], got.numpy())
    assert same_bits(bank_state(F, c), bank_state(F, a))
