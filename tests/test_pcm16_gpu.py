"""16-bit PCM frames on the MI355X (fz_run_block_pcm16): every bit against the float32 path and the conversion rule of
tests/pcm16_ref.py.  No tolerance anywhere: a float32 output of the PCM kernel is fz_run_block on the converted input, an int16 output
is the rule applied to that float32 output.

The oracle of the float32 output is oracle/flowz_oracle.py, called as tests/test_gpu_parity.py calls it -- except for div_sqrt_exp:
that oracle has no graph functions, and the function graphs' reference in this suite is tests/fn_ref.py: run_ir (the IR evaluated in
numpy with the restated sqrt / exp), which also gives the state after the block for every graph."""
import functools

import numpy as np
import pytest

import fn_ref
import grad_graphs as GG
import graphs as G
import pcm16_ref as R
from oracle import flowz_oracle as O

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

F32 = np.float32
T = 67                                            # several chunks plus a ragged last one at any chunk length <= 32
STREAMS = (1, 2, 63, 64, 65, 130, 257, 1001)      # on / off the dword grid, below and across a wave and a workgroup, even but no multiple of 4
GRAPHS = ("integrator", "df1_cascade6", "par4_sum", "cross_wire", "df1_cascade_params6", "div_sqrt_exp")


@pytest.fixture(scope="module")
def F():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    torch.cuda.set_device(0)
    from zignal_amd import flowz
    return flowz


_progs = {}


def prog(F, name, sexpr=None):
    if name not in _progs:
        _progs[name] = F.compile(F.from_sexpr(sexpr if sexpr is not None else GG.SUPPORTED[name]()))
    return _progs[name]


def dev(a):
    return torch.from_numpy(np.array(a)).cuda() if a is not None else None     # (a copy: the shared references are read-only)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.uint32), b.view(np.uint32)))


def pcm_input(seed, T_, ns, wires):
    """int16 over the full range, with -32768, 32767 and 0 in every stream"""
    q = np.random.default_rng(seed).integers(-32768, 32768, (T_, ns, wires), dtype=np.int16)
    q[0], q[1], q[2] = -32768, 32767, 0
    return q


def params_of(p, ns, seed):
    if not p.n_param:
        return None
    rng = np.random.default_rng(seed)
    par = np.empty((p.n_param, ns), F32)
    for j in range(p.n_param // 5):
        par[5 * j:5 * j + 5] = np.asarray(G.STABLE, F32)[:, None] * rng.uniform(0.9, 1.0, (5, ns)).astype(F32)
    return par


@functools.lru_cache(maxsize=None)
def reference(name, ns):
    """(q, params, the oracle's float32 output on the converted input, the state after it): computed once per case, never changed"""
    from zignal_amd import flowz
    p = prog(flowz, name)
    q = pcm_input(1000 + ns, T, ns, p.n_in)
    par = params_of(p, ns, 7 + ns)
    x = R.to_float(q)
    want, state = fn_ref.run_ir(p, x, params=par)
    if name != "div_sqrt_exp":
        y = O.compile(GG.SUPPORTED[name](), ns, params=par).run(x)
        assert same_bits(y, want), "the two references disagree"
    for a in (q, want, state):
        a.setflags(write=False)
    return q, par, want, state


# ---- parity on the graph list ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns", STREAMS)
@pytest.mark.parametrize("name", GRAPHS)
def test_parity_with_the_float_path_and_the_oracle(F, name, ns):
    p = prog(F, name)
    q, par, want, want_state = reference(name, ns)
    x = R.to_float(q)
    y32, st32 = p.run_block(dev(x), params=dev(par))
    y32, st32 = host(y32), host(st32)[:p.n_state]
    assert same_bits(y32, want), "fz_run_block on the converted input differs from the oracle"
    want16 = R.from_float(y32)
    # int16 in, float32 out: fz_run_block on the converted input, bit for bit
    yf, sf = p.run_block_pcm16(dev(q), params=dev(par), out_dtype=torch.float32)
    assert same_bits(host(yf), y32) and same_bits(host(yf), want)
    assert same_bits(host(sf)[:p.n_state], st32) and same_bits(st32, want_state[:p.n_state])
    # int16 in, int16 out: the rule applied to that float32 output
    yi, si = p.run_block_pcm16(dev(q), params=dev(par))
    assert yi.dtype == torch.int16 and np.array_equal(host(yi), want16)
    assert same_bits(host(si)[:p.n_state], st32)
    # float32 in, int16 out on the same floats: the same int16
    yo, so = p.run_block_pcm16(dev(x), params=dev(par), out_dtype=torch.int16)
    assert np.array_equal(host(yo), want16)
    assert same_bits(host(so)[:p.n_state], st32)


# ---- saturation, ties and special values through the kernel ------------------------------------------------------------------------
def gain(c):
    return G.mul(G.IN(1), G.lit(c))


@pytest.mark.parametrize("ns", (65, 130))
def test_ties_saturation_nan_and_inf_through_the_kernel(F, ns):
    rng = np.random.default_rng(5 + ns)
    odd = (rng.integers(-16384, 16384, (T, ns, 1)) * 2 + 1).astype(np.int16)
    full = pcm_input(9 + ns, T, ns, 1)
    q64 = full.astype(np.int64)
    cases = [
        # c = 0.5 on odd q: y * 32768 = q / 2, every sample a tie -> the even neighbour
        ("gain_half", gain(0.5), odd, (np.rint(odd.astype(np.float64) / 2)).astype(np.int16)),
        # c = 4: saturates on both sides
        ("gain_four", gain(4.0), full, np.clip(4 * q64, -32768, 32767).astype(np.int16)),
        # _1 / _1: q = 0 gives NaN and so 0, every other q gives 1.0 and so 32767
        ("self_ratio", ("div", G.IN(1), G.IN(1)), full, np.where(q64 == 0, 0, 32767).astype(np.int16)),
        # 1 / _1: q = 0 gives +inf and so 32767; |1 / x| >= 1 everywhere else
        ("reciprocal", ("div", G.lit(1.0), G.IN(1)), full, np.where(q64 >= 0, 32767, -32768).astype(np.int16)),
    ]
    for name, g, q, want in cases:
        p = prog(F, name, g)
        y32, _ = p.run_block(dev(R.to_float(q)))
        assert np.array_equal(R.from_float(host(y32)), want), name                # the rule in numpy agrees with the hand-written answer
        for x, odt in ((q, torch.int16), (R.to_float(q), torch.int16)):
            y, _ = p.run_block_pcm16(dev(x), out_dtype=odt)
            got = host(y)
            assert np.array_equal(got, want), (name, int((got != want).sum()))
        yf, _ = p.run_block_pcm16(dev(q), out_dtype=torch.float32)
        a, b = host(yf), host(y32)
        assert np.array_equal(np.isnan(a), np.isnan(b)) and same_bits(np.nan_to_num(a, nan=0.0), np.nan_to_num(b, nan=0.0)), name


# ---- rows outside the block are untouched --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns", (63, 1001))
@pytest.mark.parametrize("name", ("df1_cascade6", "cross_wire"))
def test_nothing_outside_the_block_is_written(F, name, ns):
    p = prog(F, name)
    q, par, want, want_state = reference(name, ns)
    n = T * ns * p.n_out
    pad = 64
    for odt, sentinel in ((torch.int16, 0x5A5A), (torch.float32, 12345.0)):
        # [64 sentinels][the block: T x ns x n_out][64 sentinels]: what the last lane's missing streams would hit lies right behind the block
        big = torch.full((pad + n + pad,), sentinel, dtype=odt, device="cuda")
        out = big[pad:pad + n].view(T, ns, p.n_out)
        # the state rows in a padded allocation too: [n_state x ns][64 sentinels]
        sbig = torch.full((p.n_state * ns + pad,), 777.0, dtype=torch.float32, device="cuda")
        sbig[:p.n_state * ns] = 0
        state = sbig[:p.n_state * ns].view(p.n_state, ns)
        assert out.data_ptr() % 16 == 0 and state.data_ptr() % 16 == 0
        y, st = p.run_block_pcm16(dev(q), state=state, out=out, out_dtype=odt)
        assert y.data_ptr() == out.data_ptr()
        b, s = host(big), host(sbig)
        assert (b[:pad] == sentinel).all() and (b[pad + n:] == sentinel).all(), "a sentinel next to out has changed"
        assert (s[p.n_state * ns:] == 777.0).all(), "a sentinel behind the state rows has changed"
        blk = b[pad:pad + n].reshape(T, ns, p.n_out)
        assert np.array_equal(blk, R.from_float(want)) if odt == torch.int16 else same_bits(blk, want)
        assert same_bits(s[:p.n_state * ns].reshape(p.n_state, ns), want_state[:p.n_state])


# ---- chaining -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns", (65, 130))
def test_float_blocks_and_pcm_blocks_chain_on_one_state(F, ns):
    p = prog(F, "df1_cascade6")
    q, _, want, want_state = reference("df1_cascade6", ns)
    x = R.to_float(q)
    want16 = R.from_float(want)
    # 33 rows through fz_run_block on the converted floats, then 34 rows through the PCM kernel, on one state buffer
    ya, st = p.run_block(dev(x[:33]))
    yb, st = p.run_block_pcm16(dev(q[33:]), state=st)
    assert same_bits(host(ya), want[:33]) and np.array_equal(host(yb), want16[33:])
    assert same_bits(host(st)[:p.n_state], want_state[:p.n_state])
    # the reverse order
    ya, st = p.run_block_pcm16(dev(q[:33]))
    yb, st = p.run_block(dev(x[33:]), state=st)
    assert np.array_equal(host(ya), want16[:33]) and same_bits(host(yb), want[33:])
    assert same_bits(host(st)[:p.n_state], want_state[:p.n_state])
    # int16 to int16 in place
    buf = dev(q)
    y, st = p.run_block_pcm16(buf, out=buf)
    assert y.data_ptr() == buf.data_ptr() and np.array_equal(host(buf), want16)
    assert same_bits(host(st)[:p.n_state], want_state[:p.n_state])


# ---- many streams, once ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns,T_", ((65600, 16), (1048577, 4)))
def test_many_streams_against_the_default_kernel(F, ns, T_):
    """the row descriptors and the 2-byte path (1 048 577 streams: rows off the dword grid) at real row lengths, every stream"""
    p = prog(F, "df1_cascade6")
    q = dev(pcm_input(ns, T_, ns, 1))
    x = (q.to(torch.float32) * (1.0 / 32768.0)).contiguous()                     # (exact: the conversion rule on the device)
    y32, st32 = p.run_block(x)
    r = y32 * 32768.0
    want = torch.where(torch.isnan(y32), torch.zeros_like(r), torch.clamp(torch.round(r), -32768.0, 32767.0)).to(torch.int16)
    y16, st16 = p.run_block_pcm16(q)
    torch.cuda.synchronize()
    assert torch.equal(y16, want)
    assert torch.equal(st16.view(torch.int32), st32.view(torch.int32))
    # (the device spelling of the rule above is the numpy one: a sample of it on the host)
    assert np.array_equal(host(want[:, :4096]), R.from_float(host(y32[:, :4096])))
    yf, _ = p.run_block_pcm16(q, out_dtype=torch.float32)
    torch.cuda.synchronize()
    assert torch.equal(yf.view(torch.int32), y32.view(torch.int32))


# ---- the host path ----------------------------------------------------------------------------------------------------------------------
# fz_bank.cpp: blocks of more than 2 x 32 MiB on their wider side are cut into time chunks of 32 MiB (whole multiples of 32 rows) that
# flow through the three-stream pipeline.  1001 streams of int16 are 2002 bytes a row: 16 736 rows a chunk, pipelined beyond 33 520 rows.
PIPELINED_ROWS = 2 * 16736 + 300


@pytest.mark.parametrize("T_", (300, PIPELINED_ROWS))
def test_host_path_equals_process_host_through_the_rule(F, T_):
    ns = 1001
    assert T_ == 300 or T_ * ns * 2 > 2 * (32 << 20)
    p = prog(F, "df1_cascade6")
    q = pcm_input(11 + T_, 2 * T_, ns, 1)
    x = R.to_float(q)
    a, b = p.bank(ns), p.bank(ns)
    # two calls in a row: the state carries from the first to the second
    for k in range(2):
        got = a.process_host_pcm16(q[k * T_:(k + 1) * T_])
        want = R.from_float(b.process_host(x[k * T_:(k + 1) * T_]))
        assert got.dtype == np.int16 and got.shape == (T_, ns, 1)
        assert np.array_equal(got, want), (k, int((got != want).sum()))


def test_host_path_takes_pinned_torch_tensors(F):
    ns, T_ = 257, 40
    p = prog(F, "cross_wire")
    q = pcm_input(21, T_, ns, p.n_in)
    want = R.from_float(p.bank(ns).process_host(R.to_float(q)))
    got = p.bank(ns).process_host_pcm16(torch.from_numpy(q).pin_memory())
    assert got.dtype == torch.int16 and np.array_equal(got.numpy(), want)


# ---- two launches give identical bits ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns", (257, 1048576))
def test_two_launches_give_identical_bits(F, ns):
    p = prog(F, "df1_cascade6")
    q = dev(pcm_input(31, 24, ns, 1))
    y1, s1 = p.run_block_pcm16(q)
    y2, s2 = p.run_block_pcm16(q)
    torch.cuda.synchronize()
    assert torch.equal(y1, y2) and torch.equal(s1.view(torch.int32), s2.view(torch.int32))
