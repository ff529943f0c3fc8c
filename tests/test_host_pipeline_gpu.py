"""The pipeline of fz_bank_process_host (time-major host frames) past its second chunk, at the shapes of tests/host_pipeline_graphs.py
(its docstring has the sums).  Output against the oracle, bit for bit; the int16 case against the oracle through the conversion rule of
tests/pcm16_ref.py.  That the chunks are really taken shows in the last test: a modulator array too short for the fourth chunk leaves the
rows of the first three in the caller's buffer."""
import functools

import numpy as np
import pytest

import host_pipeline_graphs as H
import pcm16_ref as R
from oracle import flowz_oracle as O

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

NS, T, CHUNK_BYTES, SEED = H.NS, H.T, H.CHUNK_BYTES, 4242
two_out, two_out_modulated = H.two_out, H.two_out_modulated


@pytest.fixture(scope="module")
def F():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    torch.cuda.set_device(0)
    from zignal_amd import flowz
    return flowz


def chunks(row_bytes):
    return len(H.launch_rows(row_bytes))


@functools.lru_cache(maxsize=None)
def reference(modulated):
    """(x, modulator rows or None, the oracle's output): computed once, never changed"""
    x = O.synth_input(SEED, np.arange(NS), T)
    mod = np.random.default_rng(SEED).uniform(-0.9, 0.9, (1, T)).astype(np.float32) if modulated else None
    want = O.compile(two_out_modulated(), NS).run(x, mod=mod) if modulated else O.compile(two_out(), NS).run(x)
    for a in (x, want):
        a.setflags(write=False)
    return x, mod, want


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.array_equal(a.view(np.uint32), b.view(np.uint32)))


def test_float32_frames(F, monkeypatch):
    assert chunks(NS * 2 * 4) == 5
    x, _, want = reference(False)
    p = F.compile(F.from_sexpr(two_out()))
    assert (p.n_in, p.n_out) == (1, 2) and p.n_state
    monkeypatch.setenv("FLOWZ_HIP_HOST_CHUNK_BYTES", str(CHUNK_BYTES))
    got = p.bank(NS).process_host(np.array(x))
    assert same_bits(got, want), int((got.view(np.uint32) != want.view(np.uint32)).sum())


def test_float64_output(F, monkeypatch):
    assert chunks(NS * 2 * 8) == 9
    x, _, want = reference(False)
    p = F.compile(F.from_sexpr(two_out()))
    monkeypatch.setenv("FLOWZ_HIP_HOST_CHUNK_BYTES", str(CHUNK_BYTES))
    got = p.bank(NS).process_host(np.array(x), out_f64=True)
    assert got.dtype == np.float64 and np.array_equal(got, want.astype(np.float64))


def test_pcm16_frames(F, monkeypatch):
    assert chunks(NS * 2 * 2) == 3
    p = F.compile(F.from_sexpr(two_out()))
    assert p.pcm16_supported()
    q = np.random.default_rng(SEED + 1).integers(-32768, 32768, (T, NS, 1), dtype=np.int16)
    q[0], q[1], q[2] = -32768, 32767, 0
    want = R.from_float(O.compile(two_out(), NS).run(R.to_float(q)))
    monkeypatch.setenv("FLOWZ_HIP_HOST_CHUNK_BYTES", str(CHUNK_BYTES))
    got = p.bank(NS).process_host_pcm16(q)
    assert got.dtype == np.int16 and got.shape == (T, NS, 2)
    assert np.array_equal(got, want), int((got != want).sum())


def test_modulator_rows_follow_the_chunks(F, monkeypatch):
    """every chunk is launched on a buffer of its own: t0 must still reach the launch, or the modulator rows start over at 0"""
    assert chunks(NS * 2 * 4) == 5
    x, mod, want = reference(True)
    p = F.compile(F.from_sexpr(two_out_modulated()))
    assert (p.n_in, p.n_out, p.n_mod) == (1, 2, 1)
    md = torch.from_numpy(mod).cuda()
    p.set_modulation(md)
    monkeypatch.setenv("FLOWZ_HIP_HOST_CHUNK_BYTES", str(CHUNK_BYTES))
    got = p.bank(NS).process_host(np.array(x))
    assert same_bits(got, want), int((got.view(np.uint32) != want.view(np.uint32)).sum())
    # The chunks are launches of their own.  An array 8 rows short is refused by the chunk that would overrun it, the fourth (rows 120
    # to 159 need 160 rows): the three before it have run and their rows are in the caller's buffer, the rest of it is untouched.  (One
    # round trip over the whole block would be refused before anything is written.)
    short = md[:, :T - 8].contiguous()
    p.set_modulation(short)
    out = np.full((T, NS, 2), np.float32(-7.0))
    with pytest.raises(F.FlowzError):
        p.bank(NS).process_host(np.array(x), out=out)
    done = 3 * H.chunk_rows(NS * 2 * 4)
    assert done == 120 and same_bits(out[:done], want[:done])
    assert bool((out[done:] == np.float32(-7.0)).all())
