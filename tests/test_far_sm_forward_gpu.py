"""fz_run_block_far_stream_major on the MI355X: the forward of graphs with delay lines deeper than 256 samples (rings in HBM) on
[batch, time] buffers as they lie.  Every comparison is bit for bit, NaNs of any payload equal: `out` against oracle.flowz_oracle and
against Program.run_block on the transposed frames, the state against run_block's row for row -- register rows, LDS-ring rows, far
slots and phase rows -- from a phase p0 = D - 3 that makes the rings wrap inside the first groups; around every boundary the kernel
has (wave, workgroup, group, patch, the depth of the line); windows of larger buffers between sentinels, two chained windows in turn
with the time-major kernel, untouched inputs, repeatability, the Python front door, autograd.run_far(stream_major=True) without a
transposition, and the random graphs with deep delays.  Shapes, draws and the oracle's answers are tests/far_sm_forward.py's."""
import numpy as np
import pytest

import far_sm_forward as FF
from grad_harness import dev, from_sm, gpu_flowz, to_sm, up4
from test_graph_functions_gpu import ndiff

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
SENTINEL = np.float32(-1234.5)


@pytest.fixture(scope="module")
def F():
    return gpu_flowz()


def host(t):
    return t.detach().cpu().numpy()


def stream_major(p, x, s0, par, rows=None, row0=0, out=None):
    """one call on the time-major draw x laid out stream-major in buffers of `rows` rows with the block at [row0, row0 + T): the
    window's output time-major, the state, the whole output buffer and the input buffer (host and device)"""
    T = x.shape[0]
    xs = to_sm(x, rows, row0, fill=7.0)
    xd = dev(xs)
    od = dev(np.full(xs.shape[:2] + (p.n_out,), SENTINEL, np.float32)) if out is None else out
    y, st = p.run_block_far_stream_major(xd, dev(s0), dev(par), out=od, row0=row0, n_samples=T)
    assert y is od
    return from_sm(host(y), T, row0), host(st), host(y), (xs, host(xd))


def time_major(p, x, s0, par):
    y, st = p.run_block(dev(x), dev(s0), dev(par))
    return host(y), host(st)


def same(got, want, what):
    assert ndiff(np.asarray(got, np.float32), np.asarray(want, np.float32)) == 0, what


def parity(name, ns, T, oracle=False):
    """one shape from a random state at phase D - 3: out and every state row are the time-major kernel's; oracle: and from a state of
    zero slots at that phase the output is the oracle's"""
    p = FF.prog(name)
    what = f"{name} ns={ns} T={T} {FF.geometry(p)}"
    x, s0, par = FF.draw(name, ns, T)
    y, st, ybuf, (xs, xs_after) = stream_major(p, x, s0, par)
    yt, stt = time_major(p, x, s0, par)
    same(y, yt, what + ": out against run_block")
    same(st, stt, what + ": state against run_block")
    for _, d, pr in FF.FG.far_rows(p):
        assert np.all(st[pr] == np.float32((FF.DEEPEST[name] - 3 + T) % d)), what + ": phase row"
    assert np.all(ybuf[:, T:] == SENTINEL), what + ": rows of out behind the window were written"
    assert np.array_equal(xs.view(np.uint32), xs_after.view(np.uint32)), what + ": the input was written"
    if oracle:
        x, z0, par = FF.draw(name, ns, T, zero=True)
        y0, _, _, _ = stream_major(p, x, z0, par)
        same(y0, FF.oracle(name, ns, T), what + ": out against the oracle")
        same(time_major(p, x, z0, par)[0], FF.oracle(name, ns, T), what + ": run_block against the oracle")


@pytest.mark.parametrize("name", sorted(FF.GRAPHS))
def test_stream_counts_around_a_wave_and_a_workgroup(F, name):
    for ns in FF.streams_of(name):
        parity(name, ns, FF.DEEPEST[name] + 1, oracle=ns in (1, 65))


@pytest.mark.parametrize("name", sorted(FF.GRAPHS))
def test_row_counts_around_the_group_the_patch_and_the_depth(F, name):
    G, R, _ = FF.geometry(FF.prog(name))
    D = FF.DEEPEST[name]
    rows = FF.rows_of(name)
    assert {G, R, D}.issubset(rows) and (name == "far1031" or 2 * D + 3 in rows)
    for T in rows:
        parity(name, 65, T, oracle=T == rows[-1])


@pytest.mark.parametrize("name", sorted(FF.GRAPHS))
def test_a_window_of_a_larger_buffer_between_sentinels(F, name):
    p = FF.prog(name)
    ns, T, row0 = 65, FF.DEEPEST[name] + 1, 8
    rows = up4(row0 + T) + 8
    x, s0, par = FF.draw(name, ns, T)
    y, st, ybuf, (xs, xs_after) = stream_major(p, x, s0, par, rows, row0)
    yt, stt = time_major(p, x, s0, par)
    same(y, yt, name + ": window out")
    same(st, stt, name + ": window state")
    assert np.all(ybuf[:, :row0] == SENTINEL) and np.all(ybuf[:, row0 + T:] == SENTINEL), name + ": rows of out outside the window were written"
    assert np.array_equal(xs.view(np.uint32), xs_after.view(np.uint32)), name


@pytest.mark.parametrize("name", sorted(FF.GRAPHS))
def test_two_chained_windows_in_turn_with_the_time_major_kernel(F, name):
    """up4(D - 2) rows, then D + 5, the state handed on: this kernel then run_block, run_block then this kernel, and this kernel
    twice give one block's output and state"""
    p = FF.prog(name)
    a, b = FF.chain_rows(name)
    ns, T = 65, a + b
    rows = up4(T)                                                   # (one buffer holds both windows)
    x, s0, par = FF.draw(name, ns, T)
    whole, st_whole = time_major(p, x, s0, par)
    for first_sm, second_sm in ((True, False), (False, True), (True, True)):
        if first_sm:
            ya, st, _, _ = stream_major(p, x[:a], s0, par, rows=rows, row0=0)
        else:
            ya, st = time_major(p, np.ascontiguousarray(x[:a]), s0, par)
        if second_sm:                                               # (the second window of a buffer that holds both: row0 = a)
            buf = np.concatenate([np.zeros_like(x[:a]), x[a:]])
            xd = dev(to_sm(buf, rows, 0))
            od = dev(np.full((ns, rows, p.n_out), SENTINEL, np.float32))
            y, st2 = p.run_block_far_stream_major(xd, dev(st), dev(par), out=od, row0=a, n_samples=b)
            assert np.all(host(y)[:, :a] == SENTINEL) and np.all(host(y)[:, T:] == SENTINEL)
            yb, st2 = from_sm(host(y), b, a), host(st2)
        else:
            yb, st2 = time_major(p, np.ascontiguousarray(x[a:]), st, par)
        what = f"{name} chained sm={first_sm},{second_sm}"
        same(np.concatenate([ya, yb]), whole, what + ": out")
        same(st2, st_whole, what + ": state")


def test_two_launches_are_identical_and_a_missing_state_is_zero(F):
    for name in ("far_comb", "far_mixed", "two_out"):
        p = FF.prog(name)
        ns, T = 130, FF.DEEPEST[name] + 37
        x, _, par = FF.draw(name, ns, T, zero=True)
        xd, pd = dev(to_sm(x, up4(T))), dev(par)
        y1, s1 = p.run_block_far_stream_major(xd, None, pd, n_samples=T)
        y2, s2 = p.run_block_far_stream_major(xd, None, pd, n_samples=T)
        y3, s3 = p.run_block_far_stream_major(xd, torch.zeros((p.n_state, ns), dtype=torch.float32, device="cuda"), pd, n_samples=T)
        assert y1 is not y2 and tuple(s1.shape) == (p.n_state, ns)
        same(host(y1), host(y2), name + ": repeat")
        same(host(s1), host(s2), name + ": repeat state")
        same(host(y1), host(y3), name + ": state=None")
        same(host(s1), host(s3), name + ": state=None state")
        assert np.all(host(y1)[:, T:] == 0)                         # (out allocated zeroed: rows behind the block)
        same(from_sm(host(y1), T), FF.oracle(name, ns, T), name + ": oracle")


def test_the_python_call_takes_batch_time_for_one_wire(F):
    name, ns, T = FF.PYTHON_CALL
    p = FF.prog(name)
    x, s0, par = FF.draw(name, ns, T)
    x2 = dev(np.ascontiguousarray(x[:, :, 0].T))                    # [n_streams, rows]
    y, st = p.run_block_far_stream_major(x2, dev(s0))
    assert tuple(y.shape) == (ns, T, 1)
    yt, stt = time_major(p, x, s0, par)
    same(from_sm(host(y), T), yt, "2-D x")
    same(host(st), stt, "2-D x state")
    with pytest.raises(F.FlowzError, match="multiples of 4"):
        p.run_block_far_stream_major(dev(np.zeros((ns, T - 1), np.float32)))
    with pytest.raises(F.FlowzError, match="expected contiguous float32 frames"):
        p.run_block_far_stream_major(dev(np.zeros((ns, T, 2), np.float32)))
    # a graph without a far line: run_block_stream_major's bits
    q = F.compile(F.from_sexpr(FF.DC.sexpr(*FF.NO_FAR)))
    xq = dev(to_sm(x, T))
    ya, sa = q.run_block_far_stream_major(xq)
    yb, sb = q.run_block_stream_major(xq)
    same(host(ya), host(yb), "no far line")
    same(host(sa), host(sb), "no far line state")


def test_autograd_run_far_stream_major_runs_the_forward_without_a_transposition(F, monkeypatch):
    from zignal_amd import autograd as AG
    name, ns, T = FF.AUTOGRAD
    p = FF.prog(name)
    x, s0, _ = FF.draw(name, ns, T)

    def spy(*a, **k):
        raise AssertionError("run_far(stream_major=True) transposed its input")
    # (wherever a transposition could come from: the names this module once imported, and the functions themselves)
    for mod in (AG, F):
        monkeypatch.setattr(mod, "frames_from_stream_major", spy, raising=False)
        monkeypatch.setattr(mod, "frames_to_stream_major", spy, raising=False)
    ys, ss = AG.run_far(p, dev(to_sm(x, T)), dev(s0), stream_major=True)
    yt, st = AG.run_far(p, dev(x), dev(s0))
    assert tuple(ys.shape) == (ns, T, p.n_out)
    same(from_sm(host(ys), T), host(yt), "autograd y")
    same(host(ss), host(st), "autograd state")


def test_random_graphs_with_deep_delays_match_the_oracle(F):
    from oracle import flowz_oracle as O
    ns, T = FF.RANDOM_SHAPE
    n = 0
    for seed, g, n_in, n_out in FF.random_graphs():
        p = F.compile(F.from_sexpr(g))
        x = O.synth_input(seed, np.arange(ns), T, n_wires=n_in)
        want = O.compile(g, ns).run(x)
        y, _ = p.run_block_far_stream_major(dev(to_sm(x, T)))
        same(from_sm(host(y), T), want, f"seed {seed}: {g}")
        n += 1
    assert n == FF.RANDOM_KEPT >= 8
