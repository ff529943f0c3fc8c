"""The far recording calls on stream-major buffers on the MI355X (fz_run_recording_far_grad_for, fz_run_recording_far_loss_grad_for
with FZ_GRAD_STREAM_MAJOR: the backward of a whole recording whose graph has delay lines deeper than 256 samples, on a [batch, time]
tensor as it lies).  At every case of tests/far_sm_recording.py and both windows, for the plain and the loss call: every output bit for
bit against the time-major fz_run_recording_far_* on the transposed buffers, against the one-launch fz_run_block_far_*_stream_major
over the same window and against tests/far_recording_ref.py; `starts`, read back from the head of the workspace, and state_out against
run_block chained over the same blocks, the far lines' slots and phase rows included; no state gradient, the state gradient
overwritten in place, every output left out in turn on accumulators that are not zero, two launches identical, the Python keywords
and autograd.mse_recording_far(stream_major=True).

Every launch of far_sm_recording.launch goes through the C ABI with a workspace of exactly the queried bytes and every output inside
a larger buffer of sentinels; in_grad and out are whole [n_streams][rows_total][wire] buffers of which only the window may change.
Afterwards the sentinels, the inputs and the rows outside the window kept their bits.  The time-major side, the cases' inputs and
far_recording_ref's answers (computed once) are those of tests/test_far_recording_gpu.py."""
import numpy as np
import pytest

import adjoint_ref as A
import far_grad_graphs as FG
import far_grad_ref as FR
import far_sm_graphs as FS
import far_sm_recording as S
import grad_harness as H
import test_far_recording_gpu as TR
from grad_harness import OUT, dev, gpu_flowz, same, to_sm

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

K = S.K
KEYS, LOSS_KEYS = H.GRAD_KEYS, H.LOSS_KEYS
NAMES = S.NAMES


@pytest.fixture(scope="module")
def F():
    return gpu_flowz()


def prog(F, name):
    return TR.prog(F, name)


def keys_of(loss):
    return LOSS_KEYS if loss else KEYS


def present(p, loss):
    rows = {"x": p.n_in, "state": p.n_state, "params": p.n_param, "consts": p.n_const}
    return {key for key in keys_of(loss) if rows.get(key, 1)}


def results(got):
    """what a launch computed, without the whole buffers"""
    return {k for k in got if not k.endswith("_buffer")}


def check(p, got, want, what, keys):
    H.check(p, got, want, what, keys)


def one_launch(p, d, loss, window, c=0, state_grad=True, alias=False):
    """fz_run_block_far_grad_stream_major / fz_run_block_far_loss_grad_stream_major over the same window"""
    with FS.far_entry_points():
        return H.launch(FS.AsRingFamily(p), d, ring=True, loss=loss, window=window, c=c, state_grad=state_grad, alias=alias, k=K)


_forward = {}


def forward_starts(p, name, ns, T, Be, d):
    """run_block chained over the blocks (time-major: the state rows are the same in both layouts), once per shape"""
    key = (name, ns, T, Be)
    if key not in _forward:
        _forward[key] = TR.forward_starts(p, d, Be)
    return _forward[key]


@pytest.mark.parametrize("loss", [False, True], ids=["plain", "loss"])
@pytest.mark.parametrize("name", NAMES)
def test_every_bit_is_the_time_major_recordings_the_one_launch_calls_and_the_restatements(F, name, loss):
    p = prog(F, name)
    keys = keys_of(loss)
    assert S.geometry(p) == S.symbol_geometry(p.far_states_kernel_symbol(stream_major=True))
    for ns, T, B, c in S.cases(name):
        Be = S.block_rows(name, T, B, c)
        assert Be == p.far_recording_block_rows(T, B, c)
        d, want = TR.case(F, name, ns, T, Be, loss)
        assert all(d[1][pr, 0] == (S.DEEPEST[name] - 3) % dd for _, dd, pr in FG.far_rows(p))
        tm = TR.launch(p, d, loss, recording=B, c=c)
        fs, fo = forward_starts(p, name, ns, T, Be, d)
        for window in S.windows(T):
            what = f"{name} {'loss' if loss else 'plain'} ns={ns} T={T} B={B} C={c or 'default'} window={window}"
            got = S.launch(p, d, B, loss, window, c)
            assert results(got) == present(p, loss) | {"state_out", "starts"}, what
            check(p, got, want, what + " against far_recording_ref", keys + ("state_out",))
            assert same(got["starts"], want["starts"]), what + ": starts against far_recording_ref"
            check(p, got, tm, what + " against the time-major recording", keys + ("state_out",))
            assert same(got["starts"], tm["starts"]), what + ": starts against the time-major recording"
            check(p, got, one_launch(p, d, loss, window, c), what + " against the one-launch call", keys)
            assert same(got["starts"], fs), what + ": starts against run_block"
            assert same(got["state_out"], fo), what + ": state_out against run_block"
            for _, dd, pr in FG.far_rows(p):                        # the far lines' phase rows, as the forward writes them
                p0 = S.DEEPEST[name] - 3
                assert all(got["starts"][k, pr, 0] == (p0 + k * Be) % dd for k in range(len(fs))) and got["state_out"][pr, 0] == (p0 + T) % dd


def variation_case(name):
    """two blocks and a tail, the blocks shorter than the line; the window four rows in, with rows behind it"""
    ns, T, B, c = S.cases(name)[2]
    return ns, T, B, c, S.windows(T)[1]


@pytest.mark.parametrize("loss", [False, True], ids=["plain", "loss"])
@pytest.mark.parametrize("name", NAMES)
def test_variations_match_the_one_launch_call(F, name, loss):
    """no state gradient; state0_grad in place; every output left out in turn (state0_grad too: with more than one block the call asks
    for it, so that is refused, and with one block honoured); all on accumulators that are not zero; two launches identical"""
    p = prog(F, name)
    keys = keys_of(loss)
    ns, T, B, c, window = variation_case(name)
    what = f"{name} loss={loss} ns={ns} T={T} B={B} window={window}"
    d = S.inputs(name, ns, T, loss)
    assert (d[5].any() or not p.n_param) and (d[6].any() or not p.n_const) and (not loss or d[7].any())
    check(p, S.launch(p, d, B, loss, window, state_grad=False), one_launch(p, d, loss, window, state_grad=False), what + " no state_grad", keys)
    got = S.launch(p, d, B, loss, window, alias=True)
    assert "state" in got
    whole = one_launch(p, d, loss, window)
    check(p, got, whole, what + " in place", keys)
    for b in ("in_grad", "param_grad", "const_grad") + (("loss", "out") if loss else ()) + ("state_out",):
        got = S.launch(p, d, B, loss, window, leave_out=(b,))
        assert results(got) - {"starts", "state_out"} == {k for k in present(p, loss) if OUT[k] != b}, what
        assert ("state_out" in got) == (b != "state_out")
        check(p, got, whole, what + f" without {b}", keys)
    with pytest.raises(F.FlowzError) as ei:
        S.launch(p, d, B, loss, window, leave_out=("state0_grad",))
    assert "state0_grad is null" in str(ei.value)
    one = S.launch(p, d, 4 * T, loss, window, leave_out=("state0_grad",))                  # one block: no chain
    assert "state" not in one
    check(p, one, whole, what + " one block without state0_grad", keys)
    first, second = S.launch(p, d, B, loss, window), S.launch(p, d, B, loss, window)
    assert set(first) == set(second)
    for key in first:
        assert same(first[key], second[key]), f"{what}: {key} differs between two launches"
    # from zero accumulators the bits differ wherever the graph has such an accumulator
    zero = tuple(d[:5]) + tuple(np.zeros_like(a) for a in d[5:])
    got0 = S.launch(p, zero, B, loss, window)
    check(p, got0, one_launch(p, zero, loss, window), what + " from zero", keys)
    for key, n in (("params", p.n_param), ("consts", p.n_const), ("loss", int(loss))):
        assert not n or not same(got0[key], first[key]), key


def test_layout_zero_is_the_time_major_call(F):
    name = "far_mixed"
    p = prog(F, name)
    ns, T, B, c = S.cases(name)[2]
    for loss in (False, True):
        d = S.inputs(name, ns, T, loss)
        got, tm = S.launch(p, d, B, loss, time_major=True), TR.launch(p, d, loss, recording=B)
        assert set(got) == set(tm)
        for key in got:
            assert same(got[key], tm[key]), key


def test_the_python_keywords(F):
    """run_recording_far_grad / run_recording_far_loss_grad(stream_major=True, row0, n_samples, in_grad): the shapes, windows and result
    dicts of the stream-major ring recording calls"""
    name = "far_mixed"
    p = prog(F, name)
    ns, T, B, c, (rows, row0) = variation_case(name)
    Be = S.block_rows(name, T, B, c)
    sm = lambda a: dev(to_sm(a, rows, row0, H.FILL))              # noqa: E731
    full = lambda w: torch.full((ns, rows, w), float(H.SENTINEL), device="cuda")   # noqa: E731
    for loss in (False, True):
        keys = keys_of(loss)
        d, want = TR.case(F, name, ns, T, Be, loss)
        x, s0, par, yt, sb, ap, ac = d[:7]
        accum = {"params": dev(ap), "consts": dev(ac)}
        kw = dict(want=keys + ("state_out",), block_rows=B, stream_major=True, row0=row0, n_samples=T)
        if loss:
            r = p.run_recording_far_loss_grad(sm(x), sm(yt), dev(s0), dev(par), dev(sb), grad_scale=K, accum=dict(accum, loss=dev(d[7])), in_grad=full(p.n_in),
                                              out=full(p.n_out), **kw)
        else:
            r = p.run_recording_far_grad(sm(x), sm(yt), dev(s0), dev(par), dev(sb), accum=accum, in_grad=full(p.n_in), **kw)
        assert set(r) == set(keys) | {"state_out"}
        got = H.to_numpy(r, (row0, T))
        check(p, got, want, f"python call loss={loss}", keys + ("state_out",))
        assert H.outside_keeps_sentinel(got["x_buffer"], row0, T) and (not loss or H.outside_keeps_sentinel(got["out_buffer"], row0, T))
        # without in_grad: a new tensor, zero outside the window; a [batch, time] tensor as it lies would be 2-D for one wire
        fn = p.run_recording_far_loss_grad if loss else p.run_recording_far_grad
        r = fn(sm(x), sm(yt), dev(s0), dev(par), dev(sb), want=("x",), block_rows=B, stream_major=True, row0=row0, n_samples=T,
               **({"grad_scale": K} if loss else {}))
        g = H.to_numpy(r, (row0, T))
        keep = np.ones(rows, bool)
        keep[row0:row0 + T] = False
        assert set(r) == {"x"} and same(g["x"], want["x"]) and not g["x_buffer"][:, keep].any()
        # the time-major defaults take no window, and the families below keep refusing
        with pytest.raises(F.FlowzError):
            fn(dev(x), dev(yt), dev(s0), dev(par), dev(sb), block_rows=B, row0=4)
        for refused in ((p.run_recording_ring_loss_grad_stream_major, p.run_recording_loss_grad) if loss else (p.run_recording_ring_grad_stream_major, p.run_recording_grad)):
            with pytest.raises(F.FlowzError):
                refused(sm(x), sm(yt), dev(s0), dev(par), dev(sb), block_rows=B, row0=row0, n_samples=T, **({} if "ring" in refused.__name__ else {"stream_major": True}))


def t_sm(a):
    """time-major numpy [T][ns][w] -> a stream-major device tensor [ns][T][w]: the tensor is the window"""
    return dev(np.ascontiguousarray(a.transpose(1, 0, 2)))


def test_autograd_mse_recording_far_stream_major(F):
    """bit for bit its time-major self on the transposed tensors, state_out run_block's state; loss and the gradients of x, state and
    consts within 1e-4 of float64 autograd of adjoint_ref.torch_forward on far257, the tolerance its time-major twin is held to"""
    from zignal_amd import autograd as AG
    name, ns, T, B = S.AUTOGRAD
    p = prog(F, name)
    far = FG.far_rows(p)
    D = FG.DEEPEST[name]
    x, s0, par, yb, sb, _, _ = FG.inputs(p, ns, T, 31)
    ages = lambda a, ph: FR.convert(a, [ph], far)[:D]                   # noqa: E731  (the line rows, as adjoint_ref keeps them)

    def run(stream_major):
        lay = t_sm if stream_major else dev
        xt, st = lay(x).requires_grad_(), dev(s0).requires_grad_()
        ct = torch.tensor(p.consts(), dtype=torch.float32).requires_grad_()
        before = st.detach().clone()
        loss, s_out = AG.mse_recording_far(p, xt, lay(yb), st, None, ct, block_rows=B, stream_major=stream_major)
        loss.backward()
        assert torch.equal(st.detach(), before) and not s_out.requires_grad
        gx = xt.grad.cpu().numpy()
        assert tuple(gx.shape) == ((ns, T, p.n_in) if stream_major else (T, ns, p.n_in))
        return dict(loss=loss.detach().cpu().numpy(), state_out=s_out.cpu().numpy(), x=gx.transpose(1, 0, 2) if stream_major else gx,
                    state=st.grad.cpu().numpy(), consts=ct.grad.numpy())
    sm, tm = run(True), run(False)
    for key in sm:
        assert same(sm[key], tm[key]), f"{key} differs from the time-major call"
    _, s_plain = p.run_block(dev(x), dev(s0))
    assert same(sm["state_out"], s_plain.cpu().numpy())
    L = A.Layout(p)
    t64 = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=torch.float64, requires_grad=True)   # noqa: E731
    x64, s64, c64 = t64(x), t64(ages(s0, 0)), t64(np.repeat(L.consts.astype(np.float64)[:, None], ns, 1))
    y64, _ = A.torch_forward(L, x64, s64, torch.zeros((0, ns), dtype=torch.float64), c64)
    l64 = ((y64 - torch.tensor(np.asarray(yb, np.float64))) ** 2).mean()
    gx, gs, gc = torch.autograd.grad(l64, (x64, s64, c64))
    assert abs(float(sm["loss"]) - l64.item()) <= 1e-4 * abs(l64.item())
    assert A.rel_err(sm["x"], gx.numpy()) <= 1e-4
    assert A.rel_err(ages(sm["state"], 0), gs.numpy()) <= 1e-4 and not sm["state"][D:].any()
    assert A.rel_err(sm["consts"], gc.numpy().sum(1)) <= 1e-4
    # a [batch, time] tensor as it lies, and the ring family keeps refusing
    x2 = t_sm(x)[..., 0].contiguous().requires_grad_()
    l2, _ = AG.mse_recording_far(p, x2, t_sm(yb)[..., 0].contiguous(), dev(s0), block_rows=B, stream_major=True)
    l2.backward()
    assert tuple(x2.grad.shape) == (ns, T) and same(x2.grad.cpu().numpy().T[..., None], sm["x"]) and l2.item() == float(sm["loss"])
    with pytest.raises(F.FlowzError):
        AG.mse_recording_rings(p, t_sm(x), t_sm(yb), dev(s0), block_rows=B, stream_major=True)
