"""The backward of a whole recording with deep delay lines on stream-major buffers on the MI355X
(fz_run_recording_ring_grad_stream_major, fz_run_recording_ring_loss_grad_stream_major): every output bit for bit against the
time-major ring recording on the transposed buffers, against the one-launch stream-major ring call over the same window and against
tests/recording_ref.py; the block-start states (read back from the head of the workspace) and state_out against the restatement's and
the time-major call's, state_out against run_block_stream_major's state; two windows per case (the whole buffer; four rows in, with
rows behind it), block starts on, before and after a patch boundary of the states kernel; a missing state gradient, the state gradient
overwritten in place, every output left out in turn, accumulators that are added to, two launches identical, and
autograd.mse_recording_rings(stream_major=True).

Every launch of ring_sm_recording.launch goes through the C ABI with a workspace of exactly the queried bytes and every output inside
a larger buffer of sentinels, and checks afterwards that the sentinels, the inputs and the rows outside the window kept their bits."""
import numpy as np
import pytest

import adjoint_ref as A
import grad_harness as H
import ring_loss_graphs as RL
import ring_recording_graphs as R
import ring_sm_recording as S
from grad_harness import OUT, dev, gpu_flowz, make_inputs, same, to_sm

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

K = S.K
KEYS = H.LOSS_KEYS
ALL = KEYS + ("state_out", "starts")
NAMES = sorted(S.GRAPHS)


@pytest.fixture(scope="module")
def F():
    return gpu_flowz()


def present(p, loss):
    rows = {"x": p.n_in, "state": p.n_state, "params": p.n_param, "consts": p.n_const}
    return {key for key in (KEYS if loss else KEYS[:4]) if rows.get(key, 1)}


def results(got):
    """what a launch computed, without the whole buffers"""
    return {k for k in got if not k.endswith("_buffer")}


def check(p, got, want, what, keys=ALL):
    H.check(p, got, want, what, keys)


def time_major(p, d, B, loss, c=0, state_grad=True):
    """fz_run_recording_ring_grad / _ring_loss_grad on the transposed buffers: the draw itself"""
    x, s0, par, yb, tg, sb, ap, ac, al = d
    return H.launch(p, (x, s0, par, tg if loss else yb, sb, ap, ac, al), ring=True, loss=loss, recording=B, c=c, state_grad=state_grad, k=K)


def one_launch(p, d, loss, window, c=0, state_grad=True):
    """fz_run_block_ring_grad_stream_major / _ring_loss_grad_stream_major over the same window"""
    x, s0, par, yb, tg, sb, ap, ac, al = d
    return H.launch(p, (x, s0, par, tg if loss else yb, sb, ap, ac, al), ring=True, loss=loss, window=window, c=c, state_grad=state_grad, k=K)


@pytest.mark.parametrize("loss", [False, True], ids=["plain", "loss"])
@pytest.mark.parametrize("name", NAMES)
def test_every_bit_is_the_time_major_recordings_the_one_launch_calls_and_the_restatements(F, name, loss):
    p = S.prog(name)
    for (ns, T, B), c in S.cases(name):
        d = R.case(name, ns, T)
        want, tm = R.want(name, ns, T, B, loss, c), time_major(p, d, B, loss, c)
        for window in S.windows(T):
            what = f"{name} {'loss' if loss else 'plain'} ns={ns} T={T} B={B} C={c or 'default'} window={window}"
            got = S.launch(p, d, B, loss, window, c)
            assert results(got) == present(p, loss) | {"state_out", "starts"}
            check(p, got, want, what + " against the restatement")
            check(p, got, tm, what + " against the time-major recording")
            check(p, got, one_launch(p, d, loss, window, c), what + " against the one-launch call", keys=KEYS)


@pytest.mark.parametrize("name", NAMES)
def test_state_out_is_run_block_stream_majors_state(F, name):
    p = S.prog(name)
    ns, T = S.forward_shape(name)
    d = R.case(name, ns, T)
    x, s0, par = d[:3]
    _, s_T = p.run_block_stream_major(dev(to_sm(x, T)), dev(s0), dev(par))
    for loss in (False, True):
        got = S.launch(p, d, 4, loss, (T, 0))
        assert same(got["state_out"][:p.n_state], s_T.cpu().numpy()[:p.n_state]), f"{name}: state_out is not run_block_stream_major's state"


@pytest.mark.parametrize("name", NAMES)
def test_without_a_state_gradient_and_with_state0_grad_in_place(F, name):
    p = S.prog(name)
    ns, T, B = R.below_depth(name)
    d, window = R.case(name, ns, T), S.windows(T)[1]
    for loss in (False, True):
        want = R.chained(p, d, B, loss, state_grad=False)
        check(p, S.launch(p, d, B, loss, window, state_grad=False), want, f"{name} no state_grad")
        check(p, time_major(p, d, B, loss, state_grad=False), want, f"{name} no state_grad, time-major")
        got = S.launch(p, d, B, loss, window, alias=True)
        assert "state" in got
        check(p, got, R.want(name, ns, T, B, loss), f"{name} in place")


@pytest.mark.parametrize("name", NAMES)
def test_each_output_left_out_in_turn(F, name):
    """with several blocks every output but state0_grad (the blocks chain through it); with one block state0_grad too, and all at once"""
    p = S.prog(name)
    ns, T, B = R.below_depth(name)
    d, window = R.case(name, ns, T), S.windows(T)[1]
    for loss in (False, True):
        want, keys = R.want(name, ns, T, B, loss), present(p, loss)
        for key in sorted(keys - {"state"}) + ["state_out"]:
            got = S.launch(p, d, B, loss, window, leave_out=(OUT.get(key, key),))
            assert results(got) == (keys | {"state_out", "starts"}) - {key}
            check(p, got, want, f"{name} without {key}")
        one = R.want(name, ns, T, 4 * T, loss)
        got = S.launch(p, d, 4 * T, loss, window, leave_out=("state0_grad",))
        assert results(got) == (keys | {"state_out", "starts"}) - {"state"}
        check(p, got, one, f"{name} one block without state0_grad")
        got = S.launch(p, d, 4 * T, loss, window, leave_out=tuple(OUT.values()) + ("state_out",))
        assert results(got) == {"starts"} and same(got["starts"], one["starts"])


@pytest.mark.parametrize("name", NAMES)
def test_the_accumulators_are_added_to_and_two_launches_are_identical(F, name):
    """the same recording from zero accumulators and from the pre-filled ones of every other test: both the restatement's bits, and they
    differ wherever the graph has such an accumulator; a second launch on fresh buffers gives every bit of the first, the buffers
    around the window included"""
    p = S.prog(name)
    ns, T, B = R.below_depth(name)
    d, window = R.case(name, ns, T), S.windows(T)[1]
    x, s0, par, yb, tg, sb, ap, ac, al = d
    zero = (x, s0, par, yb, tg, sb, np.zeros_like(ap), np.zeros_like(ac), np.zeros_like(al))
    for loss in (False, True):
        want, want0 = R.want(name, ns, T, B, loss), R.chained(p, d, B, loss, zero_accum=True)
        check(p, S.launch(p, zero, B, loss, window), want0, f"{name} from zero")
        for key, n in (("params", p.n_param), ("consts", p.n_const), ("loss", int(loss))):
            assert not n or not same(want0[key], want[key]), key
        first, second = S.launch(p, d, B, loss, window), S.launch(p, d, B, loss, window)
        assert set(first) == set(second)
        for key in first:
            assert same(first[key], second[key]), f"{name}: {key} differs between two launches"


@pytest.mark.parametrize("name", NAMES)
def test_autograd_mse_recording_rings_stream_major(F, name):
    """bit for bit its time-major self on the transposed tensors; and loss and the gradients of x, state, params and consts against
    float64 autograd of the mean squared error, within the 1e-4 its time-major twin is held to.  An upstream scalar that is not 1 is
    applied in backward(); state_out is run_block_stream_major's state."""
    from zignal_amd import autograd as AG
    p = S.prog(name)
    ns, T = S.forward_shape(name)
    x, s0, par, tg, _, _, _, _ = RL.draw(p, ns, T, 31)

    def run(stream_major):
        lay = (lambda a: dev(to_sm(a, T))) if stream_major else dev
        xt, st = lay(x).requires_grad_(), dev(s0).requires_grad_()
        pt = dev(par).requires_grad_() if p.n_param else None
        ct = torch.tensor(p.consts(), dtype=torch.float32).requires_grad_() if p.n_const else None
        before = st.detach().clone()
        loss, s_out = AG.mse_recording_rings(p, xt, lay(tg), st, pt, ct, block_rows=4, stream_major=stream_major)
        (loss * 3.0).backward()
        assert torch.equal(st.detach(), before) and not s_out.requires_grad    # the caller's state is not advanced
        gx = xt.grad.cpu().numpy()
        return dict(loss=loss.detach().cpu().numpy(), state_out=s_out.cpu().numpy(), x=H.from_sm(gx, T) if stream_major else gx,
                    state=st.grad.cpu().numpy(), params=pt.grad.cpu().numpy() if p.n_param else None, consts=ct.grad.numpy() if p.n_const else None)
    sm, tm = run(True), run(False)
    for key in sm:
        assert (sm[key] is None and tm[key] is None) or same(sm[key], tm[key]), f"{name}: {key} differs from the time-major call"
    _, s_T = p.run_block_stream_major(dev(to_sm(x, T)), dev(s0), dev(par))
    assert same(sm["state_out"][:p.n_state], s_T.cpu().numpy()[:p.n_state])
    mse, _, grads = RL.mse_float64(p, x, tg, s0, par)
    assert abs(float(sm["loss"]) - mse) <= 1e-4 * mse, (float(sm["loss"]), mse)
    assert A.rel_err(sm["x"] / 3.0, grads["x"]) <= 1e-4
    assert A.rel_err(sm["state"] / 3.0, grads["state"]) <= 1e-4
    if p.n_param:
        assert A.rel_err(sm["params"] / 3.0, grads["params"]) <= 1e-4
    if p.n_const:
        assert A.rel_err(sm["consts"] / 3.0, grads["consts"].sum(1)) <= 1e-4
    with pytest.raises(F.FlowzError):
        AG.mse_recording(p, dev(to_sm(x, T)), dev(to_sm(tg, T)), dev(s0), dev(par), stream_major=True)


def test_the_python_calls_return_the_dict_of_the_one_launch_call(F):
    name = "two_out_fb"
    p = S.prog(name)
    ns, T, B = R.below_depth(name)
    d, want = R.case(name, ns, T), R.want(name, ns, T, B, True)
    x, s0, par, yb, tg, sb, ap, ac, al = d
    rows, row0 = S.windows(T)[1]
    sm = lambda a: dev(to_sm(a, rows, row0, H.FILL))              # noqa: E731
    r = p.run_recording_ring_loss_grad_stream_major(sm(x), sm(tg), dev(s0), dev(par), dev(sb), grad_scale=K, block_rows=B, row0=row0, n_samples=T,
                                                    want=KEYS + ("state_out",), accum={"params": dev(ap), "consts": dev(ac), "loss": dev(al)})
    assert set(r) == set(KEYS) | {"state_out"}
    got = H.to_numpy(r, (row0, T))
    check(p, got, want, "python call", keys=KEYS + ("state_out",))
    keep = np.ones(rows, bool)
    keep[row0:row0 + T] = False
    assert not got["x_buffer"][:, keep].any() and not got["out_buffer"][:, keep].any()      # (new tensors: zero outside the window)
    r = p.run_recording_ring_grad_stream_major(sm(x), sm(yb), dev(s0), dev(par), dev(sb), block_rows=B, row0=row0, n_samples=T, want=("x",))
    assert set(r) == {"x"} and same(H.to_numpy(r, (row0, T))["x"], R.want(name, ns, T, B, False)["x"])
    with pytest.raises(F.FlowzError):
        p.run_recording_loss_grad(sm(x), sm(tg), dev(s0), dev(par), dev(sb), stream_major=True, row0=row0, n_samples=T)


def test_for_a_graph_without_a_ring_it_is_run_recording_loss_grad_stream_major(F):
    import grad_graphs as GG
    name = "moog_ladder"
    p = F.compile(F.from_sexpr(GG.SUPPORTED[name]()))
    x, s0, par, tg, sb, ap, ac = make_inputs(p, name, 257, 36, 3)
    want = KEYS + ("state_out",)
    args = lambda: (dev(to_sm(x, 36)), dev(to_sm(tg, 36)), dev(s0), dev(par), dev(sb))   # noqa: E731
    kw = lambda: dict(grad_scale=K, block_rows=8, want=want, accum={"params": dev(ap), "consts": dev(ac)})   # noqa: E731
    ring, plain = p.run_recording_ring_loss_grad_stream_major(*args(), **kw()), p.run_recording_loss_grad(*args(), stream_major=True, **kw())
    torch.cuda.synchronize()
    assert set(ring) == set(plain) == set(want)
    for key in ring:
        assert same(ring[key].cpu().numpy(), plain[key].cpu().numpy()), key
