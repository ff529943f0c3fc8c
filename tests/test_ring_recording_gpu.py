"""The backward of a whole recording with deep delay lines on the MI355X (fz_run_recording_ring_grad, fz_run_recording_ring_loss_grad):
every output bit for bit against the one-launch ring call over the same rows and against tests/recording_ref.py, the block-start
states (read back from the head of the workspace) and state_out against the restatement's, state_out against run_block's state; at
blocks far shorter than the deepest line, a recording shorter than it, B just below and above it and the default B, at the stream counts
around a wave and a workgroup; a missing state gradient, the state gradient overwritten in place, every output left out in turn,
accumulators that are added to, and autograd.mse_recording_rings.

Every launch of launch() goes through the C ABI with a workspace of exactly the queried bytes and every output inside a larger buffer of
sentinels, and checks afterwards that the sentinels and the inputs kept their bits."""
import numpy as np
import pytest

import adjoint_ref as A
import grad_harness as H
import ring_loss_graphs as RL
import ring_recording_graphs as R
from grad_harness import OUT, dev, gpu_flowz, make_inputs, same

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

K = R.K
KEYS = H.LOSS_KEYS
NAMES = sorted(R.GRAPHS)


@pytest.fixture(scope="module")
def F():
    return gpu_flowz()


def present(p, loss):
    rows = {"x": p.n_in, "state": p.n_state, "params": p.n_param, "consts": p.n_const}
    return {key for key in (KEYS if loss else KEYS[:4]) if rows.get(key, 1)}


def launch(p, d, B, loss, checkpoint_rows=0, state_grad=True, alias=False, leave_out=()):
    """one call of fz_run_recording_ring_grad / fz_run_recording_ring_loss_grad through grad_harness.launch on the draw d in blocks of B rows
    (0: the library's choice)"""
    x, s0, par, yb, tg, sb, ap, ac, al = d
    return H.launch(p, (x, s0, par, tg if loss else yb, sb, ap, ac, al), ring=True, loss=loss, recording=B, c=checkpoint_rows,
                    state_grad=state_grad, alias=alias, leave_out=leave_out, k=K)


def check(p, got, want, what, keys=KEYS + ("state_out", "starts")):
    H.check(p, got, want, what, keys)


def one_launch(p, d, loss, c=0, state_grad=True):
    """the one-launch ring call of the library over the same rows"""
    x, s0, par, yb, tg, sb, ap, ac, al = d
    accum = {key: dev(v) for key, v, n in (("params", ap, p.n_param), ("consts", ac, p.n_const)) if n}
    sg = dev(sb) if state_grad else None
    if loss:
        r = p.run_block_ring_loss_grad(dev(x), dev(tg), dev(s0), dev(par), sg, grad_scale=K, accum=dict(accum, loss=dev(al)), checkpoint_rows=c)
    else:
        r = p.run_block_ring_grad(dev(x), dev(yb), dev(s0), dev(par), sg, accum=accum, checkpoint_rows=c)
    torch.cuda.synchronize()
    return {key: v.cpu().numpy() for key, v in r.items()}


@pytest.mark.parametrize("loss", [False, True], ids=["plain", "loss"])
@pytest.mark.parametrize("name", NAMES)
def test_every_bit_is_the_one_launch_calls_and_the_restatements(F, name, loss):
    p = R.prog(name)
    for (ns, T, B), c in [(t, 0) for t in R.triples(name)] + [(R.below_depth(name), 1)]:
        d = R.case(name, ns, T)
        what = f"{name} {'loss' if loss else 'plain'} ns={ns} T={T} B={B} C={c or 'default'}"
        got = launch(p, d, B, loss, checkpoint_rows=c)
        assert set(got) == present(p, loss) | {"state_out", "starts"}
        check(p, got, R.want(name, ns, T, B, loss, c), what + " against the restatement")
        check(p, got, one_launch(p, d, loss, c), what + " against the one-launch call", keys=KEYS)


@pytest.mark.parametrize("name", NAMES)
def test_state_out_is_run_blocks_state(F, name):
    p = R.prog(name)
    (ns, T), = R.forward_shapes(name)
    x, s0, par = R.case(name, ns, T)[:3]
    _, s_T = p.run_block(dev(x), dev(s0), dev(par))
    for loss in (False, True):
        got = launch(p, R.case(name, ns, T), 4, loss)
        assert same(got["state_out"][:p.n_state], s_T.cpu().numpy()[:p.n_state]), f"{name}: state_out is not run_block's state"


@pytest.mark.parametrize("name", NAMES)
def test_without_a_state_gradient_and_with_state0_grad_in_place(F, name):
    p = R.prog(name)
    ns, T, B = R.below_depth(name)
    d = R.case(name, ns, T)
    for loss in (False, True):
        want = R.chained(p, d, B, loss, state_grad=False)
        check(p, launch(p, d, B, loss, state_grad=False), want, f"{name} no state_grad")
        check(p, one_launch(p, d, loss, state_grad=False), want, f"{name} no state_grad, one launch", keys=KEYS)
        got = launch(p, d, B, loss, alias=True)
        assert "state" in got
        check(p, got, R.want(name, ns, T, B, loss), f"{name} in place")


@pytest.mark.parametrize("name", NAMES)
def test_each_output_left_out_in_turn(F, name):
    """with several blocks every output but state0_grad (the blocks chain through it); with one block state0_grad too, and all at once"""
    p = R.prog(name)
    ns, T, B = R.below_depth(name)
    d = R.case(name, ns, T)
    for loss in (False, True):
        want, keys = R.want(name, ns, T, B, loss), present(p, loss)
        for key in sorted(keys - {"state"}) + ["state_out"]:
            got = launch(p, d, B, loss, leave_out=(OUT.get(key, key),))
            assert set(got) == (keys | {"state_out", "starts"}) - {key}
            check(p, got, want, f"{name} without {key}")
        one = R.want(name, ns, T, 4 * T, loss)
        got = launch(p, d, 4 * T, loss, leave_out=("state0_grad",))
        assert set(got) == (keys | {"state_out", "starts"}) - {"state"}
        check(p, got, one, f"{name} one block without state0_grad")
        got = launch(p, d, 4 * T, loss, leave_out=tuple(OUT.values()) + ("state_out",))
        assert set(got) == {"starts"} and same(got["starts"], one["starts"])


@pytest.mark.parametrize("name", NAMES)
def test_the_accumulators_are_added_to(F, name):
    """the same recording from zero accumulators and from the pre-filled ones of every other test: both the restatement's bits, and they
    differ wherever the graph has such an accumulator"""
    p = R.prog(name)
    ns, T, B = R.below_depth(name)
    d = R.case(name, ns, T)
    x, s0, par, yb, tg, sb, ap, ac, al = d
    zero = (x, s0, par, yb, tg, sb, np.zeros_like(ap), np.zeros_like(ac), np.zeros_like(al))
    for loss in (False, True):
        want, want0 = R.want(name, ns, T, B, loss), R.chained(p, d, B, loss, zero_accum=True)
        check(p, launch(p, zero, B, loss), want0, f"{name} from zero")
        for key, n in (("params", p.n_param), ("consts", p.n_const), ("loss", int(loss))):
            assert not n or not same(want0[key], want[key]), key


@pytest.mark.parametrize("name", NAMES)
def test_autograd_mse_recording_rings_matches_float64_autograd(F, name):
    """loss and the gradients of x, state, params and consts against float64 autograd of the mean squared error: the 1e-4 the ring host
    tests hold the restatements to.  An upstream scalar that is not 1 is applied in backward(); state_out is run_block's state."""
    from zignal_amd import autograd as AG
    p = R.prog(name)
    (ns, T), = R.forward_shapes(name)                             # (the shape whose forward kernel the manifest holds)
    x, s0, par, tg, _, _, _, _ = RL.draw(p, ns, T, 31)
    xt, st = dev(x).requires_grad_(), dev(s0).requires_grad_()
    pt = dev(par).requires_grad_() if p.n_param else None
    ct = torch.tensor(p.consts(), dtype=torch.float32).requires_grad_() if p.n_const else None
    before = st.detach().clone()
    loss, s_out = AG.mse_recording_rings(p, xt, dev(tg), st, pt, ct, block_rows=4)
    (loss * 3.0).backward()
    assert torch.equal(st.detach(), before) and not s_out.requires_grad    # the caller's state is not advanced
    _, s_T = p.run_block(dev(x), dev(s0), dev(par))
    assert same(s_out.cpu().numpy()[:p.n_state], s_T.cpu().numpy()[:p.n_state])
    mse, _, grads = RL.mse_float64(p, x, tg, s0, par)
    assert abs(loss.item() - mse) <= 1e-4 * mse, (loss.item(), mse)
    assert A.rel_err(xt.grad.cpu().numpy() / 3.0, grads["x"]) <= 1e-4
    assert A.rel_err(st.grad.cpu().numpy() / 3.0, grads["state"]) <= 1e-4
    if p.n_param:
        assert A.rel_err(pt.grad.cpu().numpy() / 3.0, grads["params"]) <= 1e-4
    if p.n_const:
        assert A.rel_err(ct.grad.numpy() / 3.0, grads["consts"].sum(1)) <= 1e-4
    with pytest.raises(F.FlowzError):
        AG.mse_recording(p, xt, dev(tg), st, pt, ct)


def test_run_recording_ring_loss_grad_returns_the_dict_of_the_one_launch_call(F):
    name = "two_out_fb"
    p = R.prog(name)
    ns, T, B = R.below_depth(name)
    d, want = R.case(name, ns, T), R.want(name, ns, T, B, True)
    x, s0, par, yb, tg, sb, ap, ac, al = d
    r = p.run_recording_ring_loss_grad(dev(x), dev(tg), dev(s0), dev(par), dev(sb), grad_scale=K, block_rows=B, want=KEYS + ("state_out",),
                                       accum={"params": dev(ap), "consts": dev(ac), "loss": dev(al)})
    torch.cuda.synchronize()
    assert set(r) == set(KEYS) | {"state_out"}
    check(p, {key: v.cpu().numpy() for key, v in r.items()}, want, "python call")
    r = p.run_recording_ring_grad(dev(x), dev(yb), dev(s0), dev(par), dev(sb), block_rows=B, want=("x",))
    assert set(r) == {"x"} and same(r["x"].cpu().numpy(), R.want(name, ns, T, B, False)["x"])
    with pytest.raises(F.FlowzError):
        p.run_recording_loss_grad(dev(x), dev(tg), dev(s0), dev(par), dev(sb))


def test_for_a_graph_without_a_ring_it_is_run_recording_loss_grad(F):
    import grad_graphs as GG
    name = "moog_ladder"
    p = F.compile(F.from_sexpr(GG.SUPPORTED[name]()))
    x, s0, par, tg, sb, ap, ac = make_inputs(p, name, 257, 37, 3)
    want = KEYS + ("state_out",)
    run = lambda fn: fn(dev(x), dev(tg), dev(s0), dev(par), dev(sb), grad_scale=K, block_rows=8, want=want, accum={"params": dev(ap), "consts": dev(ac)})   # noqa: E731
    ring, plain = run(p.run_recording_ring_loss_grad), run(p.run_recording_loss_grad)
    torch.cuda.synchronize()
    assert set(ring) == set(plain) == set(want)
    for key in ring:
        assert same(ring[key].cpu().numpy(), plain[key].cpu().numpy()), key
