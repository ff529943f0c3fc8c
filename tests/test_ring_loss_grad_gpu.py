"""The ring adjoint kernel under a squared-error loss on the MI355X (fz_run_block_ring_loss_grad): in_grad, state0_grad, param_grad,
const_grad, loss and out bit for bit against tests/loss_grad_ref.py, at the row counts around each line's depth and the stream counts
around a wave and a workgroup, at the default checkpoint stride and at 1; against the library's own run_block and run_block_ring_grad;
a missing state gradient, the state gradient overwritten in place, every output left out in turn, accumulators that are added to, two
chained blocks of which the first is shorter than the line, non-finite targets, and autograd.mse_rings.

Every launch of launch() goes through the C ABI with a workspace of exactly the queried bytes and every output inside a larger buffer of
sentinels, and checks afterwards that the sentinels, the inputs and the target kept their bits."""
import numpy as np
import pytest

import adjoint_ref as A
import grad_harness as H
import ring_grad_graphs as RG
import ring_loss_graphs as RL
from grad_harness import F32, OUT, dev, gpu_flowz, make_inputs, same

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

K = RL.K
KEYS = H.LOSS_KEYS


@pytest.fixture(scope="module")
def F():
    return gpu_flowz()


def launch(p, d, checkpoint_rows=0, state_grad=True, alias=False, leave_out=(), k=K):
    """one call of fz_run_block_ring_loss_grad through grad_harness.launch"""
    return H.launch(p, d, ring=True, loss=True, c=checkpoint_rows, state_grad=state_grad, alias=alias, leave_out=leave_out, k=k)


def check(p, got, want, what, keys=KEYS):
    H.check(p, got, want, what, keys)


@pytest.mark.parametrize("c", [0, 1])
@pytest.mark.parametrize("name", sorted(RL.GRAPHS))
def test_ring_loss_adjoint_matches_the_restatement_bitwise(F, name, c):
    p = RL.prog(name)
    for ns, T in RL.shapes(name):
        d, want = RL.case(name, ns, T)
        got = launch(p, d, checkpoint_rows=c)
        assert set(got) == {key for key in KEYS if {"x": p.n_in, "state": p.n_state, "params": p.n_param, "consts": p.n_const}.get(key, 1)}
        check(p, got, want, f"{name} C={c or 'default'} ns={ns} T={T}")


@pytest.mark.parametrize("name", sorted(RL.GRAPHS))
def test_out_is_run_blocks_and_the_gradients_are_run_block_ring_grads(F, name):
    """against the library itself: y of run_block, and run_block_ring_grad given ybar = (y - target) * K formed in float32 on the host"""
    p = RL.prog(name)
    ns, T = 65, RL.DEEPEST[name] + 1
    d, _ = RL.case(name, ns, T)
    x, s0, par, tg, sb, ap, ac, al = d
    got = launch(p, d)
    y, _ = p.run_block(dev(x), dev(s0), dev(par))
    y = y.cpu().numpy()
    assert same(got["out"], y), f"{name}: out is not run_block's y"
    ybar = ((y - tg) * F32(K)).astype(F32)
    accum = {key: dev(v) for key, v, n in (("params", ap, p.n_param), ("consts", ac, p.n_const)) if n}
    r = p.run_block_ring_grad(dev(x), dev(ybar), dev(s0), dev(par), dev(sb), accum=accum)
    torch.cuda.synchronize()
    check(p, got, {key: v.cpu().numpy() for key, v in r.items()}, f"{name} against run_block_ring_grad", keys=("x", "state", "params", "consts"))


@pytest.mark.parametrize("name", sorted(RL.GRAPHS))
def test_without_a_state_gradient_the_rings_start_from_plus_zero(F, name):
    p = RL.prog(name)
    D = RL.DEEPEST[name]
    for T in (D - 1, D + 1):
        d, _ = RL.case(name, 65, T)
        check(p, launch(p, d, state_grad=False), RL.restate(p, d, state_grad=False), f"{name} T={T} no state_grad")


@pytest.mark.parametrize("name", sorted(RL.GRAPHS))
def test_state0_grad_may_overwrite_state_grad(F, name):
    p = RL.prog(name)
    for T in (RL.DEEPEST[name] - 1, RL.DEEPEST[name] + 1):
        d, want = RL.case(name, 65, T)
        got = launch(p, d, alias=True)
        assert "state" in got
        check(p, got, want, f"{name} T={T} in place")


@pytest.mark.parametrize("name", ["lds_ring_comb", "biquad_comb17", "two_in", "two_out_fb"])
def test_each_output_left_out_in_turn(F, name):
    p = RL.prog(name)
    d, want = RL.case(name, 65, RL.DEEPEST[name] + 1)
    present = {key for key in KEYS if {"x": p.n_in, "state": p.n_state, "params": p.n_param, "consts": p.n_const}.get(key, 1)}
    for key in KEYS:
        got = launch(p, d, leave_out=(OUT[key],))
        assert set(got) == present - {key}
        check(p, got, want, f"{name} without {OUT[key]}")
    assert launch(p, d, leave_out=tuple(OUT.values())) == {}


@pytest.mark.parametrize("name", ["biquad_comb17", "two_out_fb"])
def test_loss_param_grad_and_const_grad_are_added_to(F, name):
    """the same block from zero accumulators and from pre-filled ones: both the restatement's bits, and they differ"""
    p = RL.prog(name)
    d, want = RL.case(name, 65, RL.DEEPEST[name] + 1)
    x, s0, par, tg, sb, ap, ac, al = d
    check(p, launch(p, d), want, f"{name} pre-filled")
    zero = (x, s0, par, tg, sb, np.zeros_like(ap), np.zeros_like(ac), np.zeros_like(al))
    got0, want0 = launch(p, zero), RL.restate(p, zero)
    check(p, got0, want0, f"{name} from zero")
    assert not same(want0["loss"], want["loss"]) and not same(want0["params"], want["params"]) and not same(want0["consts"], want["consts"])


@pytest.mark.parametrize("name", sorted(RL.GRAPHS))
def test_two_blocks_chain_like_one(F, name):
    """D - 2 rows, then D + 5: the backward of block 2, then of block 1 on the same three accumulators (loss included) with block 2's
    state adjoint -- the state between the blocks is run_block's -- gives the bits of one call over both"""
    p = RL.prog(name)
    D = RL.DEEPEST[name]
    T1, T2 = D - 2, D + 5
    d, want = RL.case(name, 65, T1 + T2)
    x, s0, par, tg, sb, ap, ac, al = d
    whole = launch(p, d)
    check(p, whole, want, f"{name} one call")
    _, s_mid = p.run_block(dev(x[:T1]), dev(s0), dev(par))
    s_mid = s_mid.cpu().numpy()
    second = launch(p, (x[T1:], s_mid, par, tg[T1:], sb, ap, ac, al))
    first = launch(p, (x[:T1], s0, par, tg[:T1], second["state"], second.get("params", ap), second.get("consts", ac), second["loss"]))
    chained = dict(first, x=np.concatenate([first["x"], second["x"]]), out=np.concatenate([first["out"], second["out"]]))
    check(p, chained, whole, f"{name} chained")


@pytest.mark.parametrize("name", sorted(RL.GRAPHS))
def test_non_finite_targets_stay_in_their_streams(F, name):
    """+inf in the target of one stream and NaN in that of another: the other streams keep the bits of the finite case, the two are
    non-finite where the restatement is (NaN equals NaN, as tests/loss_grad_fuzz.py compares)"""
    p = RL.prog(name)
    ns, T = 65, RL.DEEPEST[name] + 1
    d, finite = RL.case(name, ns, T)
    x, s0, par, tg, sb, ap, ac, al = d
    bad = np.array(tg)
    bad[T // 2, 3, 0] = np.inf
    bad[T - 1, 40, p.n_out - 1] = np.nan
    d2 = (x, s0, par, bad, sb, ap, ac, al)
    want = RL.restate(p, d2)
    got = launch(p, d2)
    check(p, got, want, f"{name} non-finite targets")
    assert not np.isfinite(want["loss"][3]) and np.isnan(want["loss"][40])
    others = np.ones(ns, bool)
    others[[3, 40]] = False
    for key in got:
        axis = 0 if key == "loss" else 1
        assert same(np.compress(others, got[key], axis), np.compress(others, np.asarray(finite[key])[:got[key].shape[0]] if key in ("state", "params", "consts")
                                                                     else finite[key], axis)), key
        assert np.all(np.isfinite(np.compress(others, got[key], axis))), key


def test_run_block_ring_loss_grad_returns_the_dict_of_run_block_loss_grad(F):
    name = "two_out_fb"
    p = RL.prog(name)
    d, want = RL.case(name, 257, RL.DEEPEST[name] + 1)
    x, s0, par, tg, sb, ap, ac, al = d
    r = p.run_block_ring_loss_grad(dev(x), dev(tg), dev(s0), dev(par), dev(sb), grad_scale=K,
                                   accum={"params": dev(ap), "consts": dev(ac), "loss": dev(al)})
    torch.cuda.synchronize()
    assert set(r) == set(KEYS)
    check(p, {key: v.cpu().numpy() for key, v in r.items()}, want, "python call")
    r = p.run_block_ring_loss_grad(dev(x), dev(tg), dev(s0), dev(par), dev(sb), grad_scale=K, want=("loss",), accum={"loss": dev(al)})
    assert set(r) == {"loss"} and same(r["loss"].cpu().numpy(), want["loss"])
    with pytest.raises(F.FlowzError):
        p.run_block_loss_grad(dev(x), dev(tg), dev(s0), dev(par), dev(sb))


def test_for_a_graph_without_a_ring_it_is_run_block_loss_grad(F):
    import grad_graphs as GG
    name = "moog_ladder"
    p = F.compile(F.from_sexpr(GG.SUPPORTED[name]()))
    x, s0, par, tg, sb, ap, ac = make_inputs(p, name, 257, 37, 3)
    run = lambda fn: fn(dev(x), dev(tg), dev(s0), dev(par), dev(sb), grad_scale=K, accum={"params": dev(ap), "consts": dev(ac)})   # noqa: E731
    ring, plain = run(p.run_block_ring_loss_grad), run(p.run_block_loss_grad)
    torch.cuda.synchronize()
    assert set(ring) == set(plain) == set(KEYS)
    for key in ring:
        assert same(ring[key].cpu().numpy(), plain[key].cpu().numpy()), key


@pytest.mark.parametrize("name", ["lds_ring_comb", "two_out_fb"])
def test_autograd_mse_rings_matches_float64_autograd(F, name):
    """loss and the gradients of x, state, params and consts against float64 autograd of the mean squared error: the bound of
    test_ring_loss_grad_host.py.  An upstream scalar that is not 1 is applied in backward()."""
    from zignal_amd import autograd as AG
    p = RL.prog(name)
    ns, T = 130, 2 * RL.DEEPEST[name] + 3
    x, s0, par, tg, _, _, _, _ = RL.draw(p, ns, T, 31)
    xt, st = dev(x).requires_grad_(), dev(s0).requires_grad_()
    pt = dev(par).requires_grad_() if p.n_param else None
    ct = torch.tensor(p.consts(), dtype=torch.float32).requires_grad_()
    before = st.detach().clone()
    loss = AG.mse_rings(p, xt, dev(tg), st, pt, ct)
    (loss * 3.0).backward()
    assert torch.equal(st.detach(), before)                             # the caller's state is not advanced
    mse, _, grads = RL.mse_float64(p, x, tg, s0, par)
    assert abs(loss.item() - mse) <= 1e-4 * mse, (loss.item(), mse)
    assert A.rel_err(xt.grad.cpu().numpy() / 3.0, grads["x"]) <= 1e-4
    assert A.rel_err(st.grad.cpu().numpy() / 3.0, grads["state"]) <= 1e-4
    if p.n_param:
        assert A.rel_err(pt.grad.cpu().numpy() / 3.0, grads["params"]) <= 1e-4
    assert A.rel_err(ct.grad.numpy() / 3.0, grads["consts"].sum(1)) <= 1e-4
    with pytest.raises(F.FlowzError):
        AG.mse(p, xt, dev(tg), st, pt, ct)


def test_autograd_mse_rings_raises_for_rings_that_fit_no_workgroup(F):
    from zignal_amd import autograd as AG
    p = F.compile(F.from_sexpr(RG.six_lines_256()))
    x = torch.zeros((4, 8, 6), device="cuda")
    with pytest.raises(F.FlowzError) as ei:
        AG.mse_rings(p, x, torch.zeros((4, 8, 1), device="cuda"))
    assert "393216" in str(ei.value)
