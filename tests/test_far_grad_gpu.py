"""The far adjoint kernels on the MI355X (fz_run_block_far_grad, fz_run_block_far_loss_grad: graphs with delay lines deeper than 256
samples, whose rings live in HBM): every output bit for bit against tests/far_grad_ref.py, at the row counts around each line's depth
and the stream counts around a wave and a workgroup; a phase that makes the ring wrap inside the block; checkpoint strides (and with
them both paths of sweep 2); a missing state gradient, the state gradient overwritten in place, every output left out in turn; two
chained blocks of which the first is shorter than the line, through run_block's own state rows; the loss call; autograd over both.

Every launch goes through the C ABI with a workspace of exactly the queried bytes inside a larger buffer of sentinels, and checks
afterwards that the sentinels and every input kept their bits."""
import ctypes

import numpy as np
import pytest

import adjoint_ref as A
import far_grad_graphs as FG
import far_grad_ref as FR
import grad_harness as H
from grad_harness import F32, Guarded, dev, gpu_flowz, same

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

KEYS, LOSS_KEYS = H.GRAD_KEYS, H.LOSS_KEYS
K = H.K


@pytest.fixture(scope="module")
def F():
    return gpu_flowz()


_progs, _cases = {}, {}


def prog(F, name):
    if name not in _progs:
        _progs[name] = F.compile(F.from_sexpr(FG.FARS[name]()))
    return _progs[name]


def case(F, name, ns, T, p0=0, loss=False, state_grad=True):
    """the inputs of a case and far_grad_ref's answer to them, computed once and never modified.  loss: dL/dy is the target, and an
    eighth array is the loss accumulator"""
    key = (name, ns, T, p0, loss, state_grad)
    if key not in _cases:
        p = prog(F, name)
        d = FG.inputs(p, ns, T, 7 * ns + T + 1000 * p0, p0=p0)
        x, s0, par, yb, sb, ap, ac = d
        sg = sb if state_grad else None
        if loss:
            al = np.random.default_rng(ns + T).standard_normal(ns).astype(F32)
            d = d + (al,)
            want = FR.loss_grad(p, x, yb, K, s0, par, sg, ap, ac, al)
        else:
            want = FR.grad(p, x, yb, s0, par, sg, ap, ac)
        for a in (*d, *want.values()):
            if a is not None:
                a.setflags(write=False)
        _cases[key] = (d, want)
    return _cases[key]


def stride(p):
    return int(p.far_grad_kernel_symbol().split("_c")[1].split("b")[0])


def launch(p, d, loss=False, c=0, state_grad=True, alias=False, leave_out=()):
    """One call of fz_run_block_far_grad (loss: fz_run_block_far_loss_grad, grad_scale = K) through the C ABI on the time-major draw
    d = (x, s0, par, dL/dy or target, sb, ap, ac[, al]): dict of the outputs asked for (numpy) -- grad_harness.launch for the far family,
    which it does not know.  Afterwards: every input kept its bits (state_grad excepted when aliased); the workspace is exactly the
    queried bytes and its surroundings and those of every output kept their sentinels; an output that is left out, has zero rows or is
    aliased away was not written at all."""
    from zignal_amd import _capi as CA
    x, s0, par, yt, sb, ap, ac = d[:7]
    T, ns, _ = x.shape
    ins = {"in_": dev(x), "state": dev(s0), "params": dev(par), "target" if loss else "out_grad": dev(yt), "state_grad": dev(sb) if state_grad else None}
    before = {key: v.clone() for key, v in ins.items() if v is not None}
    n = {"in_grad": p.n_in, "state0_grad": p.n_state, "param_grad": p.n_param, "const_grad": p.n_const, "loss": 1, "out": p.n_out}
    outs = {"in_grad": Guarded((T, ns, max(p.n_in, 1))), "state0_grad": Guarded((max(p.n_state, 1), ns)),
            "param_grad": Guarded((max(p.n_param, 1), ns), ap if p.n_param else None),
            "const_grad": Guarded((max(p.n_const, 1), ns), ac if p.n_const else None)}
    if loss:
        outs.update(loss=Guarded((ns,), d[7]), out=Guarded((T, ns, max(p.n_out, 1))))
    wsb = p.far_grad_workspace_bytes(ns, T, c)
    assert wsb % 4 == 0
    ws = Guarded((wsb // 4,))
    a = CA.LossGradArgs() if loss else CA.GradArgs()
    a.struct_size, a.checkpoint_rows = ctypes.sizeof(a), c
    if loss:
        a.grad_scale = K
    for key, t in ins.items():
        setattr(a, key, t.data_ptr() if t is not None and t.numel() else None)
    for key, g in outs.items():
        setattr(a, key, g.mid.data_ptr() if n[key] and key not in leave_out else None)
    if alias:
        a.state0_grad = ins["state_grad"].data_ptr()
    a.workspace, a.workspace_bytes = ws.mid.data_ptr(), wsb
    fn = CA.lib.fz_run_block_far_loss_grad if loss else CA.lib.fz_run_block_far_grad
    CA.check(fn(p._h, ctypes.byref(a), ns, T, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    for key, t in before.items():
        if not (alias and key == "state_grad"):
            assert torch.equal(ins[key].view(torch.int32), t.view(torch.int32)), f"input {key} was written"
    assert ws.guards_kept(), "the workspace's surroundings were written"
    gone = {key for key in outs if key in leave_out or not n[key] or (alias and key == "state0_grad")}
    got = {}
    for key, b in H.OUT.items():
        if b not in outs:
            continue
        assert outs[b].guards_kept(), f"the surroundings of {b} were written"
        if b in gone:
            assert outs[b].untouched(), f"{b} was left out and written"
        else:
            got[key] = outs[b].mid.cpu().numpy()
    if alias and "state0_grad" not in leave_out:
        got["state"] = ins["state_grad"].cpu().numpy()
    return got


def check(p, got, want, what, keys=KEYS):
    has = {"x": p.n_in, "state": p.n_state, "params": p.n_param, "consts": p.n_const, "loss": 1, "out": p.n_out}
    assert set(got) >= {k for k in keys if has[k]}, f"{what}: {sorted(got)} lacks a result"      # (one that went missing does not pass unseen)
    H.check(p, got, want, what, keys)


def rows_of(name, C):
    D = FG.DEEPEST[name]
    return sorted(T for T in {1, D - 1, D, D + 1, C + 1, 2 * D + 3} if name != "far1031" or T <= FG.MAX_ROWS)


def shapes(p, name):
    D = FG.DEEPEST[name]
    return [(65, T) for T in rows_of(name, stride(p))] + [(ns, D + 1) for ns in ((1, 65) if name == "far1031" else (1, 64, 257))]


@pytest.mark.parametrize("name", sorted(FG.FARS))
def test_far_adjoint_matches_reference_bitwise(F, name):
    p = prog(F, name)
    for ns, T in shapes(p, name):
        inputs, want = case(F, name, ns, T)
        check(p, launch(p, inputs), want, f"{name} ns={ns} T={T}")


@pytest.mark.parametrize("name", sorted(FG.FARS))
def test_a_phase_that_wraps_the_ring_inside_the_block(F, name):
    """p0 = D - 3 at T = D + 1: the slots run over the end of the line's rows in the block's third row"""
    p = prog(F, name)
    D = FG.DEEPEST[name]
    inputs, want = case(F, name, 65, D + 1, p0=D - 3)
    assert all(inputs[1][pr, 0] == (D - 3) % d for _, d, pr in FG.far_rows(p))
    check(p, launch(p, inputs), want, f"{name} p0={D - 3}")


@pytest.mark.parametrize("name", FG.STRIDES)
@pytest.mark.parametrize("c", [1, 32])
def test_bits_do_not_depend_on_the_checkpoint_stride(F, name, c):
    """C = 1 takes the fast path on every graph, C = 32 the per-row path on far_tap1: the two paths are held to the same bits"""
    p = prog(F, name)
    D = FG.DEEPEST[name]
    for ns, T, p0 in ((65, D + 1, 0), (65, 2 * D + 3, 0), (65, D + 1, D - 3)):
        inputs, want = case(F, name, ns, T, p0=p0)
        check(p, launch(p, inputs, c=c), want, f"{name} C={c} ns={ns} T={T} p0={p0}")


@pytest.mark.parametrize("name", sorted(FG.FARS))
def test_without_a_state_gradient_the_rings_start_from_plus_zero(F, name):
    p = prog(F, name)
    D = FG.DEEPEST[name]
    for T in (D - 1, D + 1):
        inputs, want = case(F, name, 65, T, state_grad=False)
        check(p, launch(p, inputs, state_grad=False), want, f"{name} T={T} no state_grad")


@pytest.mark.parametrize("name", sorted(FG.FARS))
def test_state0_grad_may_overwrite_state_grad(F, name):
    p = prog(F, name)
    for T in (FG.DEEPEST[name] - 1, FG.DEEPEST[name] + 1):
        inputs, want = case(F, name, 65, T)
        check(p, launch(p, inputs, alias=True), want, f"{name} T={T} in place")


@pytest.mark.parametrize("name", ["far_comb", "far_mixed", "far_two_in"])
def test_each_output_left_out_in_turn(F, name):
    p = prog(F, name)
    inputs, want = case(F, name, 65, FG.DEEPEST[name] + 1)
    has = {"x": p.n_in, "state": p.n_state, "params": p.n_param, "consts": p.n_const}
    for b in ("in_grad", "state0_grad", "param_grad", "const_grad"):
        got = launch(p, inputs, leave_out=(b,))
        assert set(got) == {k for k in KEYS if H.OUT[k] != b and has[k]}
        H.check(p, got, want, f"{name} without {b}", KEYS)
    assert launch(p, inputs, leave_out=tuple(H.OUT.values())) == {}


@pytest.mark.parametrize("name", sorted(FG.FARS))
def test_two_blocks_chain_like_one(F, name):
    """D - 2 rows, then D + 5: the backward of block 2, then of block 1 on the same accumulators with block 2's state adjoint as it is
    -- the state between the blocks is run_block's, phase row included -- gives the bits of one call over both"""
    p = prog(F, name)
    D = FG.DEEPEST[name]
    T1, T2 = D - 2, D + 5
    if name == "far1031":                                         # (2 D + 3 rows are beyond the restatement's reach: one launch stands for it)
        x, s0, par, yb, sb, ap, ac = FG.inputs(p, 65, T1 + T2, 5)
    else:
        (x, s0, par, yb, sb, ap, ac), want = case(F, name, 65, T1 + T2)
    whole = launch(p, (x, s0, par, yb, sb, ap, ac))
    if name != "far1031":
        check(p, whole, want, f"{name} one call")
    _, s_mid = p.run_block(dev(x[:T1]), dev(s0), dev(par))
    s_mid = s_mid.cpu().numpy()
    assert all(s_mid[pr, 0] == T1 % d for _, d, pr in FG.far_rows(p))
    second = launch(p, (x[T1:], s_mid, par, yb[T1:], sb, ap, ac))
    first = launch(p, (x[:T1], s0, par, yb[:T1], second["state"], second.get("params", ap), second.get("consts", ac)))
    chained = dict(first, x=np.concatenate([first["x"], second["x"]]))
    check(p, chained, whole, f"{name} chained")


@pytest.mark.parametrize("name", sorted(FG.FARS))
def test_loss_call(F, name):
    """fz_run_block_far_loss_grad against loss_grad_ref at grad_harness.K, against the plain far call given the same dL/dy, and `out` /
    `loss` against run_block's bits"""
    p = prog(F, name)
    D = FG.DEEPEST[name]
    for T, p0 in ((D + 1, 0), (D + 1, D - 3), (stride(p) + 1, 0)):
        inputs, want = case(F, name, 65, T, p0=p0, loss=True)
        x, s0, par, tg, sb, ap, ac, al = inputs
        got = launch(p, inputs, loss=True)
        check(p, got, want, f"{name} loss T={T} p0={p0}", LOSS_KEYS)
        y, _ = p.run_block(dev(x), dev(s0), dev(par))
        y = y.cpu().numpy()
        assert same(got["out"], y)
        with np.errstate(all="ignore"):
            e, ls = y - tg, al.copy()
            for t in range(T - 1, -1, -1):
                for j in range(p.n_out):
                    ls = ls + e[t, :, j] * e[t, :, j]
        assert same(got["loss"], ls)
        plain = launch(p, (x, s0, par, e * F32(K), sb, ap, ac))
        check(p, got, plain, f"{name} loss against the plain call", KEYS)
    # `out` and `loss` left out: the gradients do not change
    got = launch(p, inputs, loss=True, leave_out=("loss", "out"))
    assert "loss" not in got and "out" not in got
    H.check(p, got, want, f"{name} loss without loss and out", KEYS)


def test_run_block_far_grad_returns_the_dict_of_run_block_grad(F):
    name = "far_mixed"
    p = prog(F, name)
    (x, s0, par, yb, sb, ap, ac), want = case(F, name, 257, FG.DEEPEST[name] + 1)
    r = p.run_block_far_grad(dev(x), dev(yb), dev(s0), dev(par), dev(sb), accum={"params": dev(ap), "consts": dev(ac)})
    torch.cuda.synchronize()
    assert set(r) == set(KEYS)
    check(p, {k: v.cpu().numpy() for k, v in r.items()}, want, "python call")
    (x, s0, par, tg, sb, ap, ac, al), lwant = case(F, name, 65, FG.DEEPEST[name] + 1, loss=True)
    r = p.run_block_far_loss_grad(dev(x), dev(tg), dev(s0), dev(par), dev(sb), grad_scale=K, accum={"params": dev(ap), "consts": dev(ac), "loss": dev(al)})
    torch.cuda.synchronize()
    assert set(r) == set(LOSS_KEYS)
    check(p, {k: v.cpu().numpy() for k, v in r.items()}, lwant, "python loss call", LOSS_KEYS)
    for refused in (p.run_block_ring_grad, p.run_block_grad):
        with pytest.raises(F.FlowzError):
            refused(dev(x), dev(tg), dev(s0), dev(par), dev(sb))


def test_autograd_run_far_and_mse_far_match_float64_autograd(F):
    """far257 through torch.autograd against float64 autograd of adjoint_ref.torch_forward (which keeps ages: the state and its
    gradients go through far_grad_ref.convert): the tolerance of the ring tests"""
    from zignal_amd import autograd as AG
    name = "far257"
    p = prog(F, name)
    far = FG.far_rows(p)
    D = FG.DEEPEST[name]
    ns, T = 130, 300
    x, s0, par, yb, sb, _, _ = FG.inputs(p, ns, T, 31)
    xt, st = dev(x).requires_grad_(), dev(s0).requires_grad_()
    ct = torch.tensor(p.consts(), dtype=torch.float32).requires_grad_()
    before = st.detach().clone()
    y, s = AG.run_far(p, xt, st, None, ct)
    y_plain, s_plain = p.run_block(dev(x), dev(s0))
    assert torch.equal(y.detach().view(torch.int32), y_plain.view(torch.int32)) and torch.equal(s.detach().view(torch.int32), s_plain.view(torch.int32))
    assert torch.equal(st.detach(), before)                             # the caller's state is not advanced
    ((y * dev(yb)).sum() + (s * dev(sb)).sum()).backward()
    ages = lambda a, ph: FR.convert(a, [ph], far)[:D]                   # noqa: E731  (the line rows, as adjoint_ref keeps them)
    want = A.torch_grad(p, x, yb, ages(s0, 0), par, ages(sb, T % D))
    assert A.rel_err(xt.grad.cpu().numpy(), want["x"]) <= 1e-4
    sg = st.grad.cpu().numpy()
    assert A.rel_err(ages(sg, 0), want["state"]) <= 1e-4 and not sg[D:].any()      # the phase row's gradient: zero
    assert A.rel_err(ct.grad.numpy(), want["consts"].sum(1)) <= 1e-4
    # and bit for bit what the call under it gives, the coefficient adjoints summed over the streams in float64
    r = launch(p, (x, s0, par, yb, sb, np.zeros((0, ns), F32), np.zeros((p.n_const, ns), F32)))
    assert same(xt.grad.cpu().numpy(), r["x"]) and same(sg, r["state"])
    assert same(ct.grad.numpy(), r["consts"].astype(np.float64).sum(1).astype(F32))
    for refused in (AG.run_rings, AG.run):
        with pytest.raises(F.FlowzError):
            refused(p, xt, st, None, ct)
    # a zero state has phase 0
    y0, s_after = AG.run_far(p, dev(x))
    assert s_after[D, 0].item() == T % D
    # mse_far: ((y - target) ** 2).mean() and its gradients
    xt2, st2 = dev(x).requires_grad_(), dev(s0).requires_grad_()
    ct2 = torch.tensor(p.consts(), dtype=torch.float32).requires_grad_()
    loss = AG.mse_far(p, xt2, dev(yb), st2, None, ct2)
    loss.backward()
    L = A.Layout(p)
    t64 = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=torch.float64, requires_grad=True)   # noqa: E731
    x64, s64, c64 = t64(x), t64(ages(s0, 0)), t64(np.repeat(L.consts.astype(np.float64)[:, None], ns, 1))
    y64, _ = A.torch_forward(L, x64, s64, torch.zeros((0, ns), dtype=torch.float64), c64)
    l64 = ((y64 - torch.tensor(np.asarray(yb, np.float64))) ** 2).mean()
    gx, gs, gc = torch.autograd.grad(l64, (x64, s64, c64))
    assert abs(loss.item() - l64.item()) <= 1e-4 * abs(l64.item())
    assert A.rel_err(xt2.grad.cpu().numpy(), gx.numpy()) <= 1e-4
    assert A.rel_err(ages(st2.grad.cpu().numpy(), 0), gs.numpy()) <= 1e-4 and not st2.grad.cpu().numpy()[D:].any()
    assert A.rel_err(ct2.grad.numpy(), gc.numpy().sum(1)) <= 1e-4
    with pytest.raises(F.FlowzError):
        AG.mse_rings(p, xt2, dev(yb), st2, None, ct2)
