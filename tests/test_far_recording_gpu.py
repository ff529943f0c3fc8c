"""The far recording calls on the MI355X (fz_run_recording_far_grad, fz_run_recording_far_loss_grad: the backward of a whole recording
whose graph has delay lines deeper than 256 samples).  At every shape of tests/far_recording_graphs.py, for the plain and the loss
call: every output bit for bit against the one-launch fz_run_block_far_grad / fz_run_block_far_loss_grad over the same rows and against
tests/far_recording_ref.py; `starts`, read back from the head of the workspace, and state_out against run_block chained over the same
blocks through its own state rows; no state gradient, the state gradient overwritten in place, every output left out in turn -- the
accumulators are never zero --; and autograd.mse_recording_far against float64 autograd.

Every launch goes through the C ABI with a workspace of exactly the queried bytes inside a larger buffer of sentinels, and checks
afterwards that the sentinels around it and around every output, and every input, kept their bits."""
import ctypes

import numpy as np
import pytest

import adjoint_ref as A
import far_grad_graphs as FG
import far_grad_ref as FR
import far_recording_graphs as FRG
import far_recording_ref as RR
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
        _progs[name] = F.compile(F.from_sexpr(FRG.FARS[name]()))
    return _progs[name]


def stride(p, c=0):
    return c or int(p.far_grad_kernel_symbol().split("_c")[1].split("b")[0])


def case(F, name, ns, T, Be, loss):
    """the inputs of a case and far_recording_ref's answer to them at blocks of Be rows, computed once and never modified"""
    key = (name, ns, T, Be, loss)
    if key not in _cases:
        p = prog(F, name)
        d = FRG.inputs(name, ns, T, loss)
        x, s0, par, yt, sb, ap, ac = d[:7]
        if loss:
            want = RR.grad(p, x, Be, target=yt, k=K, state=s0, params=par, state_grad=sb, accum_params=ap, accum_consts=ac, accum_loss=d[7])
        else:
            want = RR.grad(p, x, Be, out_grad=yt, state=s0, params=par, state_grad=sb, accum_params=ap, accum_consts=ac)
        for a in (*d, *want.values()):
            if a is not None:
                a.setflags(write=False)
        _cases[key] = (d, want)
    return _cases[key]


def launch(p, d, loss=False, recording=None, c=0, state_grad=True, alias=False, leave_out=()):
    """One call of the far family through the C ABI on the time-major draw d = (x, s0, par, dL/dy or target, sb, ap, ac[, al]).
    recording None: fz_run_block_far_grad / fz_run_block_far_loss_grad; else the block_rows of fz_run_recording_far_grad /
    fz_run_recording_far_loss_grad (0: the library's choice), and "starts" (the head of the workspace) and "state_out" come back too.
    grad_harness.launch for the far family, which it does not know.  Afterwards: every input kept its bits (state_grad excepted when
    aliased); the workspace is exactly the queried bytes and its surroundings and those of every output kept their sentinels; an output
    that is left out, has zero rows or is aliased away was not written at all."""
    from zignal_amd import _capi as CA
    x, s0, par, yt, sb, ap, ac = d[:7]
    T, ns, _ = x.shape
    rec = recording is not None
    ins = {"in_": dev(x), "state": dev(s0), "params": dev(par), "target" if loss else "out_grad": dev(yt), "state_grad": dev(sb) if state_grad else None}
    before = {key: v.clone() for key, v in ins.items() if v is not None}
    n = {"in_grad": p.n_in, "state0_grad": p.n_state, "param_grad": p.n_param, "const_grad": p.n_const, "loss": 1, "out": p.n_out, "state_out": p.n_state}
    outs = {"in_grad": Guarded((T, ns, max(p.n_in, 1))), "state0_grad": Guarded((max(p.n_state, 1), ns)),
            "param_grad": Guarded((max(p.n_param, 1), ns), ap if p.n_param else None),
            "const_grad": Guarded((max(p.n_const, 1), ns), ac if p.n_const else None)}
    if loss:
        outs.update(loss=Guarded((ns,), d[7]), out=Guarded((T, ns, max(p.n_out, 1))))
    if rec:
        outs["state_out"] = Guarded((max(p.n_state, 1), ns))
    wsb = p.far_recording_workspace_bytes(ns, T, recording, c) if rec else p.far_grad_workspace_bytes(ns, T, c)
    assert wsb % 4 == 0
    ws = Guarded((wsb // 4,))
    a = CA.LossGradArgs() if loss else CA.GradArgs()
    a.struct_size, a.checkpoint_rows = ctypes.sizeof(a), c
    if loss:
        a.grad_scale = K
    for key, t in ins.items():
        setattr(a, key, t.data_ptr() if t is not None and t.numel() else None)
    for key, g in outs.items():
        if key != "state_out":
            setattr(a, key, g.mid.data_ptr() if n[key] and key not in leave_out else None)
    if alias:
        a.state0_grad = ins["state_grad"].data_ptr()
    a.workspace, a.workspace_bytes = ws.mid.data_ptr(), wsb
    hs = torch.cuda.current_stream().cuda_stream
    if rec:
        fn = CA.lib.fz_run_recording_far_loss_grad if loss else CA.lib.fz_run_recording_far_grad
        so = outs["state_out"].mid.data_ptr() if "state_out" not in leave_out else None
        CA.check(fn(p._h, ctypes.byref(a), ns, T, recording, so, hs))
    else:
        fn = CA.lib.fz_run_block_far_loss_grad if loss else CA.lib.fz_run_block_far_grad
        CA.check(fn(p._h, ctypes.byref(a), ns, T, hs))
    torch.cuda.synchronize()
    for key, t in before.items():
        if not (alias and key == "state_grad"):
            assert torch.equal(ins[key].view(torch.int32), t.view(torch.int32)), f"input {key} was written"
    assert ws.guards_kept(), "the workspace's surroundings were written"
    gone = {key for key in outs if key in leave_out or not n[key] or (alias and key == "state0_grad")}
    got = {}
    for key, g in outs.items():
        assert g.guards_kept(), f"the surroundings of {key} were written"
        if key in gone:
            assert g.untouched(), f"{key} was left out and written"
    for key, b in H.OUT.items():
        if b in outs and b not in gone:
            got[key] = outs[b].mid.cpu().numpy()
    if alias and "state0_grad" not in leave_out:
        got["state"] = ins["state_grad"].cpu().numpy()
    if rec:
        if "state_out" not in leave_out:
            got["state_out"] = outs["state_out"].mid.cpu().numpy()
        nb = -(-T // p.far_recording_block_rows(T, recording, c))
        got["starts"] = ws.mid[:nb * p.n_state * ns].view(nb, p.n_state, ns).cpu().numpy()
    return got


def check(p, got, want, what, keys):
    has = {"x": p.n_in, "state": p.n_state, "params": p.n_param, "consts": p.n_const, "loss": 1, "out": p.n_out, "state_out": p.n_state}
    assert set(got) >= {k for k in keys if has[k]}, f"{what}: {sorted(got)} lacks a result"
    H.check(p, got, want, what, keys)


def forward_starts(p, d, Be):
    """run_block chained over the blocks through its own state rows: (the state before every block, the state after the last row)"""
    x, s0, par = d[:3]
    xd, s, pd = dev(x), dev(s0), dev(par)
    out = []
    for t0 in range(0, x.shape[0], Be):
        out.append(s.clone())
        _, s = p.run_block(xd[t0:t0 + Be].contiguous(), s, pd)
    torch.cuda.synchronize()
    return torch.stack(out).cpu().numpy(), s.cpu().numpy()


@pytest.mark.parametrize("loss", [False, True])
@pytest.mark.parametrize("name", sorted(FRG.FARS))
def test_far_recording_matches_the_one_launch_call_and_the_reference_bitwise(F, name, loss):
    p = prog(F, name)
    keys = LOSS_KEYS if loss else KEYS
    for ns, T, B, c in FRG.shapes(name):
        what = f"{name} loss={loss} ns={ns} T={T} B={B} C={c}"
        Be = FRG.block_rows(name, T, stride(p, c), B)
        assert Be == p.far_recording_block_rows(T, B, c), what
        d, want = case(F, name, ns, T, Be, loss)
        assert all(d[1][pr, 0] == FRG.p0_of(name) % dd for _, dd, pr in FG.far_rows(p))
        got = launch(p, d, loss, recording=B, c=c)
        one = launch(p, d, loss, c=c)
        check(p, got, one, what + " against one launch", keys)
        check(p, got, want, what + " against far_recording_ref", keys + ("state_out",))
        assert same(got["starts"], want["starts"]), what + ": starts against far_recording_ref"
        fs, fo = forward_starts(p, d, Be)
        assert same(got["starts"], fs), what + ": starts against run_block"
        assert same(got["state_out"], fo), what + ": state_out against run_block"
        # the far lines' phase rows, as the forward writes them
        for _, dd, pr in FG.far_rows(p):
            assert all(got["starts"][k, pr, 0] == (FRG.p0_of(name) + k * Be) % dd for k in range(len(fs))) and got["state_out"][pr, 0] == (FRG.p0_of(name) + T) % dd


@pytest.mark.parametrize("loss", [False, True])
@pytest.mark.parametrize("name", sorted(FRG.FARS))
def test_variations_match_the_one_launch_call(F, name, loss):
    """no state gradient; state0_grad in place; every output left out in turn (state0_grad too: with more than one block the call asks
    for it, so that is refused and with one block honoured); all on accumulators that are not zero"""
    p = prog(F, name)
    keys = LOSS_KEYS if loss else KEYS
    has = {"x": p.n_in, "state": p.n_state, "params": p.n_param, "consts": p.n_const, "loss": 1, "out": p.n_out}
    for ns, T, B, c in FRG.shapes(name):
        what = f"{name} loss={loss} ns={ns} T={T} B={B} C={c}"
        d = FRG.inputs(name, ns, T, loss)
        assert d[5].any() or not p.n_param
        assert d[6].any() or not p.n_const
        check(p, launch(p, d, loss, recording=B, c=c, state_grad=False), launch(p, d, loss, c=c, state_grad=False), what + " no state_grad", keys)
        check(p, launch(p, d, loss, recording=B, c=c, alias=True), launch(p, d, loss, c=c, alias=True), what + " in place", keys)
        whole = launch(p, d, loss, c=c)
        for b in ("in_grad", "param_grad", "const_grad") + (("loss", "out") if loss else ()) + ("state_out",):
            got = launch(p, d, loss, recording=B, c=c, leave_out=(b,))
            assert set(got) - {"starts", "state_out"} == {k for k in keys if H.OUT[k] != b and has[k]}, what
            assert ("state_out" in got) == (b != "state_out")
            H.check(p, got, whole, what + f" without {b}", keys)
        nb = -(-T // p.far_recording_block_rows(T, B, c))
        if nb == 1:
            got = launch(p, d, loss, recording=B, c=c, leave_out=("state0_grad",))
            assert "state" not in got
            H.check(p, got, whole, what + " without state0_grad", keys)
        else:
            with pytest.raises(F.FlowzError) as ei:
                launch(p, d, loss, recording=B, c=c, leave_out=("state0_grad",))
            assert "state0_grad is null" in str(ei.value)


def test_python_calls_return_the_dict_of_the_ring_recording_calls(F):
    name = "far_mixed"
    p = prog(F, name)
    ns, T, B, c = FRG.shapes(name)[2]
    for loss in (False, True):
        keys = LOSS_KEYS if loss else KEYS
        d, want = case(F, name, ns, T, B, loss)
        x, s0, par, yt, sb, ap, ac = d[:7]
        accum = {"params": dev(ap), "consts": dev(ac)}
        if loss:
            r = p.run_recording_far_loss_grad(dev(x), dev(yt), dev(s0), dev(par), dev(sb), grad_scale=K, want=keys + ("state_out",),
                                              accum=dict(accum, loss=dev(d[7])), block_rows=B)
        else:
            r = p.run_recording_far_grad(dev(x), dev(yt), dev(s0), dev(par), dev(sb), want=keys + ("state_out",), accum=accum, block_rows=B)
        torch.cuda.synchronize()
        assert set(r) == set(keys) | {"state_out"}
        check(p, {k: v.cpu().numpy() for k, v in r.items()}, want, f"python call loss={loss}", keys + ("state_out",))
        for refused in ((p.run_recording_ring_loss_grad, p.run_recording_loss_grad) if loss else (p.run_recording_ring_grad, p.run_recording_grad)):
            with pytest.raises(F.FlowzError):
                refused(dev(x), dev(yt), dev(s0), dev(par), dev(sb), block_rows=B)


def test_autograd_mse_recording_far_matches_float64_autograd(F):
    """far257 through torch.autograd against float64 autograd of adjoint_ref.torch_forward (which keeps ages: the state and its gradient
    go through far_grad_ref.convert): the tolerance test_far_grad_gpu.py holds mse_far to"""
    from zignal_amd import autograd as AG
    name = "far257"
    p = prog(F, name)
    far = FG.far_rows(p)
    D = FG.DEEPEST[name]
    ns, T, B = 130, 300, 64
    x, s0, par, yb, sb, _, _ = FG.inputs(p, ns, T, 31)
    ages = lambda a, ph: FR.convert(a, [ph], far)[:D]                   # noqa: E731  (the line rows, as adjoint_ref keeps them)
    xt, st = dev(x).requires_grad_(), dev(s0).requires_grad_()
    ct = torch.tensor(p.consts(), dtype=torch.float32).requires_grad_()
    loss, state_out = AG.mse_recording_far(p, xt, dev(yb), st, None, ct, block_rows=B)
    loss.backward()
    L = A.Layout(p)
    t64 = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=torch.float64, requires_grad=True)   # noqa: E731
    x64, s64, c64 = t64(x), t64(ages(s0, 0)), t64(np.repeat(L.consts.astype(np.float64)[:, None], ns, 1))
    y64, _ = A.torch_forward(L, x64, s64, torch.zeros((0, ns), dtype=torch.float64), c64)
    l64 = ((y64 - torch.tensor(np.asarray(yb, np.float64))) ** 2).mean()
    gx, gs, gc = torch.autograd.grad(l64, (x64, s64, c64))
    assert abs(loss.item() - l64.item()) <= 1e-4 * abs(l64.item())
    assert A.rel_err(xt.grad.cpu().numpy(), gx.numpy()) <= 1e-4
    assert A.rel_err(ages(st.grad.cpu().numpy(), 0), gs.numpy()) <= 1e-4 and not st.grad.cpu().numpy()[D:].any()
    assert A.rel_err(ct.grad.numpy(), gc.numpy().sum(1)) <= 1e-4
    # the state after the recording is run_block's, phase row included; the bits are mse_far's over the same rows
    _, s_plain = p.run_block(dev(x), dev(s0))
    assert torch.equal(state_out.view(torch.int32), s_plain.view(torch.int32)) and not state_out.requires_grad
    xt2 = dev(x).requires_grad_()
    AG.mse_far(p, xt2, dev(yb), dev(s0)).backward()
    assert same(xt.grad.cpu().numpy(), xt2.grad.cpu().numpy())
    with pytest.raises(F.FlowzError):
        AG.mse_recording_rings(p, dev(x), dev(yb), dev(s0), block_rows=B)
