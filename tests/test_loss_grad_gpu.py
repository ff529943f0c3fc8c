"""The backward under a squared-error loss on the MI355X (fz_run_block_loss_grad, fz_run_block_loss_grad_stream_major): in_grad,
state0_grad, param_grad, const_grad, loss and out bit for bit against tests/loss_grad_ref.py, in both layouts, around every boundary the
kernels have (wave, checkpoint chunk, LDS patch); chaining, checkpoint strides, subsets, windows, repeatability, and autograd.mse."""
import ctypes
import re

import numpy as np
import pytest

import adjoint_ref as A
import grad_graphs as GG
import loss_grad_ref as LR
import grad_harness as H
from grad_harness import F32, K, SENTINEL, dev, gpu_flowz, make_inputs, outside_keeps_sentinel, same, to_sm, up4
from grad_harness import on_gpu_loss as on_gpu

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GRAPHS = ["df1_cascade_params6", "moog_ladder", "rules", "par4_sum", "div_sqrt_exp"]
KEYS = H.LOSS_KEYS


@pytest.fixture(scope="module")
def F():
    return gpu_flowz()


_progs = {}


def prog(F, name):
    if name not in _progs:
        _progs[name] = F.compile(F.from_sexpr(GG.SUPPORTED[name]()))
    return _progs[name]


def strides(p):
    """(C, R): the stream-major loss kernel's symbol names them; the time-major kernel's C is the same"""
    m = re.match(r"fz_adjoint_loss_sm_kernel_c(\d+)r(\d+)b", p.loss_grad_kernel_symbol(stream_major=True))
    assert p.loss_grad_kernel_symbol().startswith(f"fz_adjoint_loss_kernel_c{m.group(1)}b")
    return int(m.group(1)), int(m.group(2))


def draw(p, name, ns, T, seed):
    """make_inputs' draws (dL/dy serves as the target: standard normal) and a loss accumulator that is not zero"""
    x, s0, par, tg, sb, ap, ac = make_inputs(p, name, ns, T, seed)
    al = np.random.default_rng(seed + 1).standard_normal(ns).astype(F32)
    return x, s0, par, tg, sb, ap, ac, al


def check(p, got, want, what):
    H.check(p, got, want, what, KEYS)


@pytest.mark.parametrize("name", GRAPHS)
def test_both_layouts_match_the_restatement_bitwise(F, name):
    p = prog(F, name)
    C, R = strides(p)
    shapes = [(ns, T) for ns in (1, 63, 64, 1000) for T in sorted({1, max(C - 1, 1), C, C + 1})] + [(65, 4 * R + 3)]
    for i, (ns, T) in enumerate(shapes):
        d = draw(p, name, ns, T, 500 + i)
        x, s0, par, tg, sb, ap, ac, al = d
        want = LR.loss_grad(p, x, tg, K, s0, par, sb, ap, ac, al)
        y, _ = p.run_block(dev(x), dev(s0) if p.n_state else None, dev(par))
        assert same(want["out"], y.cpu().numpy()), f"{name}: the restated y is not run_block's"
        for sm in (False, True):
            what = f"{name} ns={ns} T={T} (C={C}, R={R}) {'stream' if sm else 'time'}-major"
            got = on_gpu(p, sm, *d)
            check(p, got, want, what)
            if sm:
                assert outside_keeps_sentinel(got["x_buffer"], 0, T) and outside_keeps_sentinel(got["out_buffer"], 0, T), what + ": rows behind the window written"


@pytest.mark.parametrize("sm", [False, True])
@pytest.mark.parametrize("name", GRAPHS)
def test_two_blocks_chain_like_one(F, name, sm):
    """the second block, then the first on the same three accumulators (loss included) with the second's state adjoint: one block of 2T's bits"""
    p = prog(F, name)
    C, R = strides(p)
    ns, T = 200, R + C + 3
    x, s0, par, tg, sb, ap, ac, al = draw(p, name, ns, 2 * T, 9)
    whole = on_gpu(p, sm, x, s0, par, tg, sb, ap, ac, al)
    _, s_mid = p.run_block(dev(x[:T]), dev(s0) if p.n_state else None, dev(par))
    s_mid = s_mid.cpu().numpy()
    second = on_gpu(p, sm, x[T:], s_mid, par, tg[T:], sb, ap, ac, al)
    first = on_gpu(p, sm, x[:T], s0, par, tg[:T], second["state"], second["params"], second["consts"], second["loss"])
    chained = dict(first, x=np.concatenate([first["x"], second["x"]]), out=np.concatenate([first["out"], second["out"]]))
    check(p, chained, whole, f"{name} chained")


@pytest.mark.parametrize("sm", [False, True])
@pytest.mark.parametrize("name", GRAPHS)
def test_bits_do_not_depend_on_the_checkpoint_stride(F, name, sm):
    p = prog(F, name)
    d = draw(p, name, 300, 77, 13)
    ref = on_gpu(p, sm, *d)
    for c in (1, 4):
        check(p, on_gpu(p, sm, *d, checkpoint_rows=c), ref, f"{name} C={c}")


@pytest.mark.parametrize("sm", [False, True])
def test_want_subsets_leave_the_other_buffers_alone(F, sm):
    from zignal_amd import _capi as CA
    name = "moog_ladder"
    p = prog(F, name)
    ns, T, rows = 129, 41, 44
    x, s0, par, tg, sb, ap, ac, al = draw(p, name, ns, T, 17)
    full = on_gpu(p, sm, x, s0, par, tg, sb, ap, ac, al, rows=rows)
    names = {"x": "in_grad", "state": "state0_grad", "params": "param_grad", "consts": "const_grad", "loss": "loss", "out": "out"}
    fshape = lambda w: (ns, rows, w) if sm else (T, ns, w)        # noqa: E731
    for want in (("x",), ("state",), ("params",), ("consts",), ("loss",), ("out",), ("x", "consts"), ("state", "params", "loss"), ("out", "loss"), ()):
        bufs = {"in_grad": torch.full(fshape(p.n_in), float(SENTINEL), device="cuda"), "state0_grad": torch.full((p.n_state, ns), float(SENTINEL), device="cuda"),
                "param_grad": dev(ap), "const_grad": dev(ac), "loss": dev(al), "out": torch.full(fshape(p.n_out), float(SENTINEL), device="cuda")}
        before = {k: v.clone() for k, v in bufs.items()}
        ws = torch.empty(max(p.grad_workspace_bytes(ns, T), 16) // 4, device="cuda")
        a = CA.LossGradArgs()
        a.struct_size, a.grad_scale = ctypes.sizeof(CA.LossGradArgs), K
        keep = [dev(to_sm(x, rows) if sm else x), dev(s0), dev(par), dev(to_sm(tg, rows) if sm else tg), dev(sb)]
        a.in_, a.state, a.params, a.target, a.state_grad = (t.data_ptr() for t in keep)
        for k, b in names.items():
            setattr(a, b, bufs[b].data_ptr() if k in want else None)
        a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel() * 4
        hs = torch.cuda.current_stream().cuda_stream
        CA.check(CA.lib.fz_run_block_loss_grad_stream_major(p._h, ctypes.byref(a), ns, rows, 0, T, hs) if sm else
                 CA.lib.fz_run_block_loss_grad(p._h, ctypes.byref(a), ns, T, hs))
        torch.cuda.synchronize()
        for k, b in names.items():
            got = bufs[b].cpu().numpy()
            if k in want:
                w = full[k + "_buffer"] if sm and k in ("x", "out") else full[k]
                assert same(got, w if k in ("x", "out", "loss") else w[:got.shape[0]]), (want, k)
            else:
                assert torch.equal(bufs[b], before[b]), (want, k)


@pytest.mark.parametrize("name", GRAPHS)
def test_a_window_of_a_larger_buffer_leaves_the_rows_outside_it_alone(F, name):
    p = prog(F, name)
    C, R = strides(p)
    for ns, row0, T, tail in ((200, 4, R + 5, 9), (65, 2 * R, 2 * R + 3, 0), (130, 8, 3, 1)):
        rows = up4(row0 + T + tail)
        d = draw(p, name, ns, T, 31 + T)
        got = on_gpu(p, True, *d, rows=rows, row0=row0)
        check(p, got, on_gpu(p, False, *d), f"{name} window [{row0}, {row0 + T}) of {rows}")
        assert outside_keeps_sentinel(got["x_buffer"], row0, T), f"{name}: rows of in_grad outside [{row0}, {row0 + T}) were written"
        assert outside_keeps_sentinel(got["out_buffer"], row0, T), f"{name}: rows of out outside [{row0}, {row0 + T}) were written"


@pytest.mark.parametrize("sm", [False, True])
def test_two_launches_give_identical_bits(F, sm):
    p = prog(F, "df1_cascade_params6")
    d = draw(p, "df1_cascade_params6", 777, 50, 19)
    check(p, on_gpu(p, sm, *d), on_gpu(p, sm, *d), "repeat")


# ---- autograd.mse --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sm", [False, True])
def test_mse_equals_run_then_torch_mse(F, sm):
    """value and gradients against the route before it: AG.run, ((y - target) ** 2).mean(), backward().  torch rounds the error, its
    square and their mean differently, so the comparison is the relative one test_autograd_chain_over_two_blocks uses for sums
    whose order differs"""
    from zignal_amd import autograd as AG
    name = "moog_ladder"
    p = prog(F, name)
    ns, T = 500, 40
    x, s0, par, tg, sb, ap, ac, al = draw(p, name, ns, T, 23)
    xin, tgd = (dev(to_sm(x, T)), dev(to_sm(tg, T))) if sm else (dev(x), dev(tg))

    def route(fused):
        xt, st, pt = xin.clone().requires_grad_(), dev(s0).requires_grad_(), dev(par).requires_grad_()
        ct = torch.tensor(p.consts(), dtype=torch.float32).requires_grad_()
        if fused:
            loss = AG.mse(p, xt, tgd, st, pt, ct, stream_major=sm)
        else:
            y, _ = AG.run(p, xt, st, pt, ct, stream_major=sm)
            loss = ((y - tgd) ** 2).mean()
        (loss * 3.0).backward()                                       # (an upstream scalar that is not 1)
        return loss.item(), xt.grad.cpu().numpy(), st.grad.cpu().numpy(), pt.grad.cpu().numpy(), ct.grad.numpy()
    got, want = route(True), route(False)
    errs = [abs(got[0] - want[0]) / abs(want[0])] + [A.rel_err(g, w) for g, w in zip(got[1:], want[1:])]
    print("mse vs run + torch: relative errors of value, x, state, params, consts:", errs)
    assert tuple(got[1].shape) == tuple(xin.shape)
    assert all(e <= 1e-6 for e in errs), errs


def test_mse_computes_dx_only_if_x_requires_grad_and_takes_batch_by_time_tensors(F):
    from zignal_amd import autograd as AG
    p = prog(F, "df1_cascade_params6")
    ns, T = 256, 48
    x, s0, par, tg, sb, ap, ac, al = draw(p, "df1_cascade_params6", ns, T, 27)
    x2, t2 = dev(to_sm(x, T)[:, :, 0]), dev(to_sm(tg, T)[:, :, 0])            # [batch, time]
    pt = dev(par).requires_grad_()
    loss = AG.mse(p, x2, t2, dev(s0), pt, stream_major=True)
    loss.backward()
    want = LR.loss_grad(p, x, tg, 2.0 / (T * ns), s0, par)
    assert same(pt.grad.cpu().numpy(), want["params"])
    xg = x2.clone().requires_grad_()
    AG.mse(p, xg, t2, dev(s0), dev(par), stream_major=True).backward()
    assert tuple(xg.grad.shape) == (ns, T) and same(xg.grad.cpu().numpy().T[:, :, None], want["x"])


def test_adam_fits_per_stream_one_pole_coefficients_with_mse(F):
    from zignal_amd import autograd as AG
    import graphs as G
    p = F.compile(F.from_sexpr(G.fb(G.add(G.mul(G.param(0), G.DEL(1, 1)), G.IN(2)))))
    ns, T = 4096, 256
    gen = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn((T, ns, 1), device="cuda", generator=gen)
    a_true = torch.rand((1, ns), device="cuda", generator=gen) * 0.7 + 0.2
    target, _ = p.run_block(x, None, a_true.contiguous())
    a = torch.full((1, ns), 0.5, device="cuda", requires_grad=True)
    opt = torch.optim.Adam([a], lr=0.05)
    losses = []
    for _ in range(50):
        opt.zero_grad()
        loss = AG.mse(p, x, target, None, a)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert losses[-1] * 10 <= losses[0], (losses[0], losses[-1])
