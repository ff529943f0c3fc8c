"""The adjoint kernel on the MI355X (fz_run_block_grad): every output bit for bit against tests/adjoint_ref.py, the numpy statement
of the documented order; chaining, checkpoint strides, subsets, repeatability, and the torch.autograd.Function over it."""
import ctypes

import numpy as np
import pytest

import adjoint_ref as A
import grad_graphs as GG
import grad_harness as H
from grad_harness import F32, dev, gpu_flowz, make_inputs, on_gpu, same

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

KEYS = H.GRAD_KEYS


@pytest.fixture(scope="module")
def F():
    return gpu_flowz()


_progs = {}


def prog(F, name):
    if name not in _progs:
        _progs[name] = F.compile(F.from_sexpr(GG.SUPPORTED[name]()))
    return _progs[name]


def stride(p):
    return int(p.grad_kernel_symbol().split("_c")[1].split("b")[0])


def check(p, got, want, what):
    H.check(p, got, want, what, KEYS)


@pytest.mark.parametrize("name", sorted(GG.SUPPORTED))
def test_adjoint_matches_reference_bitwise(F, name):
    p = prog(F, name)
    C = stride(p)
    shapes = [(ns, T) for ns in (1, 63, 64, 1000) for T in sorted({1, max(C - 1, 1), C, C + 1})] + [(63, 1000), (1000, 1000)]
    for i, (ns, T) in enumerate(shapes):
        x, s0, par, yb, sb, ap, ac = make_inputs(p, name, ns, T, 100 + i)
        got = on_gpu(p, x, s0, par, yb, sb, ap, ac)
        want = A.grad(p, x, yb, s0, par, sb, ap, ac)
        check(p, got, want, f"{name} ns={ns} T={T}")


@pytest.mark.parametrize("name", ["df1_cascade6", "moog_ladder"])
def test_adjoint_many_streams(F, name):
    p = prog(F, name)
    ns, T = 65537, stride(p) + 3
    x, s0, par, yb, sb, ap, ac = make_inputs(p, name, ns, T, 7)
    check(p, on_gpu(p, x, s0, par, yb, sb, ap, ac), A.grad(p, x, yb, s0, par, sb, ap, ac), f"{name} ns={ns}")


@pytest.mark.parametrize("name", ["df1_cascade6", "osc_chain6", "moog_ladder", "rules", "cross_wire"])
def test_two_blocks_chain_like_one(F, name):
    """the backward of block 2, then of block 1 on the same accumulators with block 2's state adjoint, gives one block of 2T's bits"""
    p = prog(F, name)
    ns, T = 200, stride(p) + 3
    x, s0, par, yb, sb, ap, ac = make_inputs(p, name, ns, 2 * T, 9)
    whole = on_gpu(p, x, s0, par, yb, sb, ap, ac)
    y, s_mid = p.run_block(dev(x[:T]), dev(s0) if p.n_state else None, dev(par))
    s_mid = s_mid.cpu().numpy()
    second = on_gpu(p, x[T:], s_mid, par, yb[T:], sb, ap, ac)
    first = on_gpu(p, x[:T], s0, par, yb[:T], second["state"], second["params"], second["consts"])
    chained = {"x": np.concatenate([first["x"], second["x"]]), "state": first["state"], "params": first["params"], "consts": first["consts"]}
    check(p, chained, whole, f"{name} chained")


@pytest.mark.parametrize("name", ["df1_cascade6", "moog_ladder", "envelope_follower", "div_sqrt_exp"])
def test_bits_do_not_depend_on_the_checkpoint_stride(F, name):
    p = prog(F, name)
    ns, T = 300, 37
    x, s0, par, yb, sb, ap, ac = make_inputs(p, name, ns, T, 13)
    ref = on_gpu(p, x, s0, par, yb, sb, ap, ac)
    for c in (1, 4):
        check(p, on_gpu(p, x, s0, par, yb, sb, ap, ac, checkpoint_rows=c), ref, f"{name} C={c}")


def test_want_subset_and_sentinels(F):
    name = "moog_ladder"
    p = prog(F, name)
    ns, T = 129, 21
    x, s0, par, yb, sb, ap, ac = make_inputs(p, name, ns, T, 17)
    full = on_gpu(p, x, s0, par, yb, sb, ap, ac)
    sentinel = np.float32(-1234.5)
    for want in (("x",), ("state",), ("params",), ("consts",), ("x", "consts"), ("state", "params")):
        bufs = {"in_grad": torch.full((T, ns, p.n_in), sentinel, device="cuda"), "state0_grad": torch.full((p.n_state, ns), sentinel, device="cuda"),
                "param_grad": dev(ap), "const_grad": dev(ac)}
        before = {k: v.clone() for k, v in bufs.items()}
        names = {"x": "in_grad", "state": "state0_grad", "params": "param_grad", "consts": "const_grad"}
        ws = torch.empty(max(p.grad_workspace_bytes(ns, T), 16) // 4, device="cuda")
        from zignal_amd import _capi as CA
        a = CA.GradArgs()
        a.struct_size = ctypes.sizeof(CA.GradArgs)
        keep = [dev(x), dev(s0), dev(par), dev(yb), dev(sb)]
        a.in_, a.state, a.params, a.out_grad, a.state_grad = (t.data_ptr() for t in keep)
        for k, b in names.items():
            setattr(a, b, bufs[b].data_ptr() if k in want else None)
        a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel() * 4
        CA.check(CA.lib.fz_run_block_grad(p._h, ctypes.byref(a), ns, T, torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        for k, b in names.items():
            got = bufs[b].cpu().numpy()
            if k in want:
                assert same(got, full[k][:got.shape[0]]), (want, k)
            else:
                assert torch.equal(bufs[b], before[b]), (want, k)


def test_two_launches_give_identical_bits(F):
    p = prog(F, "soft_clip_cascade")
    x, s0, par, yb, sb, ap, ac = make_inputs(p, "soft_clip_cascade", 777, 50, 19)
    a, b = on_gpu(p, x, s0, par, yb, sb, ap, ac), on_gpu(p, x, s0, par, yb, sb, ap, ac)
    check(p, a, b, "repeat")


# ---- torch.autograd -----------------------------------------------------------------------------------------------------------
def test_autograd_run_equals_run_block_grad(F):
    from zignal_amd import autograd as AG
    name = "moog_ladder"
    p = prog(F, name)
    ns, T = 500, 40
    x, s0, par, yb, sb, ap, ac = make_inputs(p, name, ns, T, 23)
    xt, st, pt = dev(x).requires_grad_(), dev(s0).requires_grad_(), dev(par).requires_grad_()
    ct = torch.tensor(p.consts(), dtype=torch.float32).requires_grad_()
    st_before = st.detach().clone()
    y, s = AG.run(p, xt, st, pt, ct)
    y_plain, _ = p.run_block(dev(x), dev(s0), dev(par))
    assert torch.equal(y.detach().view(torch.int32), y_plain.view(torch.int32))
    assert torch.equal(st.detach(), st_before)                          # the caller's state is not advanced
    loss = (y * dev(yb)).sum() + (s * dev(sb)).sum()
    loss.backward()
    r = on_gpu(p, x, s0, par, yb, sb, np.zeros_like(ap), np.zeros_like(ac))
    assert same(xt.grad.cpu().numpy(), r["x"]) and same(st.grad.cpu().numpy(), r["state"]) and same(pt.grad.cpu().numpy(), r["params"])
    want_c = r["consts"][:p.n_const].astype(np.float64).sum(1).astype(F32)
    assert same(ct.grad.numpy(), want_c)


def test_autograd_chain_over_two_blocks(F):
    from zignal_amd import autograd as AG
    name = "df1_cascade6"
    p = prog(F, name)
    ns, T = 256, 45
    x, s0, par, yb, sb, ap, ac = make_inputs(p, name, ns, 2 * T, 29)
    ct0 = torch.tensor(p.consts(), dtype=torch.float32)

    def grads(blocks):
        xt, st, ct = dev(x).requires_grad_(), dev(s0).requires_grad_(), ct0.clone().requires_grad_()
        s, loss = st, 0
        for lo, hi in blocks:
            y, s = AG.run(p, xt[lo:hi].contiguous() if len(blocks) > 1 else xt, s, None, ct)
            loss = loss + (y * dev(yb[lo:hi])).sum()
        loss = loss + (s * dev(sb)).sum()
        loss.backward()
        return xt.grad.cpu().numpy(), st.grad.cpu().numpy(), ct.grad.numpy()
    gx1, gs1, gc1 = grads([(0, 2 * T)])
    gx2, gs2, gc2 = grads([(0, T), (T, 2 * T)])
    assert same(gx1, gx2) and same(gs1, gs2)
    assert A.rel_err(gc2, gc1) <= 1e-6


def test_adam_fits_per_stream_one_pole_coefficients(F):
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
        y, _ = AG.run(p, x, None, a)
        loss = ((y - target) ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert losses[-1] * 10 <= losses[0], (losses[0], losses[-1])
