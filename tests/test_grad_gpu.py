"""The adjoint kernel on the MI355X (fz_run_block_grad): every output bit for bit against tests/adjoint_ref.py, the numpy statement
of the documented order; chaining, checkpoint strides, subsets, repeatability, and the torch.autograd.Function over it."""
import ctypes

import numpy as np
import pytest

import adjoint_ref as A
import grad_graphs as GG

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

F32 = np.float32
KEYS = ("x", "state", "params", "consts")


@pytest.fixture(scope="module")
def F():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from zignal_amd import flowz
    return flowz


_progs = {}


def prog(F, name):
    if name not in _progs:
        _progs[name] = F.compile(F.from_sexpr(GG.SUPPORTED[name]()))
    return _progs[name]


def stride(p):
    return int(p.grad_kernel_symbol().split("_c")[1].split("b")[0])


def same(a, b):
    """bit for bit, a NaN of any payload equal to a NaN"""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    if a.shape != b.shape:
        return False
    eq = a.view(np.uint32) == b.view(np.uint32)
    return bool(np.all(eq | (np.isnan(a) & np.isnan(b))))


def make_inputs(p, name, ns, T, seed, ties=None, draw_params=None, special_every=1):
    """x, state, params, dL/dy, dL/d(state after) and the two accumulators, none of them zero.  ties (default: by name): the ties and
    specials below mixed into x -- special_every = k: only into every k-th stream, the others stay finite (behind a feedback a NaN
    never leaves its stream); draw_params(p, ns, rng): the per-stream coefficients of a graph that is none of the named ones"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((T, ns, p.n_in)) * 0.5).astype(F32)
    if name == "div_sqrt_exp":
        x = np.abs(x)
    if name in ("rules", "envelope_follower", "clipped_biquad") if ties is None else ties:
        # ties of MIN / MAX (equal values, +0 against -0), +-0 under ABS, NaN and inf through the comparisons
        special = np.array([0.0, -0.0, 1.0, 0.5, np.nan, np.inf, -np.inf, 0.75], F32)
        m = rng.random(x.shape) < 0.2
        m[:, np.arange(ns) % special_every != 0] = False
        x[m] = special[rng.integers(0, special.size, int(m.sum()))]
        if p.n_in >= 2:
            tie = rng.random((T, ns)) < 0.2
            x[:, :, 1][tie] = x[:, :, 0][tie]
    s0 = (rng.standard_normal((p.n_state, ns)) * 0.1).astype(F32)
    par = None
    if p.n_param:
        if draw_params is not None:
            par = draw_params(p, ns, rng)
        elif name == "moog_ladder":
            par = rng.uniform(0.05, 0.5, (1, ns)).astype(F32)
        elif name == "osc_chain6":
            import graphs as G
            par = np.asarray(G.osc_chain_params(G.SEED, np.arange(ns)), F32)
        else:
            import graphs as G
            par = np.empty((p.n_param, ns), F32)
            for j in range(p.n_param // 5):
                par[5 * j:5 * j + 5] = np.asarray(G.STABLE, F32)[:, None] * rng.uniform(0.9, 1.0, (5, ns)).astype(F32)
    yb = rng.standard_normal((T, ns, p.n_out)).astype(F32)
    sb = rng.standard_normal((p.n_state, ns)).astype(F32)
    ap = rng.standard_normal((p.n_param, ns)).astype(F32)
    ac = rng.standard_normal((p.n_const, ns)).astype(F32)
    return x, s0, par, yb, sb, ap, ac


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda() if a is not None else None


def on_gpu(p, x, s0, par, yb, sb, ap, ac, checkpoint_rows=0, want=KEYS):
    accum = {}
    if p.n_param and "params" in want:
        accum["params"] = dev(ap)
    if p.n_const and "consts" in want:
        accum["consts"] = dev(ac)
    r = p.run_block_grad(dev(x), dev(yb), dev(s0) if p.n_state else None, dev(par), dev(sb) if p.n_state else None, want=want,
                         accum=accum, checkpoint_rows=checkpoint_rows)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in r.items()}


def check(p, got, want, what):
    for k in KEYS:
        if k not in got:
            continue
        rows = {"x": None, "state": p.n_state, "params": p.n_param, "consts": p.n_const}[k]
        g = got[k] if rows is None else got[k][:rows]
        w = want[k] if rows is None else want[k][:rows]
        assert same(g, w), f"{what}: {k} differs in {int((~((g.view(np.uint32) == w.view(np.uint32)) | (np.isnan(g) & np.isnan(w)))).sum())} of {g.size}"


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
