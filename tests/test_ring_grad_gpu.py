"""The ring adjoint kernel on the MI355X (fz_run_block_ring_grad: graphs with delay lines deeper than 8 samples): every output bit for
bit against tests/adjoint_ref.py, at the row counts around each line's depth and the stream counts around a wave and a workgroup;
checkpoint strides, a missing state gradient, the state gradient overwritten in place, every output left out in turn, two chained
blocks of which the first is shorter than the line, the inputs and the workspace's surroundings untouched; autograd over it.

Every launch goes through the C ABI with a workspace of exactly the queried bytes inside a larger buffer of sentinels, and checks
afterwards that the sentinels and every input kept their bits."""
import ctypes

import numpy as np
import pytest

import adjoint_ref as A
import grad_graphs as GG
import ring_grad_graphs as RG

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

F32 = np.float32
KEYS = ("x", "state", "params", "consts")
OUT = {"x": "in_grad", "state": "state0_grad", "params": "param_grad", "consts": "const_grad"}
SENTINEL = np.float32(-1234.5)


@pytest.fixture(scope="module")
def F():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from zignal_amd import flowz
    return flowz


_progs, _cases = {}, {}


def prog(F, name):
    if name not in _progs:
        _progs[name] = F.compile(F.from_sexpr((RG.RINGS.get(name) or GG.SUPPORTED[name])()))
    return _progs[name]


def case(F, name, ns, T, seed=0):
    """the inputs of a case and adjoint_ref's answer to them, computed once and never modified"""
    key = (name, ns, T, seed)
    if key not in _cases:
        p = prog(F, name)
        x, s0, par, yb, sb, ap, ac = RG.inputs(p, ns, T, 1000 * seed + 7 * ns + T)
        want = A.grad(p, x, yb, s0, par, sb, ap, ac)
        for a in (x, s0, par, yb, sb, ap, ac, *want.values()):
            if a is not None:
                a.setflags(write=False)
        _cases[key] = ((x, s0, par, yb, sb, ap, ac), want)
    return _cases[key]


def stride(p):
    return int(p.ring_grad_kernel_symbol().split("_c")[1].split("b")[0])


def same(a, b):
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def dev(a):
    return torch.from_numpy(np.array(a, F32, order="C")).cuda() if a is not None else None     # (a copy: the cases are read-only)


def launch(p, inputs, checkpoint_rows=0, state_grad=True, alias=False, leave_out=(), fn="fz_run_block_ring_grad"):
    """one call through the C ABI: dict of the outputs asked for (numpy).  The accumulators start from ap / ac.  alias: state0_grad is
    the state_grad buffer.  Afterwards: the inputs kept their bits, outputs left out and the workspace's surroundings their sentinels."""
    from zignal_amd import _capi as CA
    x, s0, par, yb, sb, ap, ac = inputs
    T, ns, _ = x.shape
    ins = {"in_": dev(x), "state": dev(s0), "params": dev(par), "out_grad": dev(yb), "state_grad": dev(sb) if state_grad else None}
    before = {k: v.clone() for k, v in ins.items() if v is not None}
    outs = {"in_grad": torch.full((T, ns, max(p.n_in, 1)), SENTINEL, device="cuda"),
            "state0_grad": ins["state_grad"] if alias else torch.full((max(p.n_state, 1), ns), SENTINEL, device="cuda"),
            "param_grad": dev(ap) if p.n_param else torch.full((1, ns), SENTINEL, device="cuda"),
            "const_grad": dev(ac) if p.n_const else torch.full((1, ns), SENTINEL, device="cuda")}
    rows = {"in_grad": p.n_in, "state0_grad": p.n_state, "param_grad": p.n_param, "const_grad": p.n_const}
    untouched = {k: v.clone() for k, v in outs.items()}
    wsb = p.ring_grad_workspace_bytes(ns, T, checkpoint_rows) if fn == "fz_run_block_ring_grad" else p.grad_workspace_bytes(ns, T, checkpoint_rows)
    pad = 64                                                   # floats of sentinel on either side (the head stays 16-byte aligned)
    ws = torch.full((pad + (wsb + 3) // 4 + pad,), SENTINEL, device="cuda")
    a = CA.GradArgs()
    a.struct_size = ctypes.sizeof(CA.GradArgs)
    a.checkpoint_rows = checkpoint_rows
    for k, t in ins.items():
        setattr(a, k, t.data_ptr() if t is not None and t.numel() else None)
    for k, t in outs.items():
        setattr(a, k, t.data_ptr() if rows[k] and k not in leave_out else None)
    a.workspace, a.workspace_bytes = ws.data_ptr() + 4 * pad, wsb
    CA.check(getattr(CA.lib, fn)(p._h, ctypes.byref(a), ns, T, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    for k, t in before.items():
        if not (alias and k == "state_grad"):
            assert torch.equal(ins[k].view(torch.int32), t.view(torch.int32)), f"input {k} was written"
    assert bool((ws[:pad] == SENTINEL).all()) and bool((ws[pad + (wsb + 3) // 4:] == SENTINEL).all()), "the workspace's surroundings were written"
    for k in leave_out:
        if not (alias and k == "state0_grad"):
            assert torch.equal(outs[k], untouched[k]), f"{k} was left out and written"
    return {key: outs[b].cpu().numpy() for key, b in OUT.items() if rows[b] and b not in leave_out}


def check(p, got, want, what, keys=KEYS):
    for k in keys:
        if k not in got:
            continue
        g, w = got[k], want[k][:got[k].shape[0]] if k != "x" else want[k]
        assert same(g, w), f"{what}: {k} differs in {int((g.view(np.uint32) != np.asarray(w, F32).view(np.uint32)).sum())} of {g.size}"


def shapes(p, name):
    D, C = RG.DEEPEST[name], stride(p)
    rows = sorted(T for T in {1, D - 1, D, D + 1, C + 1, 2 * D + 3} if T <= 515)
    return [(65, T) for T in rows] + [(ns, D + 1) for ns in (1, 64, 257)]


@pytest.mark.parametrize("name", sorted(RG.RINGS))
def test_ring_adjoint_matches_reference_bitwise(F, name):
    p = prog(F, name)
    for ns, T in shapes(p, name):
        inputs, want = case(F, name, ns, T)
        check(p, launch(p, inputs), want, f"{name} ns={ns} T={T}")


@pytest.mark.parametrize("name", ["lds_ring_comb", "biquad_comb17"])
@pytest.mark.parametrize("c", [1, 32])
def test_bits_do_not_depend_on_the_checkpoint_stride(F, name, c):
    p = prog(F, name)
    D = RG.DEEPEST[name]
    for ns, T in ((65, D + 1), (257, 2 * D + 3)):
        inputs, want = case(F, name, ns, T)
        check(p, launch(p, inputs, checkpoint_rows=c), want, f"{name} C={c} ns={ns} T={T}")


@pytest.mark.parametrize("name", sorted(RG.RINGS))
def test_without_a_state_gradient_the_rings_start_from_plus_zero(F, name):
    p = prog(F, name)
    D = RG.DEEPEST[name]
    for T in (D - 1, D + 1):
        (x, s0, par, yb, sb, ap, ac), _ = case(F, name, 65, T)
        want = A.grad(p, x, yb, s0, par, None, ap, ac)
        check(p, launch(p, (x, s0, par, yb, sb, ap, ac), state_grad=False), want, f"{name} T={T} no state_grad")


@pytest.mark.parametrize("name", sorted(RG.RINGS))
def test_state0_grad_may_overwrite_state_grad(F, name):
    p = prog(F, name)
    for T in (RG.DEEPEST[name] - 1, RG.DEEPEST[name] + 1):
        inputs, want = case(F, name, 65, T)
        check(p, launch(p, inputs, alias=True), want, f"{name} T={T} in place")


@pytest.mark.parametrize("name", ["lds_ring_comb", "biquad_comb17", "two_in"])
def test_each_output_left_out_in_turn(F, name):
    p = prog(F, name)
    inputs, want = case(F, name, 65, RG.DEEPEST[name] + 1)
    for b in ("in_grad", "state0_grad", "param_grad", "const_grad"):
        got = launch(p, inputs, leave_out=(b,))
        assert {OUT[k] for k in got} == {v for k, v in OUT.items() if v != b and {"x": p.n_in, "state": p.n_state, "params": p.n_param, "consts": p.n_const}[k]}
        check(p, got, want, f"{name} without {b}")
    assert launch(p, inputs, leave_out=tuple(OUT.values())) == {}


@pytest.mark.parametrize("name", sorted(RG.RINGS))
def test_two_blocks_chain_like_one(F, name):
    """D - 2 rows, then D + 5: the backward of block 2, then of block 1 on the same accumulators with block 2's state adjoint -- the
    state between the blocks is run_block's -- gives the bits of one call over both"""
    p = prog(F, name)
    D = RG.DEEPEST[name]
    T1, T2 = D - 2, D + 5
    (x, s0, par, yb, sb, ap, ac), want = case(F, name, 65, T1 + T2)
    whole = launch(p, (x, s0, par, yb, sb, ap, ac))
    check(p, whole, want, f"{name} one call")
    _, s_mid = p.run_block(dev(x[:T1]), dev(s0), dev(par))
    s_mid = s_mid.cpu().numpy()
    second = launch(p, (x[T1:], s_mid, par, yb[T1:], sb, ap, ac))
    first = launch(p, (x[:T1], s0, par, yb[:T1], second["state"], second.get("params", ap), second.get("consts", ac)))
    chained = dict(first, x=np.concatenate([first["x"], second["x"]]))
    check(p, chained, whole, f"{name} chained")


@pytest.mark.parametrize("name", ["df1_cascade6", "moog_ladder", "rules"])
def test_for_a_graph_without_a_ring_it_is_run_block_grad(F, name):
    import test_grad_gpu as TG
    p = prog(F, name)
    inputs = TG.make_inputs(p, name, 257, 37, 3)
    ring, plain = launch(p, inputs), launch(p, inputs, fn="fz_run_block_grad")
    assert set(ring) == set(plain)
    for k in ring:
        assert same(ring[k], plain[k]), k
    x, s0, par, yb, sb, ap, ac = inputs
    accum = {k: dev(a) for k, a, n in (("params", ap, p.n_param), ("consts", ac, p.n_const)) if n}
    r = p.run_block_ring_grad(dev(x), dev(yb), dev(s0), dev(par), dev(sb), accum=accum)
    torch.cuda.synchronize()
    for k in ring:
        assert same(r[k].cpu().numpy()[:ring[k].shape[0]], ring[k]), k


def test_run_block_ring_grad_returns_the_dict_of_run_block_grad(F):
    name = "biquad_comb17"
    p = prog(F, name)
    (x, s0, par, yb, sb, ap, ac), want = case(F, name, 257, 18)
    r = p.run_block_ring_grad(dev(x), dev(yb), dev(s0), dev(par), dev(sb), accum={"params": dev(ap), "consts": dev(ac)})
    torch.cuda.synchronize()
    assert set(r) == set(KEYS)
    check(p, {k: v.cpu().numpy() for k, v in r.items()}, want, "python call")
    r = p.run_block_ring_grad(dev(x), dev(yb), dev(s0), dev(par), dev(sb), want=("state",))
    assert set(r) == {"state"} and same(r["state"].cpu().numpy(), want["state"])
    with pytest.raises(F.FlowzError):
        p.run_block_grad(dev(x), dev(yb), dev(s0), dev(par), dev(sb))


def test_autograd_run_rings_matches_float64_autograd(F):
    """fb9 through torch.autograd against float64 autograd of adjoint_ref.torch_forward: the tolerance of test_ring_grad_host.py"""
    from zignal_amd import autograd as AG
    name = "fb9"
    p = prog(F, name)
    ns, T = 130, 30
    x, s0, par, yb, sb, _, _ = RG.inputs(p, ns, T, 31)
    xt, st = dev(x).requires_grad_(), dev(s0).requires_grad_()
    ct = torch.tensor(p.consts(), dtype=torch.float32).requires_grad_()
    before = st.detach().clone()
    y, s = AG.run_rings(p, xt, st, None, ct)
    y_plain, s_plain = p.run_block(dev(x), dev(s0))
    assert torch.equal(y.detach().view(torch.int32), y_plain.view(torch.int32)) and torch.equal(s.detach().view(torch.int32), s_plain.view(torch.int32))
    assert torch.equal(st.detach(), before)                             # the caller's state is not advanced
    ((y * dev(yb)).sum() + (s * dev(sb)).sum()).backward()
    want = A.torch_grad(p, x, yb, s0, par, sb)
    assert A.rel_err(xt.grad.cpu().numpy(), want["x"]) <= 1e-4
    assert A.rel_err(st.grad.cpu().numpy(), want["state"]) <= 1e-4
    assert A.rel_err(ct.grad.numpy(), want["consts"].sum(1)) <= 1e-4
    # and bit for bit what the call under it gives, the coefficient adjoints summed over the streams in float64
    r = launch(p, (x, s0, par, yb, sb, np.zeros((0, ns), F32), np.zeros((p.n_const, ns), F32)))
    assert same(xt.grad.cpu().numpy(), r["x"]) and same(st.grad.cpu().numpy(), r["state"])
    assert same(ct.grad.numpy(), r["consts"].astype(np.float64).sum(1).astype(F32))
    with pytest.raises(F.FlowzError):
        AG.run(p, xt, st, None, ct)
