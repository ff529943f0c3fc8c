"""The ring adjoint kernel on the MI355X (fz_run_block_ring_grad: graphs with delay lines deeper than 8 samples): every output bit for
bit against tests/adjoint_ref.py, at the row counts around each line's depth and the stream counts around a wave and a workgroup;
checkpoint strides, a missing state gradient, the state gradient overwritten in place, every output left out in turn, two chained
blocks of which the first is shorter than the line, the inputs and the workspace's surroundings untouched; autograd over it.

Every launch goes through the C ABI with a workspace of exactly the queried bytes inside a larger buffer of sentinels, and checks
afterwards that the sentinels and every input kept their bits."""
import numpy as np
import pytest

import adjoint_ref as A
import grad_graphs as GG
import grad_harness as H
import ring_grad_graphs as RG
from grad_harness import F32, OUT, dev, gpu_flowz, make_inputs, same

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

KEYS = H.GRAD_KEYS
OUT = {key: OUT[key] for key in KEYS}


@pytest.fixture(scope="module")
def F():
    return gpu_flowz()


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


def launch(p, inputs, checkpoint_rows=0, state_grad=True, alias=False, leave_out=(), ring=True):
    """one call of fz_run_block_ring_grad (ring=False: fz_run_block_grad) through grad_harness.launch"""
    return H.launch(p, inputs, ring=ring, c=checkpoint_rows, state_grad=state_grad, alias=alias, leave_out=leave_out)


def check(p, got, want, what, keys=KEYS):
    H.check(p, got, want, what, keys)


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
    p = prog(F, name)
    inputs = make_inputs(p, name, 257, 37, 3)
    ring, plain = launch(p, inputs), launch(p, inputs, ring=False)
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
