"""The ring adjoint kernels for stream-major buffers on the MI355X (fz_run_block_ring_grad_stream_major,
fz_run_block_ring_loss_grad_stream_major): every output bit for bit against the restatements (tests/adjoint_ref.py,
tests/loss_grad_ref.py) on the transposed arrays AND against the time-major ring kernels on the transposed buffers -- the layout does
not change a bit --, around every boundary the kernels have (wave, workgroup, checkpoint chunk, LDS patch, the depth of the line);
windows of larger buffers, two chained windows, checkpoint strides, a missing state gradient, the state gradient overwritten in place,
every output left out in turn, accumulators, repeatability, and autograd.run_rings / mse_rings (stream_major=True).

Every launch of launch() goes through the C ABI with a workspace of exactly the queried bytes and every output inside a larger buffer
of sentinels; in_grad and out are whole [n_streams][rows_total][wire] buffers of sentinels of which only the window may change.
Afterwards the sentinels and every input kept their bits."""
import numpy as np
import pytest

import adjoint_ref as A
import grad_harness as H
import ring_grad_graphs as RG
import ring_loss_graphs as RL
import ring_sm_graphs as RS
from grad_harness import F32, OUT, dev, gpu_flowz, outside_keeps_sentinel, same, to_sm, up4

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

K = RL.K
KEYS = H.GRAD_KEYS
LOSS_KEYS = H.LOSS_KEYS


@pytest.fixture(scope="module")
def F():
    return gpu_flowz()


_plain = {}


def plain_case(name, ns, T, seed=0):
    """the draw of a plain case and adjoint_ref's answer to it, computed once and never modified"""
    key = (name, ns, T, seed)
    if key not in _plain:
        p = RS.prog(name)
        d = RG.inputs(p, ns, T, 1000 * seed + 7 * ns + T)
        want = A.grad(p, *[d[i] for i in (0, 3, 1, 2, 4, 5, 6)])
        for a in (*d, *want.values()):
            if a is not None:
                a.setflags(write=False)
        _plain[key] = (d, want)
    return _plain[key]


def case(name, ns, T, loss):
    return RL.case(name, ns, T) if loss else plain_case(name, ns, T)


def geometry(p, loss=False, c=0):
    """(C, R, block): the symbol names them"""
    return RS.symbol_geometry((p.ring_loss_grad_kernel_symbol if loss else p.ring_grad_kernel_symbol)(c, stream_major=True))


def launch(p, d, loss, c=0, rows=None, row0=0, state_grad=True, alias=False, leave_out=(), frames=None, k=K):
    """one call of fz_run_block_ring_grad_stream_major / fz_run_block_ring_loss_grad_stream_major through grad_harness.launch: the
    time-major draw d in stream-major buffers of `rows` rows with the block at [row0, row0 + T)"""
    return H.launch(p, d, ring=True, loss=loss, window=(rows, row0), c=c, state_grad=state_grad, alias=alias, leave_out=leave_out, k=k,
                    frames=frames)


def time_major(p, d, loss, c=0, state_grad=True, k=K):
    """the time-major ring backward of the same draw, through the Python call"""
    x, s0, par, yt, sb, ap, ac = d[:7]
    accum = {key: dev(v) for key, v, n in (("params", ap, p.n_param), ("consts", ac, p.n_const)) if n}
    sg = dev(sb) if state_grad and p.n_state else None
    if loss:
        accum["loss"] = dev(d[7])
        r = p.run_block_ring_loss_grad(dev(x), dev(yt), dev(s0), dev(par), sg, grad_scale=k, accum=accum, checkpoint_rows=c)
    else:
        r = p.run_block_ring_grad(dev(x), dev(yt), dev(s0), dev(par), sg, accum=accum, checkpoint_rows=c)
    torch.cuda.synchronize()
    return {key: v.cpu().numpy() for key, v in r.items()}


def check(p, got, want, what, keys=LOSS_KEYS):
    H.check(p, got, want, what, keys)


def present(p, loss):
    n = {"x": p.n_in, "state": p.n_state, "params": p.n_param, "consts": p.n_const}
    return {key for key in (LOSS_KEYS if loss else KEYS) if n.get(key, 1)}


def shapes(name, loss):
    """(ns, D + 1) around a wave and a workgroup, (65, T) around the stride, the depth and the patch"""
    p = RS.prog(name)
    C, R, _ = geometry(p, loss)
    D = RS.DEEPEST[name]
    Ts = sorted({1, max(C - 1, 1), C + 1, D - 1, D, R - 1, R, R + 1, 2 * D + 3, 2 * R + 3})
    return [(ns, D + 1) for ns in (1, 63, 64, 65, 257)] + [(65, T) for T in Ts]


def parity(name, loss):
    p = RS.prog(name)
    for ns, T in shapes(name, loss):
        d, want = case(name, ns, T, loss)
        got = launch(p, d, loss)
        what = f"{name} ns={ns} T={T} {geometry(p, loss)}"
        assert {key for key in got if not key.endswith("_buffer")} == present(p, loss), what
        check(p, got, want, what + " against the restatement")
        check(p, got, time_major(p, d, loss), what + " against the time-major ring kernel")
        assert outside_keeps_sentinel(got["x_buffer"], 0, T), what + ": rows of in_grad behind the window were written"
        if loss:
            assert outside_keeps_sentinel(got["out_buffer"], 0, T), what + ": rows of out behind the window were written"


@pytest.mark.parametrize("name", sorted(RS.RINGS))
def test_stream_major_ring_adjoint_matches_restatement_and_time_major_bitwise(F, name):
    parity(name, False)


@pytest.mark.parametrize("name", sorted(RS.GRAPHS))
def test_stream_major_ring_loss_adjoint_matches_restatement_and_time_major_bitwise(F, name):
    parity(name, True)


@pytest.mark.parametrize("loss", [False, True])
@pytest.mark.parametrize("name", sorted(RS.RINGS))
def test_a_window_equals_the_time_major_ring_backward_of_the_slice(F, name, loss):
    p = RS.prog(name)
    _, R, _ = geometry(p, loss)
    D = RS.DEEPEST[name]
    for ns, row0, T, tail in ((130, 4, R + 5, 9), (65, 2 * R, D + 3, 0), (130, 8, 3, 1)):
        rows = up4(row0 + T + tail)
        d, want = case(name, ns, T, loss)
        got = launch(p, d, loss, rows=rows, row0=row0)
        what = f"{name} window [{row0}, {row0 + T}) of {rows}"
        check(p, got, time_major(p, d, loss), what)
        check(p, got, want, what + " against the restatement")
        assert outside_keeps_sentinel(got["x_buffer"], row0, T), what + ": rows of in_grad outside the window were written"
        if loss:
            assert outside_keeps_sentinel(got["out_buffer"], row0, T), what + ": rows of out outside the window were written"


@pytest.mark.parametrize("loss", [False, True])
@pytest.mark.parametrize("name", sorted(RS.RINGS))
def test_two_windows_of_one_buffer_chain_like_one(F, name, loss):
    """up4(D - 2) rows, then D + 5: the backward of the second window, then of the first on the same accumulators with the second's
    state adjoint -- the state between them is run_block_stream_major's --, both writing into ONE in_grad (and out) buffer, give the
    bits of one window over both"""
    p = RS.prog(name)
    T1, T2 = RS.chain_rows(name)
    ns, rows = 65, up4(T1 + T2)
    d, want = case(name, ns, T1 + T2, loss)
    x, s0, par, yt, sb, ap, ac = d[:7]
    whole = launch(p, d, loss, rows=rows)
    check(p, whole, want, f"{name} one window")
    _, s_mid = p.run_block_stream_major(dev(to_sm(x, rows)), dev(s0), dev(par), row0=0, n_samples=T1)
    s_mid = s_mid.cpu().numpy()
    frames = {}
    second = launch(p, (x[T1:], s_mid, par, yt[T1:], sb, ap, ac) + tuple(d[7:]), loss, rows=rows, row0=T1, frames=frames)
    first = launch(p, (x[:T1], s0, par, yt[:T1], second["state"], second.get("params", ap), second.get("consts", ac)) + ((second["loss"],) if loss else ()),
                   loss, rows=rows, row0=0, frames=frames)
    assert same(first["x_buffer"], whole["x_buffer"]), f"{name}: the in_grad buffer filled by two windows differs"
    if loss:
        assert same(first["out_buffer"], whole["out_buffer"]), f"{name}: the out buffer filled by two windows differs"
    check(p, first, whole, f"{name} chained windows", keys=("state", "params", "consts", "loss"))


@pytest.mark.parametrize("loss", [False, True])
@pytest.mark.parametrize("name", RS.STRIDE_GRAPHS)
def test_bits_do_not_depend_on_the_checkpoint_stride(F, name, loss):
    p = RS.prog(name)
    D = RS.DEEPEST[name]
    for T in (D + 1, 2 * D + 3):
        d, want = case(name, 65, T, loss)
        for c in RS.STRIDES[1:]:
            assert geometry(p, loss, c)[0] == c
            check(p, launch(p, d, loss, c=c), want, f"{name} T={T} checkpoint_rows={c}")


@pytest.mark.parametrize("loss", [False, True])
@pytest.mark.parametrize("name", sorted(RS.RINGS))
def test_without_a_state_gradient_and_with_it_overwritten_in_place(F, name, loss):
    p = RS.prog(name)
    T = RS.DEEPEST[name] + 1
    d, want = case(name, 65, T, loss)
    check(p, launch(p, d, loss, state_grad=False), time_major(p, d, loss, state_grad=False), f"{name} no state_grad")
    got = launch(p, d, loss, alias=True)
    assert "state" in got
    check(p, got, want, f"{name} in place")


@pytest.mark.parametrize("loss", [False, True])
@pytest.mark.parametrize("name", ["lds_ring_comb", "biquad_comb17", "two_in"])
def test_each_output_left_out_in_turn(F, name, loss):
    p = RS.prog(name)
    d, want = case(name, 65, RS.DEEPEST[name] + 1, loss)
    keys = present(p, loss)
    for key in sorted(keys):
        got = launch(p, d, loss, leave_out=(OUT[key],))
        assert {g for g in got if not g.endswith("_buffer")} == keys - {key}
        check(p, got, want, f"{name} without {OUT[key]}")
    assert launch(p, d, loss, leave_out=tuple(OUT.values())) == {}


@pytest.mark.parametrize("loss", [False, True])
def test_accumulators_are_added_to_and_two_launches_agree(F, loss):
    """the same block from pre-filled accumulators (the cases') and from zero: both the restatement's bits, and they differ; the same
    launch twice gives the same bits"""
    name = "biquad_comb17"
    p = RS.prog(name)
    d, want = case(name, 65, RS.DEEPEST[name] + 1, loss)
    got = launch(p, d, loss)
    check(p, got, want, f"{name} pre-filled")
    again = launch(p, d, loss)
    for key in got:
        assert same(got[key], again[key]), f"{name}: {key} differs between two launches"
    zero = tuple(d[:5]) + tuple(np.zeros_like(a) for a in d[5:])
    got0 = launch(p, zero, loss)
    check(p, got0, time_major(p, zero, loss), f"{name} from zero")
    assert not same(got0["params"], got["params"]) and not same(got0["consts"], got["consts"])


# ---- autograd ---------------------------------------------------------------------------------------------------------------------------
def t_sm(a):
    """time-major numpy [T][ns][w] -> a stream-major device tensor [ns][T][w] (T itself on the float4 grid is not needed: the tensor is the window)"""
    return dev(np.ascontiguousarray(a.transpose(1, 0, 2)))


@pytest.mark.parametrize("name", RS.AUTOGRAD_GRAPHS)
def test_autograd_stream_major_has_the_bits_of_time_major(F, name):
    from zignal_amd import autograd as AG
    p = RS.prog(name)
    ns, T = 130, up4(2 * RS.DEEPEST[name] + 3)
    x, s0, par, tg, _, _, _, _ = RL.draw(p, ns, T, 31)
    w = np.random.default_rng(5).standard_normal((T, ns, p.n_out)).astype(F32)

    def grads(stream_major, fused):
        xt = (t_sm(x) if stream_major else dev(x)).requires_grad_()
        st = dev(s0).requires_grad_()
        pt = dev(par).requires_grad_() if p.n_param else None
        ct = torch.tensor(p.consts(), dtype=torch.float32).requires_grad_()
        tgt, wt = (t_sm(tg), t_sm(w)) if stream_major else (dev(tg), dev(w))
        if fused:
            loss = AG.mse_rings(p, xt, tgt, st, pt, ct, stream_major=stream_major)
        else:
            y, _ = AG.run_rings(p, xt, st, pt, ct, stream_major=stream_major)
            assert tuple(y.shape) == ((ns, T, p.n_out) if stream_major else (T, ns, p.n_out))
            loss = (y * wt).sum()
        loss.backward()
        gx = xt.grad.cpu().numpy()
        return (loss.item(), gx.transpose(1, 0, 2) if stream_major else gx, st.grad.cpu().numpy(), pt.grad.cpu().numpy() if pt is not None else None,
                ct.grad.numpy())

    for fused in (False, True):
        sm, tm = grads(True, fused), grads(False, fused)
        assert same(sm[1], tm[1]) and same(sm[2], tm[2]), f"{name} fused={fused}: x or state"
        if p.n_param:
            assert same(sm[3], tm[3]), f"{name} fused={fused}: params"
        assert np.allclose(sm[4], tm[4], rtol=1e-6, atol=1e-6 * float(np.abs(tm[4]).max(initial=0.0))), f"{name} fused={fused}: consts"
        if fused:
            mse, _, g64 = RL.mse_float64(p, x, tg, s0, par)
            assert abs(sm[0] - mse) <= 1e-4 * mse, (sm[0], mse)
            assert A.rel_err(sm[1], g64["x"]) <= 1e-4 and A.rel_err(sm[2], g64["state"]) <= 1e-4
            if p.n_param:
                assert A.rel_err(sm[3], g64["params"]) <= 1e-4
            assert A.rel_err(sm[4], g64["consts"].sum(1)) <= 1e-4
        else:
            g64 = A.torch_grad(p, x, w, s0, par, None, dtype=torch.float64)
            assert A.rel_err(sm[1], g64["x"]) <= 1e-4 and A.rel_err(sm[2], g64["state"]) <= 1e-4
            if p.n_param:
                assert A.rel_err(sm[3], g64["params"]) <= 1e-4
            assert A.rel_err(sm[4], g64["consts"].sum(1)) <= 1e-4


def test_autograd_takes_batch_time_tensors_for_one_wire(F):
    from zignal_amd import autograd as AG
    name = "lds_ring_comb"
    p = RS.prog(name)
    assert p.n_in == 1 and p.n_out == 1
    ns, T = 130, up4(2 * RS.DEEPEST[name] + 3)
    x, s0, par, tg, _, _, _, _ = RL.draw(p, ns, T, 31)
    x2, x3 = t_sm(x)[..., 0].contiguous().requires_grad_(), t_sm(x).requires_grad_()
    assert tuple(x2.shape) == (ns, T)
    l2 = AG.mse_rings(p, x2, t_sm(tg)[..., 0].contiguous(), dev(s0), stream_major=True)
    l3 = AG.mse_rings(p, x3, t_sm(tg), dev(s0), stream_major=True)
    l2.backward()
    l3.backward()
    assert tuple(x2.grad.shape) == (ns, T) and same(x2.grad.cpu().numpy(), x3.grad.cpu().numpy()[..., 0]) and l2.item() == l3.item()
    y2, _ = AG.run_rings(p, x2.detach().requires_grad_(), dev(s0), stream_major=True)
    assert tuple(y2.shape) == (ns, T, 1)
    with pytest.raises(F.FlowzError):
        AG.run(p, x3, dev(s0), stream_major=True)
