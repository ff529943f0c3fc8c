"""The far adjoint kernels for stream-major buffers on the MI355X (fz_run_block_far_grad_stream_major,
fz_run_block_far_loss_grad_stream_major: graphs with delay lines deeper than 256 samples, whose rings live in HBM, on a [batch, time]
tensor as it lies): every output bit for bit against the restatements (tests/far_grad_ref.py, tests/loss_grad_ref.py through it) on
the transposed arrays AND against the time-major far kernels on the transposed buffers, with a phase p0 = D - 3 that makes the ring
wrap inside the block -- around every boundary the kernels have (wave, workgroup, checkpoint chunk, LDS patch, the depth of the line);
windows of larger buffers, two chained windows, checkpoint strides (and with them both paths of sweep 2), a missing state gradient,
the state gradient overwritten in place, every output left out in turn, accumulators, repeatability, the loss call, the Python front
doors and autograd.run_far / mse_far (stream_major=True).

Every launch of launch() goes through the C ABI (grad_harness.launch) with a workspace of exactly the queried bytes and every output
inside a larger buffer of sentinels; in_grad and out are whole [n_streams][rows_total][wire] buffers of sentinels of which only the
window may change.  Afterwards the sentinels and every input kept their bits.  The time-major side and the cases (inputs and
far_grad_ref's answer, computed once) are those of tests/test_far_grad_gpu.py."""
import numpy as np
import pytest

import adjoint_ref as A
import far_grad_ref as FR
import far_sm_graphs as FS
import grad_harness as H
import test_far_grad_gpu as TM
from grad_harness import F32, OUT, dev, gpu_flowz, outside_keeps_sentinel, same, to_sm, up4

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

K = H.K
KEYS, LOSS_KEYS = H.GRAD_KEYS, H.LOSS_KEYS


@pytest.fixture(scope="module")
def F():
    return gpu_flowz()


def prog(F, name):
    return TM.prog(F, name)


def case(F, name, ns, T, loss=False, state_grad=True):
    """the case of test_far_grad_gpu.py at the phase p0 = D - 3: the ring wraps inside the block"""
    return TM.case(F, name, ns, T, p0=FS.DEEPEST[name] - 3, loss=loss, state_grad=state_grad)


def geometry(p, loss=False, c=0):
    """(C, R, block): the symbol names them"""
    return FS.symbol_geometry((p.far_loss_grad_kernel_symbol if loss else p.far_grad_kernel_symbol)(c, stream_major=True))


def launch(p, d, loss=False, c=0, rows=None, row0=0, state_grad=True, alias=False, leave_out=(), frames=None):
    """one call of fz_run_block_far_grad_stream_major / fz_run_block_far_loss_grad_stream_major (grad_scale = K) through
    grad_harness.launch: the time-major draw d in stream-major buffers of `rows` rows with the block at [row0, row0 + T)"""
    with FS.far_entry_points():
        return H.launch(FS.AsRingFamily(p), d, ring=True, loss=loss, window=(rows, row0), c=c, state_grad=state_grad, alias=alias,
                        leave_out=leave_out, k=K, frames=frames)


def time_major(p, d, loss=False, c=0, state_grad=True):
    """the time-major far call on the same draw, through the C ABI"""
    return TM.launch(p, d, loss=loss, c=c, state_grad=state_grad)


def present(p, loss):
    n = {"x": p.n_in, "state": p.n_state, "params": p.n_param, "consts": p.n_const}
    return {key for key in (LOSS_KEYS if loss else KEYS) if n.get(key, 1)}


def check(p, got, want, what, keys=LOSS_KEYS):
    H.check(p, got, want, what, keys)


def parity(F, name, ns, T, loss=False, c=0):
    """one shape: the stream-major call against the restatement and against the time-major call; nothing behind the window written"""
    p = prog(F, name)
    d, want = case(F, name, ns, T, loss)
    got = launch(p, d, loss, c=c)
    what = f"{name} ns={ns} T={T} loss={loss} {geometry(p, loss, c)}"
    assert {key for key in got if not key.endswith("_buffer")} == present(p, loss), what
    check(p, got, want, what + " against the restatement")
    check(p, got, time_major(p, d, loss, c=c), what + " against the time-major far kernel")
    assert outside_keeps_sentinel(got["x_buffer"], 0, T), what + ": rows of in_grad behind the window were written"
    if loss:
        assert outside_keeps_sentinel(got["out_buffer"], 0, T), what + ": rows of out behind the window were written"
    return got


def streams_of(name):
    return (1, 63, 64, 65) if name == "far1031" else (1, 63, 64, 65, 257)


def rows_of(p, name):
    """around the stride, the patch and the depth; far1031 within the restatement's reach"""
    C, R, _ = geometry(p)
    D = FS.DEEPEST[name]
    return sorted(T for T in {1, max(C - 1, 1), C + 1, R - 1, R, R + 1, D - 1, D, D + 1, 2 * D + 3} if name != "far1031" or T <= TM.FG.MAX_ROWS)


@pytest.mark.parametrize("name", sorted(FS.FARS))
def test_stream_counts_around_a_wave_and_a_workgroup(F, name):
    for ns in streams_of(name):
        parity(F, name, ns, FS.DEEPEST[name] + 1)


@pytest.mark.parametrize("name", sorted(FS.FARS))
def test_row_counts_around_the_stride_the_patch_and_the_depth(F, name):
    p = prog(F, name)
    D = FS.DEEPEST[name]
    inputs, _ = case(F, name, 65, D + 1)
    assert all(inputs[1][pr, 0] == (D - 3) % d for _, d, pr in TM.FG.far_rows(p))       # (the phase the cases carry)
    for T in rows_of(p, name):
        parity(F, name, 65, T)


@pytest.mark.parametrize("loss", [False, True])
@pytest.mark.parametrize("name", sorted(FS.FARS))
def test_a_window_equals_the_time_major_far_backward_of_the_slice(F, name, loss):
    p = prog(F, name)
    _, R, _ = geometry(p, loss)
    D = FS.DEEPEST[name]
    wide = 65 if name == "far1031" else 130
    for ns, row0, T, tail in ((wide, 4, R + 5, 9), (65, 2 * R, D + 3, 0), (wide, 8, 3, 1)):
        rows = up4(row0 + T + tail)
        d, want = case(F, name, ns, T, loss)
        got = launch(p, d, loss, rows=rows, row0=row0)
        what = f"{name} window [{row0}, {row0 + T}) of {rows}"
        check(p, got, time_major(p, d, loss), what)
        check(p, got, want, what + " against the restatement")
        assert outside_keeps_sentinel(got["x_buffer"], row0, T), what + ": rows of in_grad outside the window were written"
        if loss:
            assert outside_keeps_sentinel(got["out_buffer"], row0, T), what + ": rows of out outside the window were written"


@pytest.mark.parametrize("loss", [False, True])
@pytest.mark.parametrize("name", sorted(FS.FARS))
def test_two_windows_of_one_buffer_chain_like_one(F, name, loss):
    """up4(D - 2) rows, then D + 5: the backward of the second window, then of the first on the same accumulators with the second's
    state adjoint as it is -- the state between them is the time-major run_block's, phase row included --, both writing into ONE
    in_grad (and out) buffer, give the bits of one window over both"""
    p = prog(F, name)
    D = FS.DEEPEST[name]
    T1, T2 = FS.chain_rows(name)
    ns, rows = 65, up4(T1 + T2)
    if name == "far1031":                                         # (2 D + 3 rows are beyond the restatement's reach: one launch stands for it)
        d = TM.FG.inputs(p, ns, T1 + T2, 5, p0=D - 3)
        if loss:
            d = d + (np.random.default_rng(9).standard_normal(ns).astype(F32),)
    else:
        d, want = case(F, name, ns, T1 + T2, loss)
    x, s0, par, yt, sb, ap, ac = d[:7]
    whole = launch(p, d, loss, rows=rows)
    if name != "far1031":
        check(p, whole, want, f"{name} one window")
    _, s_mid = p.run_block(dev(x[:T1]), dev(s0), dev(par))
    s_mid = s_mid.cpu().numpy()
    assert all(s_mid[pr, 0] == (D - 3 + T1) % d_ for _, d_, pr in TM.FG.far_rows(p))
    frames = {}
    second = launch(p, (x[T1:], s_mid, par, yt[T1:], sb, ap, ac) + tuple(d[7:]), loss, rows=rows, row0=T1, frames=frames)
    first = launch(p, (x[:T1], s0, par, yt[:T1], second["state"], second.get("params", ap), second.get("consts", ac)) + ((second["loss"],) if loss else ()),
                   loss, rows=rows, row0=0, frames=frames)
    assert same(first["x_buffer"], whole["x_buffer"]), f"{name}: the in_grad buffer filled by two windows differs"
    if loss:
        assert same(first["out_buffer"], whole["out_buffer"]), f"{name}: the out buffer filled by two windows differs"
    check(p, first, whole, f"{name} chained windows", keys=("state", "params", "consts", "loss"))


@pytest.mark.parametrize("name", FS.STRIDES)
@pytest.mark.parametrize("c", [1, 32])
def test_bits_do_not_depend_on_the_checkpoint_stride(F, name, c):
    """C = 1 takes the fast path on every graph, C = 32 the per-row path on far_tap1: the two paths are held to the same bits"""
    p = prog(F, name)
    D = FS.DEEPEST[name]
    assert geometry(p, False, c)[0] == c
    for ns, T in ((65, D + 1), (63, 2 * D + 3)):
        parity(F, name, ns, T, c=c)


@pytest.mark.parametrize("loss", [False, True])
@pytest.mark.parametrize("name", sorted(FS.FARS))
def test_without_a_state_gradient_and_with_it_overwritten_in_place(F, name, loss):
    p = prog(F, name)
    for T in (FS.DEEPEST[name] - 1, FS.DEEPEST[name] + 1):
        d, want = case(F, name, 65, T, loss)
        d0, want0 = case(F, name, 65, T, loss, state_grad=False)
        got0 = launch(p, d0, loss, state_grad=False)
        check(p, got0, want0, f"{name} T={T} no state_grad")
        check(p, got0, time_major(p, d0, loss, state_grad=False), f"{name} T={T} no state_grad against the time-major far kernel")
        got = launch(p, d, loss, alias=True)
        assert "state" in got
        check(p, got, want, f"{name} T={T} in place")


@pytest.mark.parametrize("loss", [False, True])
@pytest.mark.parametrize("name", ["far_comb", "far_mixed", "far_two_in"])
def test_each_output_left_out_in_turn(F, name, loss):
    p = prog(F, name)
    d, want = case(F, name, 65, FS.DEEPEST[name] + 1, loss)
    keys = present(p, loss)
    for key in sorted(keys):
        got = launch(p, d, loss, leave_out=(OUT[key],))
        assert {g for g in got if not g.endswith("_buffer")} == keys - {key}
        check(p, got, want, f"{name} without {OUT[key]}")
    assert launch(p, d, loss, leave_out=tuple(OUT.values())) == {}


@pytest.mark.parametrize("loss", [False, True])
def test_accumulators_are_added_to_and_two_launches_agree(F, loss):
    """the same block from pre-filled accumulators (the cases') and from zero: both the reference's bits, and they differ; the same
    launch twice gives the same bits"""
    name = "far_mixed"
    p = prog(F, name)
    d, want = case(F, name, 65, FS.DEEPEST[name] + 1, loss)
    got = launch(p, d, loss)
    check(p, got, want, f"{name} pre-filled")
    again = launch(p, d, loss)
    for key in got:
        assert same(got[key], again[key]), f"{name}: {key} differs between two launches"
    zero = tuple(d[:5]) + tuple(np.zeros_like(a) for a in d[5:])
    got0 = launch(p, zero, loss)
    check(p, got0, time_major(p, zero, loss), f"{name} from zero")
    assert not same(got0["params"], got["params"]) and not same(got0["consts"], got["consts"])


@pytest.mark.parametrize("name", sorted(FS.FARS))
def test_loss_call(F, name):
    """fz_run_block_far_loss_grad_stream_major against loss_grad_ref at grad_harness.K (through far_grad_ref) and the time-major loss
    call, against the plain new call given the same dL/dy, and `out` / `loss` against the time-major run_block's bits"""
    p = prog(F, name)
    C, R, _ = geometry(p, True)
    D = FS.DEEPEST[name]
    for T in (D + 1, C + 1, R + 1):
        got = parity(F, name, 65, T, loss=True)
        (x, s0, par, tg, sb, ap, ac, al), _ = case(F, name, 65, T, True)
        if T == D + 1:
            y, _ = p.run_block(dev(x), dev(s0), dev(par))
            y = y.cpu().numpy()
            assert same(got["out"], y) and same(got["out_buffer"][:, :T], y.transpose(1, 0, 2))
        else:
            y = got["out"]
        with np.errstate(all="ignore"):
            e, ls = y - tg, al.copy()
            for t in range(T - 1, -1, -1):
                for j in range(p.n_out):
                    ls = ls + e[t, :, j] * e[t, :, j]
        assert same(got["loss"], ls)
        plain = launch(p, (x, s0, par, e * F32(K), sb, ap, ac))
        check(p, got, plain, f"{name} loss against the plain call", KEYS)
    # `out` and `loss` left out: the gradients do not change
    d, want = case(F, name, 65, D + 1, True)
    got = launch(p, d, True, leave_out=("loss", "out"))
    assert "loss" not in got and "out" not in got
    check(p, got, want, f"{name} loss without loss and out", KEYS)


def test_the_python_calls_return_the_dicts_of_the_ring_calls(F):
    name = "far_mixed"
    p = prog(F, name)
    T, row0 = FS.DEEPEST[name] + 1, 8
    rows = up4(row0 + T + 5)
    sm = lambda a: dev(to_sm(a, rows, row0, H.FILL))                  # noqa: E731
    full = lambda w: torch.full((257, rows, w), float(H.SENTINEL), device="cuda")   # noqa: E731
    (x, s0, par, yb, sb, ap, ac), want = case(F, name, 257, T)
    r = p.run_block_far_grad_stream_major(sm(x), sm(yb), dev(s0), dev(par), dev(sb), accum={"params": dev(ap), "consts": dev(ac)},
                                          row0=row0, n_samples=T, in_grad=full(p.n_in))
    assert set(r) == set(KEYS)
    got = H.to_numpy(r, (row0, T))
    check(p, got, want, "python call", KEYS)
    assert outside_keeps_sentinel(got["x_buffer"], row0, T)
    d = x, s0, par, tg, sb, ap, ac, al = case(F, name, 257, T, True)[0]
    lwant = case(F, name, 257, T, True)[1]
    r = p.run_block_far_loss_grad_stream_major(sm(x), sm(tg), dev(s0), dev(par), dev(sb), grad_scale=K, accum={"params": dev(ap), "consts": dev(ac), "loss": dev(al)},
                                               row0=row0, n_samples=T, in_grad=full(p.n_in), out=full(p.n_out))
    assert set(r) == set(LOSS_KEYS) and len(d) == 8
    got = H.to_numpy(r, (row0, T))
    check(p, got, lwant, "python loss call", LOSS_KEYS)
    assert outside_keeps_sentinel(got["x_buffer"], row0, T) and outside_keeps_sentinel(got["out_buffer"], row0, T)
    for refused in (p.run_block_ring_grad_stream_major, p.run_block_grad_stream_major):
        with pytest.raises(F.FlowzError):
            refused(sm(x), sm(tg), dev(s0), dev(par), dev(sb), row0=row0, n_samples=T)
    with pytest.raises(F.FlowzError):                                  # the forward has no stream-major body for rings in HBM
        p.run_block_stream_major(sm(x), dev(s0), dev(par), row0=row0, n_samples=T)


# ---- autograd ---------------------------------------------------------------------------------------------------------------------------
def t_sm(a):
    """time-major numpy [T][ns][w] -> a stream-major device tensor [ns][T][w]: the tensor is the window"""
    return dev(np.ascontiguousarray(a.transpose(1, 0, 2)))


def test_autograd_stream_major_has_the_bits_of_time_major_and_matches_float64(F):
    """autograd.run_far and mse_far with stream_major=True: bit for bit their time-major selves on the transposed tensors (the
    coefficient adjoints, summed over the streams in float64, included), and within 1e-4 of float64 autograd of
    adjoint_ref.torch_forward, the tolerance of the far tests"""
    from zignal_amd import autograd as AG
    name, ns, T = FS.AUTOGRAD
    p = prog(F, name)
    far = TM.FG.far_rows(p)
    D = FS.DEEPEST[name]
    x, s0, par, yb, sb, _, _ = TM.FG.inputs(p, ns, T, 31)
    ages = lambda a, ph: FR.convert(a, [ph], far)[:D]                   # noqa: E731  (the line rows, as adjoint_ref keeps them)

    def grads(stream_major, fused):
        xt = (t_sm(x) if stream_major else dev(x)).requires_grad_()
        st = dev(s0).requires_grad_()
        ct = torch.tensor(p.consts(), dtype=torch.float32).requires_grad_()
        wt = t_sm(yb) if stream_major else dev(yb)
        if fused:
            loss = AG.mse_far(p, xt, wt, st, None, ct, stream_major=stream_major)
            y = s = None
        else:
            y, s = AG.run_far(p, xt, st, None, ct, stream_major=stream_major)
            assert tuple(y.shape) == ((ns, T, p.n_out) if stream_major else (T, ns, p.n_out))
            loss = (y * wt).sum() + (s * dev(sb)).sum()
        loss.backward()
        gx = xt.grad.cpu().numpy()
        ycpu = None if y is None else y.detach().cpu().numpy()
        return (loss.item(), gx.transpose(1, 0, 2) if stream_major else gx, st.grad.cpu().numpy(), ct.grad.numpy(),
                ycpu.transpose(1, 0, 2) if stream_major and ycpu is not None else ycpu, None if s is None else s.detach().cpu().numpy())

    for fused in (False, True):
        sm, tm = grads(True, fused), grads(False, fused)
        assert same(sm[1], tm[1]) and same(sm[2], tm[2]) and same(sm[3], tm[3]), f"fused={fused}"
        if fused:
            assert sm[0] == tm[0]
        else:
            assert same(sm[4], tm[4]) and same(sm[5], tm[5])           # y through the layout adapter, the state rows as they are
    # run_far against float64 autograd
    sm = grads(True, False)
    want = A.torch_grad(p, x, yb, ages(s0, 0), par, ages(sb, T % D))
    assert A.rel_err(sm[1], want["x"]) <= 1e-4
    assert A.rel_err(ages(sm[2], 0), want["state"]) <= 1e-4 and not sm[2][D:].any()      # the phase row's gradient: zero
    assert A.rel_err(sm[3], want["consts"].sum(1)) <= 1e-4
    # mse_far against float64 autograd
    sm = grads(True, True)
    L = A.Layout(p)
    t64 = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=torch.float64, requires_grad=True)   # noqa: E731
    x64, s64, c64 = t64(x), t64(ages(s0, 0)), t64(np.repeat(L.consts.astype(np.float64)[:, None], ns, 1))
    y64, _ = A.torch_forward(L, x64, s64, torch.zeros((0, ns), dtype=torch.float64), c64)
    l64 = ((y64 - torch.tensor(np.asarray(yb, np.float64))) ** 2).mean()
    gx, gs, gc = torch.autograd.grad(l64, (x64, s64, c64))
    assert abs(sm[0] - l64.item()) <= 1e-4 * abs(l64.item())
    assert A.rel_err(sm[1], gx.numpy()) <= 1e-4
    assert A.rel_err(ages(sm[2], 0), gs.numpy()) <= 1e-4 and not sm[2][D:].any()
    assert A.rel_err(sm[3], gc.numpy().sum(1)) <= 1e-4
    # a [batch, time] tensor as it lies, and the families below keep refusing
    x2 = t_sm(x)[..., 0].contiguous().requires_grad_()
    l2 = AG.mse_far(p, x2, t_sm(yb)[..., 0].contiguous(), dev(s0), stream_major=True)
    l2.backward()
    assert tuple(x2.grad.shape) == (ns, T) and same(x2.grad.cpu().numpy().T[..., None], sm[1]) and l2.item() == sm[0]
    for refused in (AG.run_rings, AG.run):
        with pytest.raises(F.FlowzError):
            refused(p, t_sm(x), dev(s0), stream_major=True)
    with pytest.raises(F.FlowzError):
        AG.mse_rings(p, t_sm(x), t_sm(yb), dev(s0), stream_major=True)
