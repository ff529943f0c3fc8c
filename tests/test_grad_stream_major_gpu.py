"""The adjoint kernel for stream-major buffers on the MI355X (fz_run_block_grad_stream_major): every output bit for bit against
tests/adjoint_ref.py on the transposed arrays AND against the time-major kernel on the transposed buffers -- the layout does not
change a bit --, around every boundary the kernel has (wave, checkpoint chunk, LDS patch); windows of larger buffers, chaining,
checkpoint strides, subsets, repeatability, and autograd.run(..., stream_major=True)."""
import ctypes
import re

import pytest

import adjoint_ref as A
import grad_graphs as GG
import grad_harness as H
from grad_harness import SENTINEL, dev, gpu_flowz, make_inputs, on_gpu_sm, outside_keeps_sentinel, same, to_sm, up4
from grad_harness import on_gpu as on_gpu_time_major

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


def strides(p, checkpoint_rows=0):
    """(C, R) of the stream-major kernel: its symbol names them"""
    m = re.match(r"fz_adjoint_sm_kernel_c(\d+)r(\d+)b", p.grad_kernel_symbol(checkpoint_rows, stream_major=True))
    return int(m.group(1)), int(m.group(2))


def check(p, got, want, what):
    H.check(p, got, want, what, KEYS)


@pytest.mark.parametrize("name", sorted(GG.SUPPORTED))
def test_stream_major_adjoint_matches_reference_and_time_major_bitwise(F, name):
    p = prog(F, name)
    C, R = strides(p)
    Ts = sorted({1, max(C - 1, 1), C, C + 1, R - 1, R, R + 1, 2 * R + 3, 1000})
    for i, (ns, T) in enumerate((ns, T) for ns in (1, 63, 64, 65, 1000) for T in Ts):
        x, s0, par, yb, sb, ap, ac = make_inputs(p, name, ns, T, 300 + i)
        got = on_gpu_sm(p, x, s0, par, yb, sb, ap, ac)           # rows_total = T rounded up to the float4 grid; T itself is free
        what = f"{name} ns={ns} T={T} (C={C}, R={R})"
        check(p, got, A.grad(p, x, yb, s0, par, sb, ap, ac), what + " against the reference")
        check(p, got, on_gpu_time_major(p, x, s0, par, yb, sb, ap, ac), what + " against the time-major kernel")
        assert outside_keeps_sentinel(got["x_buffer"], 0, T), what + ": rows of in_grad behind the window were written"


@pytest.mark.parametrize("name", ["df1_cascade6", "moog_ladder"])
def test_stream_major_adjoint_many_streams(F, name):
    p = prog(F, name)
    C, R = strides(p)
    ns, T = 65537, R + C + 3
    x, s0, par, yb, sb, ap, ac = make_inputs(p, name, ns, T, 7)
    got = on_gpu_sm(p, x, s0, par, yb, sb, ap, ac)
    check(p, got, A.grad(p, x, yb, s0, par, sb, ap, ac), f"{name} ns={ns}")
    check(p, got, on_gpu_time_major(p, x, s0, par, yb, sb, ap, ac), f"{name} ns={ns} against the time-major kernel")


@pytest.mark.parametrize("name", ["df1_cascade6", "osc_chain6", "moog_ladder", "rules", "cross_wire", "par4_sum"])
def test_a_window_equals_the_time_major_backward_of_the_slice(F, name):
    p = prog(F, name)
    C, R = strides(p)
    for ns, row0, T, tail in ((200, 4, R + 5, 9), (65, 2 * R, 2 * R + 3, 0), (130, 8, 3, 1)):
        rows = up4(row0 + T + tail)
        x, s0, par, yb, sb, ap, ac = make_inputs(p, name, ns, T, 31 + T)
        got = on_gpu_sm(p, x, s0, par, yb, sb, ap, ac, rows=rows, row0=row0)
        check(p, got, on_gpu_time_major(p, x, s0, par, yb, sb, ap, ac), f"{name} window [{row0}, {row0 + T}) of {rows}")
        assert outside_keeps_sentinel(got["x_buffer"], row0, T), f"{name}: rows of in_grad outside [{row0}, {row0 + T}) were written"


@pytest.mark.parametrize("name", ["df1_cascade6", "osc_chain6", "moog_ladder", "rules", "cross_wire"])
def test_two_windows_of_one_buffer_chain_like_one(F, name):
    """the backward of the second window, then of the first on the same accumulators with the second's state adjoint, both writing
    into ONE in_grad buffer, give the bits of one window over both"""
    p = prog(F, name)
    C, R = strides(p)
    ns, T1 = 200, up4(R + C + 1)                                  # (the second window starts on the float4 grid)
    T2 = R + 3
    x, s0, par, yb, sb, ap, ac = make_inputs(p, name, ns, T1 + T2, 9)
    rows = up4(T1 + T2)
    whole = on_gpu_sm(p, x, s0, par, yb, sb, ap, ac, rows=rows)
    xs = dev(to_sm(x, rows))
    _, s_mid = p.run_block_stream_major(xs, dev(s0) if p.n_state else None, dev(par), row0=0, n_samples=T1)
    s_mid = s_mid.cpu().numpy()
    buf = torch.full((ns, rows, p.n_in), float(SENTINEL), device="cuda")
    second = on_gpu_sm(p, x[T1:], s_mid, par, yb[T1:], sb, ap, ac, rows=rows, row0=T1, in_grad=buf)
    first = on_gpu_sm(p, x[:T1], s0, par, yb[:T1], second["state"], second["params"], second["consts"], rows=rows, row0=0, in_grad=buf)
    assert same(first["x_buffer"], whole["x_buffer"]), f"{name}: the in_grad buffer filled by two windows differs"
    check(p, {k: first[k] for k in ("state", "params", "consts")}, whole, f"{name} chained windows")


@pytest.mark.parametrize("name", ["df1_cascade6", "moog_ladder", "envelope_follower", "div_sqrt_exp"])
def test_bits_do_not_depend_on_the_checkpoint_stride(F, name):
    p = prog(F, name)
    ns, T = 300, 77
    x, s0, par, yb, sb, ap, ac = make_inputs(p, name, ns, T, 13)
    ref = on_gpu_sm(p, x, s0, par, yb, sb, ap, ac)
    for c in (1, 4):
        check(p, on_gpu_sm(p, x, s0, par, yb, sb, ap, ac, checkpoint_rows=c), ref, f"{name} C={c}")


def test_want_subset_and_sentinels(F):
    name = "moog_ladder"
    p = prog(F, name)
    ns, T, rows = 129, 41, 44
    x, s0, par, yb, sb, ap, ac = make_inputs(p, name, ns, T, 17)
    full = on_gpu_sm(p, x, s0, par, yb, sb, ap, ac, rows=rows)
    from zignal_amd import _capi as CA
    for want in (("x",), ("state",), ("params",), ("consts",), ("x", "consts"), ("state", "params")):
        bufs = {"in_grad": torch.full((ns, rows, p.n_in), float(SENTINEL), device="cuda"), "state0_grad": torch.full((p.n_state, ns), float(SENTINEL), device="cuda"),
                "param_grad": dev(ap), "const_grad": dev(ac)}
        before = {k: v.clone() for k, v in bufs.items()}
        names = {"x": "in_grad", "state": "state0_grad", "params": "param_grad", "consts": "const_grad"}
        ws = torch.empty(max(p.grad_workspace_bytes(ns, T), 16) // 4, device="cuda")
        a = CA.GradArgs()
        a.struct_size = ctypes.sizeof(CA.GradArgs)
        keep = [dev(to_sm(x, rows)), dev(s0), dev(par), dev(to_sm(yb, rows)), dev(sb)]
        a.in_, a.state, a.params, a.out_grad, a.state_grad = (t.data_ptr() for t in keep)
        for k, b in names.items():
            setattr(a, b, bufs[b].data_ptr() if k in want else None)
        a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel() * 4
        CA.check(CA.lib.fz_run_block_grad_stream_major(p._h, ctypes.byref(a), ns, rows, 0, T, torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        for k, b in names.items():
            got = bufs[b].cpu().numpy()
            if k in want:
                assert same(got, full["x_buffer"] if k == "x" else full[k][:got.shape[0]]), (want, k)
            else:
                assert torch.equal(bufs[b], before[b]), (want, k)


def test_two_launches_give_identical_bits(F):
    p = prog(F, "soft_clip_cascade")
    x, s0, par, yb, sb, ap, ac = make_inputs(p, "soft_clip_cascade", 777, 50, 19)
    a, b = on_gpu_sm(p, x, s0, par, yb, sb, ap, ac), on_gpu_sm(p, x, s0, par, yb, sb, ap, ac)
    check(p, a, b, "repeat")
    assert same(a["x_buffer"], b["x_buffer"])


# ---- torch.autograd -----------------------------------------------------------------------------------------------------------
def test_autograd_stream_major_equals_time_major_on_transposed_tensors(F):
    from zignal_amd import autograd as AG
    name = "moog_ladder"
    p = prog(F, name)
    ns, T = 500, 40
    x, s0, par, yb, sb, ap, ac = make_inputs(p, name, ns, T, 23)

    def grads(stream_major):
        xin, ybd = (to_sm(x, T), to_sm(yb, T)) if stream_major else (x, yb)
        xt, st, pt = dev(xin).requires_grad_(), dev(s0).requires_grad_(), dev(par).requires_grad_()
        ct = torch.tensor(p.consts(), dtype=torch.float32).requires_grad_()
        st_before = st.detach().clone()
        y, s = AG.run(p, xt, st, pt, ct, stream_major=stream_major)
        assert torch.equal(st.detach(), st_before)                  # the caller's state is not advanced
        ((y * dev(ybd)).sum() + (s * dev(sb)).sum()).backward()
        return y.detach(), xt.grad.cpu().numpy(), st.grad.cpu().numpy(), pt.grad.cpu().numpy(), ct.grad.numpy()
    y_sm, gx_sm, gs_sm, gp_sm, gc_sm = grads(True)
    y_tm, gx_tm, gs_tm, gp_tm, gc_tm = grads(False)
    assert tuple(y_sm.shape) == (ns, T, p.n_out)
    y_plain, _ = p.run_block_stream_major(dev(to_sm(x, T)), dev(s0), dev(par))
    assert torch.equal(y_sm.view(torch.int32), y_plain.view(torch.int32))
    assert same(gx_sm.transpose(1, 0, 2), gx_tm) and same(gs_sm, gs_tm) and same(gp_sm, gp_tm)
    assert same(gc_sm, gc_tm)                                       # the same float64 sum of the same bits


def test_autograd_stream_major_one_wire_tensors_are_batch_by_time(F):
    from zignal_amd import autograd as AG
    p = prog(F, "df1_cascade6")
    ns, T = 256, 48
    x, s0, par, yb, sb, ap, ac = make_inputs(p, "df1_cascade6", ns, T, 27)
    x3 = dev(to_sm(x, T)).requires_grad_()
    x2 = dev(to_sm(x, T)[:, :, 0]).requires_grad_()                 # [batch, time]
    for xt in (x3, x2):
        y, s = AG.run(p, xt, dev(s0), stream_major=True)
        (y * dev(to_sm(yb, T))).sum().backward()
    assert tuple(x2.grad.shape) == (ns, T) and same(x2.grad.cpu().numpy(), x3.grad.cpu().numpy()[:, :, 0])


def test_autograd_stream_major_chain_over_two_blocks(F):
    from zignal_amd import autograd as AG
    name = "df1_cascade6"
    p = prog(F, name)
    ns, T = 256, 44
    x, s0, par, yb, sb, ap, ac = make_inputs(p, name, ns, 2 * T, 29)
    xs, ybs = to_sm(x, 2 * T), to_sm(yb, 2 * T)
    ct0 = torch.tensor(p.consts(), dtype=torch.float32)

    def grads(blocks):
        xt, st, ct = dev(xs).requires_grad_(), dev(s0).requires_grad_(), ct0.clone().requires_grad_()
        s, loss = st, 0
        for lo, hi in blocks:
            y, s = AG.run(p, xt[:, lo:hi].contiguous() if len(blocks) > 1 else xt, s, None, ct, stream_major=True)
            loss = loss + (y * dev(ybs[:, lo:hi])).sum()
        loss = loss + (s * dev(sb)).sum()
        loss.backward()
        return xt.grad.cpu().numpy(), st.grad.cpu().numpy(), ct.grad.numpy()
    gx1, gs1, gc1 = grads([(0, 2 * T)])
    gx2, gs2, gc2 = grads([(0, T), (T, 2 * T)])
    assert same(gx1, gx2) and same(gs1, gs2)
    assert A.rel_err(gc2, gc1) <= 1e-6
