"""Both loss-gradient kernels on the MI355X over the fuzz cells (tests/grad_fuzz_cells.py; the draws and the kernels' manifest in
tests/loss_grad_fuzz.py): in_grad, state0_grad, param_grad, const_grad, loss and out bit for bit against tests/loss_grad_ref.py, the
stream-major kernel also against the time-major one -- with more than one output wire, frames of unequal widths, no input wire, no
state, output slots without arithmetic, every (C, R) class; the gradients against the plain adjoint kernels given the same dL/dy;
chaining, checkpoint strides, subsets, targets at their edges, and the sin / cos / log graphs.  Every comparison is bit for bit, a NaN
of any payload equal to a NaN."""
import ctypes

import numpy as np
import pytest

import adjoint_ref as A
import adjoint_ref_trig as AT
import grad_fuzz_cells as GC
import loss_grad_fuzz as LF
import loss_grad_ref as LR
import grad_harness as H
import trig_cells as TC
from grad_harness import F32, K, SENTINEL, dev, gpu_flowz, grid, on_gpu_sm, outside_keeps_sentinel, same, to_sm
from grad_harness import on_gpu as on_gpu_plain
from grad_harness import on_gpu_loss as on_gpu

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

N_CHUNKS = LF.N_CHUNKS
assert K == LF.K


@pytest.fixture(scope="module")
def F():
    return gpu_flowz()


KEYS = H.LOSS_KEYS


def check(p, got, want, what, keys=KEYS):
    H.check(p, got, want, what, keys)


def refused(F, p):
    with pytest.raises(F.FlowzError) as ei:
        p.loss_grad_resources(stream_major=True)
    assert ei.value.code == F.C.FZ_E_UNSUPPORTED and "does not fit the LDS" in str(ei.value)
    return True


def bits(a, b):
    return a.shape == b.shape and bool(np.all(a.view(np.uint32) == b.view(np.uint32)))


def window_is_clean(p, got, row0, T, what):
    """a stream-major launch with in_grad and out asked for: rows of both outside the window keep the sentinel, and the caller's target
    is what it was (y takes the target's place in the LDS patch only)"""
    assert outside_keeps_sentinel(got["x_buffer"], row0, T), what + ": rows of in_grad outside the window were written"
    assert outside_keeps_sentinel(got["out_buffer"], row0, T), what + ": rows of out outside the window were written"
    assert bits(got["target_after"], got["target_sent"]), what + ": the target buffer was written"


# ---- a. both kernels against the restatement ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("part", range(N_CHUNKS))
def test_both_loss_kernels_match_the_restatement_bitwise(F, part):
    for cell in GC.CELLS[part::N_CHUNKS]:
        p = GC.prog(cell)
        c, r = GC.strides(p)
        for i, (ns, T) in enumerate(GC.shapes(cell)):
            d = LF.draw(cell, ns, T, GC.GPU_SEED + i)
            x, s0, par, tg, sb, ap, ac, al = d
            what = f"{cell} ns={ns} T={T} (C={c}, R={r}, {p.n_in} in, {p.n_out} out)"
            want = LR.loss_grad(p, x, tg, K, s0, par, sb, ap, ac, al)
            tm = on_gpu(p, False, *d)
            assert set(KEYS) <= set(tm)
            check(p, tm, want, what + " time-major against the restatement")
            if r is None:
                assert refused(F, p)
                continue
            # one shape per cell: the window starts behind row 0 and a tail follows it
            row0, tail = (grid(p, 4), 5) if i == 4 else (0, 0)
            rows = grid(p, row0 + T + tail)
            sm = on_gpu(p, True, *d, rows=rows, row0=row0)
            check(p, sm, want, what + f" stream-major window [{row0}, {row0 + T}) of {rows} against the restatement")
            check(p, sm, tm, what + " stream-major against time-major")
            window_is_clean(p, sm, row0, T, what)


# ---- b. every gradient bit is fz_run_block_grad's for that dL/dy --------------------------------------------------------------------
@pytest.mark.parametrize("part", range(N_CHUNKS))
def test_the_gradients_are_the_plain_adjoint_kernels_given_the_same_out_grad(F, part):
    for cell in GC.CELLS[part::N_CHUNKS]:
        p = GC.prog(cell)
        c, r = GC.strides(p)
        i, T = LF.longest_65(cell)
        d = LF.draw(cell, 65, T, GC.GPU_SEED + i)
        x, s0, par, tg, sb, ap, ac, al = d
        y, _ = A.forward(p, x, s0, par)
        with np.errstate(all="ignore"):
            ybar = ((y - tg) * F32(K)).astype(F32)
        tm = on_gpu(p, False, *d)
        assert same(tm["out"], y), f"{cell}: the restated y is not the kernel's"
        check(p, tm, on_gpu_plain(p, x, s0, par, ybar, sb, ap, ac), f"{cell} time-major, loss kernel against plain kernel", H.GRAD_KEYS)
        if r is None:
            assert refused(F, p)
            continue
        rows = grid(p, T)
        check(p, on_gpu(p, True, *d, rows=rows), on_gpu_sm(p, x, s0, par, ybar, sb, ap, ac, rows=rows), f"{cell} stream-major, loss kernel against plain kernel", H.GRAD_KEYS)


# ---- c. two blocks chain like one ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("part", range(N_CHUNKS))
def test_two_blocks_chain_like_one_in_both_layouts(F, part):
    """the second half, then the first on the same three accumulators (the loss among them) with the second's state adjoint, give the
    whole block's bits; stream-major, the two windows fill one in_grad and one out buffer.  The state between the halves is
    adjoint_ref.forward's (the forward kernels' bits: no forward kernel is compiled)"""
    for cell in GC.CELLS[part::N_CHUNKS]:
        p = GC.prog(cell)
        c, r = GC.strides(p)
        ns, T1 = 65, grid(p, (r or c) + c + 1)                     # (the second window starts on the float4 grid)
        T2 = (r or c) + 3
        x, s0, par, tg, sb, ap, ac, al = LF.draw(cell, ns, T1 + T2, 600)
        _, s_mid = A.forward(p, x[:T1], s0, par)

        def halves(sm, row0=0, **kw):
            second = on_gpu(p, sm, x[T1:], s_mid, par, tg[T1:], sb, ap, ac, al, row0=row0, **kw)
            return second, on_gpu(p, sm, x[:T1], s0, par, tg[:T1], second["state"], second["params"], second["consts"], second["loss"], row0=0, **kw)
        whole = on_gpu(p, False, x, s0, par, tg, sb, ap, ac, al)
        second, first = halves(False)
        chained = dict(first, x=np.concatenate([first["x"], second["x"]]), out=np.concatenate([first["out"], second["out"]]))
        check(p, chained, whole, f"{cell} chained, time-major")
        if r is None:
            assert refused(F, p)
            continue
        rows = grid(p, T1 + T2)
        whole_sm = on_gpu(p, True, x, s0, par, tg, sb, ap, ac, al, rows=rows)
        check(p, whole_sm, whole, f"{cell} whole block, stream-major against time-major")
        bx, bo = (torch.full((ns, rows, w), float(SENTINEL), device="cuda") for w in (p.n_in, p.n_out))
        second, first = halves(True, rows=rows, row0=T1, in_grad=bx, out=bo)
        assert same(first["x_buffer"], whole_sm["x_buffer"]), f"{cell}: the in_grad buffer filled by two windows differs"
        assert same(first["out_buffer"], whole_sm["out_buffer"]), f"{cell}: the out buffer filled by two windows differs"
        check(p, {k: first[k] for k in ("state", "params", "consts", "loss")}, whole_sm, f"{cell} chained windows, stream-major")


# ---- d. checkpoint strides ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sm", [False, True])
@pytest.mark.parametrize("cell", GC.STRIDE_CELLS)
def test_bits_do_not_depend_on_the_checkpoint_stride(F, cell, sm):
    p = GC.prog(cell)
    ns, T = 65, 37
    d = LF.draw(cell, ns, T, 700)
    x, s0, par, tg, sb, ap, ac, al = d
    ref = on_gpu(p, sm, *d, rows=grid(p, T))
    check(p, ref, LR.loss_grad(p, x, tg, K, s0, par, sb, ap, ac, al), f"{cell} default stride")
    for c in (1, 4):
        check(p, on_gpu(p, sm, *d, checkpoint_rows=c, rows=grid(p, T)), ref, f"{cell} C={c}")


# ---- e. subsets, where in_grad and out differ in width ------------------------------------------------------------------------------
@pytest.mark.parametrize("sm", [False, True])
def test_want_subsets_leave_the_other_buffers_alone(F, sm):
    from zignal_amd import _capi as CA
    cell = LF.SUBSET_CELL
    p = GC.prog(cell)
    assert p.n_out >= 2 and p.n_out != p.n_in
    ns, T = 129, 41
    rows = grid(p, T + 3)
    x, s0, par, tg, sb, ap, ac, al = LF.draw(cell, ns, T, 17)
    full = on_gpu(p, sm, x, s0, par, tg, sb, ap, ac, al, rows=rows)
    check(p, full, LR.loss_grad(p, x, tg, K, s0, par, sb, ap, ac, al), f"{cell} everything asked for")
    names = {"x": "in_grad", "state": "state0_grad", "params": "param_grad", "consts": "const_grad", "loss": "loss", "out": "out"}
    fshape = lambda w: (ns, rows, w) if sm else (T, ns, w)        # noqa: E731
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None   # noqa: E731
    for want in (("out",), ("loss",), ("x",), ("x", "out"), (), ("state", "params", "consts"), ("out", "loss")):
        bufs = {"in_grad": torch.full(fshape(p.n_in), float(SENTINEL), device="cuda"), "state0_grad": torch.full((p.n_state, ns), float(SENTINEL), device="cuda"),
                "param_grad": dev(ap), "const_grad": dev(ac), "loss": dev(al), "out": torch.full(fshape(p.n_out), float(SENTINEL), device="cuda")}
        before = {k: v.clone() for k, v in bufs.items()}
        ws = torch.empty(max(p.grad_workspace_bytes(ns, T), 16) // 4, device="cuda")
        a = CA.LossGradArgs()
        a.struct_size, a.grad_scale = ctypes.sizeof(CA.LossGradArgs), K
        keep = [dev(to_sm(x, rows) if sm else x), dev(s0), dev(par), dev(to_sm(tg, rows) if sm else tg), dev(sb)]
        a.in_, a.state, a.params, a.target, a.state_grad = (ptr(t) for t in keep)
        for k, b in names.items():
            setattr(a, b, ptr(bufs[b]) if k in want else None)
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


# ---- f. targets at their edges --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sm", [False, True])
@pytest.mark.parametrize("cell", LF.EDGE_CELLS)
def test_targets_at_their_edges(F, cell, sm):
    """loss_grad_fuzz.edge_case: streams whose target is y itself, NaN, +-inf, +-0, far enough for e * e to overflow, near enough for it
    to be denormal, next to ordinary streams"""
    p = GC.prog(cell)
    ns, T = 65, GC.strides(p)[1] + 3
    d, kinds = LF.edge_case(cell, ns, T, 900)
    x, s0, par, tg, sb, ap, ac, al = d
    want = LR.loss_grad(p, x, tg, K, s0, par, sb, ap, ac, al)
    got = on_gpu(p, sm, *d, rows=grid(p, T))
    assert set(KEYS) <= set(got)
    check(p, got, want, f"{cell} {'stream' if sm else 'time'}-major, targets at their edges")
    s = kinds.index("y")                                          # (the value fills this stream: e = +0 in every row)
    assert got["loss"][s].view(np.uint32) == al[s].view(np.uint32), "e = +0 in every row: the loss is the accumulator"
    assert np.all(np.isinf(got["loss"][[k == "overflow" for k in kinds]]))
    if sm:
        window_is_clean(p, got, 0, T, cell)


# ---- g. sin, cos, log -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", TC.GRAD_GRAPHS)
@pytest.mark.parametrize("C", LF.TRIG_STRIDES)
def test_sin_cos_log_under_the_loss(F, name, C):
    p = TC.graph(name)
    ns, T = LF.TRIG_SHAPE
    d = LF.draw_trig(p, ns, T, 21)
    x, s0, par, tg, sb, ap, ac, al = d
    want = LR.loss_grad(p, x, tg, K, s0, par, sb, ap, ac, al, ref=AT)
    tm = on_gpu(p, False, *d, checkpoint_rows=C)
    check(p, tm, want, f"{name} time-major C={C}")
    sm = on_gpu(p, True, *d, checkpoint_rows=C)
    check(p, sm, want, f"{name} stream-major C={C}")
    check(p, sm, tm, f"{name} stream-major against time-major C={C}")
    win = on_gpu(p, True, *d, checkpoint_rows=C, row0=LF.TRIG_ROW0)
    check(p, win, want, f"{name} stream-major window at row {LF.TRIG_ROW0}, C={C}")
    window_is_clean(p, win, LF.TRIG_ROW0, T, name)
