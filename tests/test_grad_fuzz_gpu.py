"""Both adjoint kernels on the MI355X over the fuzz cells (tests/grad_fuzz_cells.py): the time-major kernel against tests/adjoint_ref.py
bit for bit, the stream-major kernel against it and against the time-major kernel, around the wave, chunk and patch boundaries; windows
of larger buffers, chaining of two blocks in both layouts, and checkpoint strides other than the default's."""
import numpy as np
import pytest

import adjoint_ref as A
import grad_fuzz_cells as GC
import grad_harness as H
from grad_harness import gpu_flowz, grid, on_gpu, on_gpu_sm, outside_keeps_sentinel, same

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

N_CHUNKS = 8                                       # about six cells per test


@pytest.fixture(scope="module")
def F():
    return gpu_flowz()


def check(p, got, want, what):
    H.check(p, got, want, what, H.GRAD_KEYS)


def refused(F, p):
    with pytest.raises(F.FlowzError) as ei:
        p.grad_resources(stream_major=True)
    assert ei.value.code == F.C.FZ_E_UNSUPPORTED and "does not fit the LDS" in str(ei.value)
    return True


@pytest.mark.parametrize("part", range(N_CHUNKS))
def test_both_kernels_match_the_restatement_bitwise(F, part):
    for cell in GC.CELLS[part::N_CHUNKS]:
        p = GC.prog(cell)
        c, r = GC.strides(p)
        for i, (ns, T) in enumerate(GC.shapes(cell)):
            args = GC.inputs(cell, ns, T, GC.GPU_SEED + i)
            x, s0, par, yb, sb, ap, ac = args
            what = f"{cell} ns={ns} T={T} (C={c}, R={r})"
            want = A.grad(p, x, yb, s0, par, sb, ap, ac)
            tm = on_gpu(p, *args)
            check(p, tm, want, what + " time-major against the restatement")
            if r is None:
                assert refused(F, p)
                continue
            # one shape per cell: the window starts behind row 0 and a tail follows it
            row0, tail = (grid(p, 4), 5) if i == 4 else (0, 0)
            rows = grid(p, row0 + T + tail)
            sm = on_gpu_sm(p, *args, rows=rows, row0=row0)
            check(p, sm, want, what + f" stream-major window [{row0}, {row0 + T}) of {rows} against the restatement")
            check(p, sm, tm, what + " stream-major against time-major")
            if p.n_in:
                assert outside_keeps_sentinel(sm["x_buffer"], row0, T), what + ": rows of in_grad outside the window were written"


@pytest.mark.parametrize("part", range(N_CHUNKS))
def test_two_blocks_chain_like_one_in_both_layouts(F, part):
    """the backward of the second half, then of the first on the same accumulators with the second's state adjoint, gives the whole
    block's bits; the state between the halves is adjoint_ref.forward's (the forward kernels' bits: no forward kernel is compiled)"""
    for cell in GC.CELLS[part::N_CHUNKS]:
        p = GC.prog(cell)
        c, r = GC.strides(p)
        ns, T1 = 65, grid(p, (r or c) + c + 1)                     # (the second window starts on the float4 grid)
        T2 = (r or c) + 3
        x, s0, par, yb, sb, ap, ac = GC.inputs(cell, ns, T1 + T2, 600)
        _, s_mid = A.forward(p, x[:T1], s0, par)
        whole = on_gpu(p, x, s0, par, yb, sb, ap, ac)
        second = on_gpu(p, x[T1:], s_mid, par, yb[T1:], sb, ap, ac)
        first = on_gpu(p, x[:T1], s0, par, yb[:T1], second["state"], second.get("params"), second.get("consts"))
        chained = dict(first, x=np.concatenate([first["x"], second["x"]]))
        check(p, chained, whole, f"{cell} chained, time-major")
        if r is None:
            assert refused(F, p)
            continue
        rows = grid(p, T1 + T2)
        whole_sm = on_gpu_sm(p, x, s0, par, yb, sb, ap, ac, rows=rows)
        check(p, whole_sm, whole, f"{cell} whole block, stream-major against time-major")
        buf = torch.full((ns, rows, p.n_in), -1234.5, device="cuda")
        second = on_gpu_sm(p, x[T1:], s_mid, par, yb[T1:], sb, ap, ac, rows=rows, row0=T1, in_grad=buf)
        first = on_gpu_sm(p, x[:T1], s0, par, yb[:T1], second["state"], second.get("params"), second.get("consts"), rows=rows, row0=0, in_grad=buf)
        assert same(first["x_buffer"], whole_sm["x_buffer"]), f"{cell}: the in_grad buffer filled by two windows differs"
        check(p, {k: first[k] for k in ("state", "params", "consts") if k in first}, whole_sm, f"{cell} chained windows, stream-major")


@pytest.mark.parametrize("cell", GC.STRIDE_CELLS)
def test_bits_do_not_depend_on_the_checkpoint_stride(F, cell):
    p = GC.prog(cell)
    ns, T = 65, 37
    args = GC.inputs(cell, ns, T, 700)
    ref_tm, ref_sm = on_gpu(p, *args), on_gpu_sm(p, *args, rows=grid(p, T))
    check(p, ref_tm, A.grad(p, *[args[k] for k in (0, 3, 1, 2, 4, 5, 6)]), f"{cell} default stride")
    check(p, ref_sm, ref_tm, f"{cell} default stride, stream-major")
    for c in (1, 4):
        check(p, on_gpu(p, *args, checkpoint_rows=c), ref_tm, f"{cell} C={c} time-major")
        check(p, on_gpu_sm(p, *args, checkpoint_rows=c, rows=grid(p, T)), ref_sm, f"{cell} C={c} stream-major")
