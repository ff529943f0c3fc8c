"""The backward under a squared-error loss (fz_run_block_loss_grad) restated with tests/adjoint_ref.py, in the order include/flowz_hip.h
documents: y = the forward's float32 bits, e = y - target, ybar = e * k (one rounding each), then fz_run_block_grad's restatement given
that ybar; the loss is one float32 accumulator per stream that starts from what the caller passed and takes e * e (the product rounded,
then the sum) over the rows T-1 .. 0, the output slots of a row in ascending order."""
import numpy as np

import adjoint_ref as A

F32 = np.float32


def loss_grad(prog, x, target, k, state=None, params=None, state_grad=None, accum_params=None, accum_consts=None, accum_loss=None, ref=A):
    """dict x / state / params / consts / loss / out of fz_run_block_loss_grad's bits; time-major arrays, target [T, ns, n_out].
    ref: the module whose forward() and grad() restate the program -- tests/adjoint_ref_trig.py for one with sin, cos or log"""
    x, target = np.asarray(x, F32), np.asarray(target, F32)
    T, ns, _ = x.shape
    y, _ = ref.forward(prog, x, state, params)
    with np.errstate(all="ignore"):
        e = y - target
        ybar = e * F32(k)
        loss = np.zeros(ns, F32) if accum_loss is None else np.array(accum_loss, F32).copy()
        for t in range(T - 1, -1, -1):
            for j in range(y.shape[2]):
                loss = loss + e[t, :, j] * e[t, :, j]
    r = ref.grad(prog, x, ybar, state, params, state_grad, accum_params, accum_consts)
    r["loss"], r["out"] = loss, y
    return r


# ---- the kernels the tests resolve: tests/golden/loss_grad_kernels.fzm.gz ---------------------------------------------------------------
GPU_GRAPHS = ("df1_cascade_params6", "moog_ladder", "rules", "par4_sum", "div_sqrt_exp")


def kernel_requests():
    """(program, checkpoint_rows, stream_major) of every loss kernel tests/test_loss_grad_gpu.py launches and tests/test_loss_grad_host.py
    builds.  The manifest is recorded without a GPU:
        FLOWZ_HIP_MANIFEST=m.fzm python -c "import sys; sys.path.insert(0, 'tests'); import loss_grad_ref as L; L.record()"; gzip -9n m.fzm"""
    import grad_graphs as GG
    import graphs as G
    from zignal_amd import flowz as F
    for name in sorted(GG.SUPPORTED):
        p = F.compile(F.from_sexpr(GG.SUPPORTED[name]()))
        for c in (0, 1, 4) if name in GPU_GRAPHS else (0,):
            for sm in (False, True):
                yield p, c, sm
    yield F.compile(F.from_sexpr(G.fb(G.add(G.mul(G.param(0), G.DEL(1, 1)), G.IN(2))))), 0, False   # the one-pole of the Adam fit


def record():
    for p, c, sm in kernel_requests():
        p.loss_grad_resources(c, stream_major=sm)
