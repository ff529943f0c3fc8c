"""The backward of a whole recording (fz_run_recording_grad, fz_run_recording_loss_grad) restated in numpy: tests/adjoint_ref.py or
tests/loss_grad_ref.py applied block by block, from the last block to the first -- block k is rows [k B, min((k + 1) B, T)), its state
the forward's state before row k B, its state gradient the state0 gradient the block behind it left, the parameter, coefficient and
loss accumulators handed on.  include/flowz_hip.h says every bit equals the single call over the T rows; test_recording_grad_host.py
holds this file to that (the chaining property the driver rests on, independently of the kernels), the GPU test the kernels to both."""
import numpy as np

import adjoint_ref as A
import loss_grad_ref as LR

F32 = np.float32


def block_rows(T, C, B=0):
    """the rows per block: B, at most T; B = 0: the library's rule -- sqrt(T C) rounded up to a multiple of lcm(4, C) = max(4, C), and T
    when that is not smaller"""
    if B:
        return min(B, T)
    m = max(4, C)
    b = int(np.ceil(np.sqrt(float(T * C))))
    while b * b < T * C:
        b += 1
    b = (b + m - 1) // m * m
    return b if b < T else T


def starts(prog, x, B, state=None, params=None, ref=A):
    """(the state before rows 0, B, 2B, ... [ceil(T / B)][n_state][ns], the state after row T-1): the forward's bits"""
    T, ns = x.shape[:2]
    L = A.Layout(prog)
    s = np.zeros((L.n_state, ns), F32) if state is None else np.array(state, F32)[:L.n_state].reshape(L.n_state, ns).copy()
    out = []
    for t0 in range(0, T, B):
        out.append(s.copy())
        _, s = ref.forward(prog, x[t0:t0 + B], s, params)
        s = np.asarray(s, F32)[:L.n_state].reshape(L.n_state, ns)
    return np.stack(out), s


def grad(prog, x, B, out_grad=None, target=None, k=None, state=None, params=None, state_grad=None, accum_params=None, accum_consts=None,
         accum_loss=None, ref=A):
    """dict x / state / params / consts (and loss / out with a target) of the recording calls, plus "starts" and "state_out".
    out_grad: the plain backward (adjoint_ref.grad per block); target and k: the squared-error one (loss_grad_ref.loss_grad per block)"""
    x = np.asarray(x, F32)
    T = x.shape[0]
    B = min(B, T)
    st, s_out = starts(prog, x, B, state, params, ref)
    sb, ap, ac, al = state_grad, accum_params, accum_consts, accum_loss
    gx, ys = [None] * len(st), [None] * len(st)
    r = None
    for kb in range(len(st) - 1, -1, -1):
        rows = slice(kb * B, min((kb + 1) * B, T))
        s0 = st[kb] if st.shape[1] else None
        if target is None:
            r = ref.grad(prog, x[rows], out_grad[rows], s0, params, sb, ap, ac)
        else:
            r = LR.loss_grad(prog, x[rows], target[rows], k, s0, params, sb, ap, ac, al, ref=ref)
            al, ys[kb] = r["loss"], r["out"]
        gx[kb], sb, ap, ac = r["x"], r["state"], r["params"], r["consts"]
    res = dict(r, x=np.concatenate(gx), starts=st, state_out=s_out)
    if target is not None:
        res["out"] = np.concatenate(ys)
    return res


# ---- the kernels the tests resolve: tests/golden/recording_kernels.fzm.gz -----------------------------------------------------------
GPU_GRAPHS = ("integrator", "df1_cascade_params6", "moog_ladder", "par4_sum")
GPU_CELLS = ("make11", "grad133", "generator_without_input", "no_delay_line", "cascade9_depth8")
# (n_streams, T, block_rows) of the GPU test: the masked tail, a wave boundary, a second workgroup; a partial last block with chunk tails at
# C = 4 and C = 8; B no multiple of C; a single block; one block of exactly T rows
GPU_SHAPES = [(ns, 37, 8) for ns in (1, 63, 65, 257)] + [(65, 37, 12), (257, 37, 40), (63, 8, 8)]


def programs():
    """name -> program of every graph tests/test_recording_grad_gpu.py runs"""
    import grad_fuzz_cells as GC
    import grad_graphs as GG
    from zignal_amd import flowz as F
    out = {n: F.compile(F.from_sexpr(GG.SUPPORTED[n]())) for n in GPU_GRAPHS}
    out.update({c: GC.prog(c) for c in GPU_CELLS})
    return out


def record():
    """resolve every kernel the GPU test launches -- the states kernels, the adjoint and loss kernels at the strides it asks for, the forward kernels it compares states with --
    and the one-pole of examples/fit_one_pole_recording.py.  The manifest is recorded without a GPU:
        FLOWZ_HIP_MANIFEST=m.fzm python -c "import sys; sys.path.insert(0, 'tests'); import recording_ref as R; R.record()"; gzip -9n m.fzm"""
    import graphs as G
    from zignal_amd import flowz as F
    progs = list(programs().values()) + [F.compile(F.from_sexpr(G.fb(G.add(G.mul(G.param(0), G.DEL(1, 1)), G.IN(2)))))]
    for p in progs:
        for sm in (False, True):
            if p.n_state:
                p.states_resources(sm)
            for c in (0, 8):
                p.grad_resources(c, stream_major=sm)
                if p.n_out:
                    p.loss_grad_resources(c, stream_major=sm)
    for p in progs[:-1]:                                          # the forward kernels the test takes its block-start states from
        for ns, T, B in GPU_SHAPES:
            for rows in sorted(set(range(min(B, T), T, min(B, T))) | {T}):
                p.build(None, ns, rows)
