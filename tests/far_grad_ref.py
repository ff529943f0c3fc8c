"""The far backward (fz_run_block_far_grad, fz_run_block_far_loss_grad) restated: tests/adjoint_ref.py and tests/loss_grad_ref.py
unchanged -- their shifts take a line of any depth -- wrapped by the conversion between the two ways a far line's state rows are laid
out.  adjoint_ref keeps AGES (row row0 + j is the value j + 1 samples ago); the caller of the library keeps ring SLOTS and a phase p
(the value j + 1 samples ago sits in slot (p - 1 - j) mod D).  On the way in `state` is converted by the phase p0 it carries and
state_grad by (p0 + T) mod D, the phase after the block; on the way out state0_grad by p0, its phase rows +0.0."""
import numpy as np

import adjoint_ref as A
import far_grad_graphs as FG
import loss_grad_ref as LR

F32 = np.float32


def convert(rows, phases, far):
    """the far lines' rows from slots to ages or from ages to slots -- j <-> (p - 1 - j) mod D is its own inverse --, every other row as
    it is.  far: far_grad_graphs.far_rows(p); phases: one per far line"""
    rows = np.asarray(rows, F32)
    out = rows.copy()
    for (r0, D, _), ph in zip(far, phases):
        out[r0:r0 + D] = rows[r0:r0 + D][(int(ph) - 1 - np.arange(D)) % D]
    return out


def phases(state, far):
    """the phase every far line's phase row of `state` carries (the first stream's, as the kernels take it), modulo its depth"""
    return [int(state[pr, 0]) % D for _, D, pr in far]


def _in(prog, T, ns, state, state_grad):
    far = FG.far_rows(prog)
    state = np.zeros((prog.n_state, ns), F32) if state is None else np.asarray(state, F32)
    ph = phases(state, far)
    after = [(p + T) % D for p, (_, D, _) in zip(ph, far)]
    return far, ph, convert(state, ph, far), None if state_grad is None else convert(state_grad, after, far)


def _out(prog, r, ph, far):
    ns = r["state"].shape[1]
    st = np.zeros((prog.n_state, ns), F32)                # (the phase rows: +0.0)
    st[:r["state"].shape[0]] = convert(r["state"], ph, far)
    r["state"] = st
    return r


def forward(prog, x, state=None, params=None):
    """(y, the state after the block in the caller's layout: slots, and the phase rows advanced by T modulo the depths)"""
    x = np.asarray(x, F32)
    T, ns, _ = x.shape
    far, ph, ages, _ = _in(prog, T, ns, state, None)
    y, s = A.forward(prog, x, ages, params)
    after = [(p + T) % D for p, (_, D, _) in zip(ph, far)]
    st = np.zeros((prog.n_state, ns), F32)
    st[:s.shape[0]] = convert(s, after, far)
    for (_, _, pr), p in zip(far, after):
        st[pr] = F32(p)
    return y, st


def grad(prog, x, out_grad, state=None, params=None, state_grad=None, accum_params=None, accum_consts=None):
    """dict x / state / params / consts of fz_run_block_far_grad's bits"""
    x = np.asarray(x, F32)
    T, ns, _ = x.shape
    far, ph, ages, sg = _in(prog, T, ns, state, state_grad)
    return _out(prog, A.grad(prog, x, out_grad, ages, params, sg, accum_params, accum_consts), ph, far)


def loss_grad(prog, x, target, k, state=None, params=None, state_grad=None, accum_params=None, accum_consts=None, accum_loss=None):
    """dict x / state / params / consts / loss / out of fz_run_block_far_loss_grad's bits"""
    x = np.asarray(x, F32)
    T, ns, _ = x.shape
    far, ph, ages, sg = _in(prog, T, ns, state, state_grad)
    return _out(prog, LR.loss_grad(prog, x, target, k, ages, params, sg, accum_params, accum_consts, accum_loss), ph, far)
