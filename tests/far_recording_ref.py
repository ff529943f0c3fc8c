"""The far backward of a whole recording (fz_run_recording_far_grad, fz_run_recording_far_loss_grad) restated in numpy:
tests/far_grad_ref.py applied block by block, from the last block to the first -- tests/recording_ref.py's chaining restated over the
far layout.  The state carries prog.n_state rows in the caller's layout: a far line's rows are ring SLOTS, and its phase row advances by
the block's rows modulo its depth from one block start to the next; the state0 gradient a block leaves is the state gradient of the
block in front of it AS IT IS, slot for slot.  include/flowz_hip.h says every bit equals the single far call over the T rows;
test_far_recording_host.py holds this file to that, the GPU test the kernels to both.

wrong: a chain that is NOT the contract, for the host test that shows the restatement tells them apart --
  "rotated"      the far slots of every block start but the first are rotated by one slot,
  "stale_phase"  the phase rows of every block start but the first are those of the block start before it."""
import numpy as np

import far_grad_graphs as FG
import far_grad_ref as FR

F32 = np.float32


def starts(prog, x, B, state=None, params=None):
    """(the state before rows 0, B, 2B, ... [ceil(T / B)][n_state][ns] in the caller's layout, the state after row T-1): the forward's
    bits, slots and phase rows included"""
    x = np.asarray(x, F32)
    T, ns = x.shape[:2]
    s = np.zeros((prog.n_state, ns), F32) if state is None else np.array(state, F32).reshape(prog.n_state, ns)
    out = []
    for t0 in range(0, T, B):
        out.append(s.copy())
        _, s = FR.forward(prog, x[t0:t0 + B], s, params)
    return np.stack(out), s


def spoil(prog, st, wrong):
    """the block starts of a wrong chain (a copy)"""
    assert wrong in ("rotated", "stale_phase")
    right, st = st, st.copy()
    for k in range(1, len(st)):
        for r0, D, pr in FG.far_rows(prog):
            if wrong == "rotated":
                st[k, r0:r0 + D] = np.roll(right[k, r0:r0 + D], 1, axis=0)
            else:
                st[k, pr] = right[k - 1, pr]
    return st


def grad(prog, x, B, out_grad=None, target=None, k=None, state=None, params=None, state_grad=None, accum_params=None, accum_consts=None,
         accum_loss=None, wrong=None):
    """dict x / state / params / consts (and loss / out with a target) of the far recording calls, plus "starts" and "state_out".
    out_grad: the plain backward (far_grad_ref.grad per block); target and k: the squared-error one (far_grad_ref.loss_grad per block)"""
    x = np.asarray(x, F32)
    T = x.shape[0]
    B = min(B, T)
    st, s_out = starts(prog, x, B, state, params)
    use = st if wrong is None else spoil(prog, st, wrong)
    sb, ap, ac, al = state_grad, accum_params, accum_consts, accum_loss
    gx, ys = [None] * len(st), [None] * len(st)
    r = None
    for kb in range(len(st) - 1, -1, -1):
        rows = slice(kb * B, min((kb + 1) * B, T))
        if target is None:
            r = FR.grad(prog, x[rows], out_grad[rows], use[kb], params, sb, ap, ac)
        else:
            r = FR.loss_grad(prog, x[rows], target[rows], k, use[kb], params, sb, ap, ac, al)
            al, ys[kb] = r["loss"], r["out"]
        gx[kb], sb, ap, ac = r["x"], r["state"], r["params"], r["consts"]
    res = dict(r, x=np.concatenate(gx), starts=st, state_out=s_out)
    if target is not None:
        res["out"] = np.concatenate(ys)
    return res
