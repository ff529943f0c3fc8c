"""PyTorch autograd over flow-graph blocks: y, state_out = run(prog, x, state, params, consts).

The forward is Program.run_block with the library's default plan (the fast kernel); the backward is Program.run_block_grad, the
generated adjoint kernel (include/flowz_hip.h: fz_run_block_grad).  Differentiable in x, state, params and consts; chaining run()
over consecutive blocks back-propagates through time across them (the state gradient of block k is the state_out gradient of block
k-1).  Time-major frames [T, n_streams, n_in] (or [T, n_streams] for one input wire) on the GPU; there is no CPU path.
run(..., stream_major=True) takes stream-major tensors instead, [n_streams, T, n_in] or [n_streams, T] -- a [batch, time] tensor as it
lies: the forward is Program.run_block_stream_major, the backward Program.run_block_grad_stream_major, and nothing is transposed.

run_rings(prog, x, state, params, consts) is run() for graphs with delay lines deeper than 8 samples (combs, echoes, plucked strings):
time-major frames, the backward is Program.run_block_ring_grad (include/flowz_hip.h: fz_run_block_ring_grad).  run() keeps refusing them.
run_rings(..., stream_major=True) takes the stream-major tensors of run(..., stream_major=True): the forward is
Program.run_block_stream_major, the backward Program.run_block_ring_grad_stream_major, and nothing is transposed.

run_far(prog, x, state, params, consts) is run_rings() for graphs with delay lines deeper than 256 samples as well (echoes, reverb
combs, low plucked strings), whose rings live in HBM: time-major frames, the backward is Program.run_block_far_grad
(include/flowz_hip.h: fz_run_block_far_grad).  The rows of such a line in `state` are ring slots and one more row holds the phase: a
zero state has phase 0, and the state gradient's phase rows are zero.  run_rings() keeps refusing such graphs.
run_far(..., stream_major=True) takes the stream-major tensors of run(..., stream_major=True): the forward is
Program.run_block_far_stream_major, the backward Program.run_block_far_grad_stream_major, both on the tensors as they lie: nothing is
transposed.

mse(prog, x, target, ...) is the mean squared error of one block against a target as ONE launch (Program.run_block_loss_grad:
the adjoint kernel forms y, the error and dL/dy itself), where run() followed by ((y - target) ** 2).mean() is a forward launch,
several elementwise kernels and the backward launch.

mse_rings(prog, x, target, ...) is mse() for every graph run_rings() takes, time-major (Program.run_block_ring_loss_grad: the ring
adjoint kernel with the loss formed in it); mse() keeps refusing graphs with delay lines deeper than 8 samples.
mse_rings(..., stream_major=True) is the same on stream-major tensors (Program.run_block_ring_loss_grad_stream_major).

mse_far(prog, x, target, ...) is mse_rings() for every graph run_far() takes, time-major (Program.run_block_far_loss_grad).
mse_far(..., stream_major=True) is the same on stream-major tensors (Program.run_block_far_loss_grad_stream_major): one launch on a
[batch, time] tensor as it lies, no forward launch and nothing transposed.

mse_recording(prog, x, target, ...) is the same loss over a whole recording of many blocks in bounded workspace
(Program.run_recording_loss_grad: one forward launch that keeps the state before every block, then the loss kernel block by block
from the last to the first), and also returns the state after the recording.

mse_recording_rings(prog, x, target, ...) is mse_recording() for every graph run_rings() takes, time-major
(Program.run_recording_ring_loss_grad: the ring states kernel, then the ring loss kernel block by block); mse_recording() keeps refusing
graphs with delay lines deeper than 8 samples.
mse_recording_rings(..., stream_major=True) is the same on stream-major tensors (Program.run_recording_ring_loss_grad_stream_major):
a batch of recordings lying as [batch, time] is fitted in bounded workspace without a transposed copy.

mse_recording_far(prog, x, target, ...) is mse_recording_rings() for every graph run_far() takes, time-major
(Program.run_recording_far_loss_grad: the far states kernel, then the far loss kernel block by block); mse_recording_rings() keeps
refusing graphs with delay lines deeper than 256 samples.
mse_recording_far(..., stream_major=True) is the same on stream-major tensors (Program.run_recording_far_loss_grad with
stream_major=True): a batch of recordings lying as [batch, time] is fitted in bounded workspace without a transposed copy.
"""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from .flowz import FlowzError, Program
from . import _capi as C


def _apply_consts(prog: Program, consts):
    if consts is None:
        return
    for k, v in enumerate(consts.tolist()):
        prog.set_const(k, v)


def _front_door(prog: Program, x, consts, rings):
    """the checks every public function starts with, in this order: the graph is supported, 2-D frames have one input wire, consts fit.
    rings: False (the plain family), True (the ring family) or "far" (the far family)"""
    if rings == "far":
        if not prog.far_grad_supported():
            raise FlowzError(C.FZ_E_UNSUPPORTED, prog.far_grad_unsupported_reason())
    elif rings:
        if not prog.ring_grad_supported():
            raise FlowzError(C.FZ_E_UNSUPPORTED, prog.ring_grad_unsupported_reason())
    elif not prog.grad_supported():
        raise FlowzError(C.FZ_E_UNSUPPORTED, prog.grad_unsupported_reason())
    if x.dim() == 2 and prog.n_in != 1:
        raise FlowzError(C.FZ_E_INVALID, f"x: two-dimensional frames are for one input wire, the graph has {prog.n_in}")
    if consts is not None:
        if consts.device.type != "cpu" or consts.dtype != torch.float32 or tuple(consts.shape) != (prog.n_const,):
            raise FlowzError(C.FZ_E_INVALID, f"consts: a CPU float32 tensor of shape ({prog.n_const},)")


def _backward_call(prog: Program, rings, stream_major, loss=False, recording=False):
    """the bound Program method of one corner of the backward family"""
    name = ("run_recording_" if recording else "run_block_") + ("far_" if rings == "far" else "ring_" if rings else "") + ("loss_grad" if loss else "grad")
    # (the plain and the far recording calls take the layout as a keyword; every other stream-major corner is a method of its own)
    return getattr(prog, name + ("_stream_major" if stream_major and (rings is True or not recording) else ""))


_WANT = ("x", "state", "params", "consts")


def _want(needs):
    """the gradients to ask the launch for, from needs_input_grad of (x, state, params, consts)"""
    return [k for k, n in zip(_WANT, needs) if n]


def _grads(prog: Program, r, needs, x_shape, consts):
    """(dx, dstate, dparams, dconsts) from the dict a launch returned, None where not needed"""
    need_x, need_s, need_p, need_c = needs
    return (r["x"].reshape(x_shape) if need_x else None, r["state"] if need_s else None, r["params"] if need_p else None,
            # per-stream coefficient adjoints, summed over the streams in float64
            r["consts"][:prog.n_const].double().sum(1).to(consts.dtype).to(consts.device) if need_c else None)


class _Block(torch.autograd.Function):
    @staticmethod
    def forward(ctx, prog, x, state, params, consts, stream_major=False, rings=False):
        _apply_consts(prog, consts)
        ctx.rings = rings
        st = state.detach().clone() if state is not None else None    # (the caller's state is never advanced in place)
        # (a line in HBM on stream-major buffers: the far forward call; for every other graph it is run_block_stream_major itself)
        fwd = prog.run_block if not stream_major else prog.run_block_far_stream_major if rings == "far" else prog.run_block_stream_major
        y, st = fwd(x.detach(), st, params.detach() if params is not None else None)
        ctx.prog = prog
        ctx.stream_major = stream_major
        ctx.consts = consts.detach().clone() if consts is not None else None
        ctx.x_shape = x.shape
        ctx.save_for_backward(x, state, params)
        return y, st

    @staticmethod
    @once_differentiable
    def backward(ctx, gy, gs):
        prog = ctx.prog
        x, state, params = ctx.saved_tensors
        needs = ctx.needs_input_grad[1:5]
        want = _want(needs)
        if not want:
            return None, None, None, None, None, None, None
        xx = x.detach() if x.dim() == 3 else x.detach().unsqueeze(-1)
        if gy is None:
            gy = torch.zeros(tuple(xx.shape[:2]) + (prog.n_out,), dtype=torch.float32, device=x.device)
        sg = gs.contiguous() if gs is not None and prog.n_state else None
        _apply_consts(prog, ctx.consts)                               # (the constants of the forward launch)
        r = _backward_call(prog, ctx.rings, ctx.stream_major)(
            xx, gy.contiguous(), state.detach() if state is not None else None,
            params.detach() if params is not None else None, state_grad=sg, want=want)
        return (None,) + _grads(prog, r, needs, ctx.x_shape, ctx.consts) + (None, None)


def _run(prog, x, state, params, consts, stream_major, rings):
    _front_door(prog, x, consts, rings)
    if state is None:
        state = torch.zeros((max(prog.n_state, 1), x.shape[0 if stream_major else 1]), dtype=torch.float32, device=x.device)
    return _Block.apply(prog, x, state, params, consts, bool(stream_major), rings)


def run(prog: Program, x, state=None, params=None, consts=None, stream_major=False):
    """One block through autograd: returns (y [T, n_streams, n_out], state after the block [n_state, n_streams]).
    stream_major: x is [n_streams, T, n_in] (or [n_streams, T] for one input wire) and y comes back as [n_streams, T, n_out].
    state: the state before the block (None: zeros; never modified), params: [n_param, n_streams] per-stream coefficients,
    consts: an optional CPU float32 tensor [n_const] of uniform coefficient slots (Program.consts() order), applied with
    set_const before the forward launch and again before the backward one (None: the program's current values, constant)."""
    return _run(prog, x, state, params, consts, stream_major, False)


def run_rings(prog: Program, x, state=None, params=None, consts=None, stream_major=False):
    """run() for graphs with delay lines deeper than 8 samples -- and every graph run() takes --, time-major frames: returns (y [T,
    n_streams, n_out], state after the block).  The forward is Program.run_block, the backward Program.run_block_ring_grad; x, state,
    params and consts as for run(), the uniform-coefficient gradients summed over the streams in float64 as there.  Chaining it over
    consecutive blocks back-propagates through time across them, whatever the blocks' lengths against the lines' depths.
    stream_major: the tensor shapes of run(..., stream_major=True) -- x [n_streams, T, n_in], or [n_streams, T] for one input wire --;
    the forward is Program.run_block_stream_major, the backward Program.run_block_ring_grad_stream_major."""
    return _run(prog, x, state, params, consts, stream_major, True)


def run_far(prog: Program, x, state=None, params=None, consts=None, stream_major=False):
    """run_rings() for graphs with delay lines deeper than 256 samples -- and every graph run_rings() takes --, time-major frames:
    returns (y [T, n_streams, n_out], state after the block).  The forward is Program.run_block, the backward
    Program.run_block_far_grad.  The rows of a line deeper than 256 samples are ring slots in `state` and in its gradient, and the
    line's phase row (behind all line rows) is 0 in a zero state and has a zero gradient.  Chaining it over consecutive blocks
    back-propagates through time across them: the state after a block carries the phase the next block starts from.
    stream_major: the tensor shapes of run(..., stream_major=True) -- x [n_streams, T, n_in], or [n_streams, T] for one input wire, y
    [n_streams, T, n_out].  The forward is Program.run_block_far_stream_major, the backward Program.run_block_far_grad_stream_major,
    both on the tensors as they lie: neither costs an extra pass, and y has the bits of the time-major call's y transposed.  The
    state rows are [row, n_streams] in either layout, so blocks chain as in the time-major call."""
    return _run(prog, x, state, params, consts, stream_major, "far")


class _Mse(torch.autograd.Function):
    """the loss of one block, or (block_rows not None) of a whole recording, which also returns the state after it"""

    @staticmethod
    def forward(ctx, prog, x, target, state, params, consts, stream_major, rings, block_rows):
        _apply_consts(prog, consts)
        recording = block_rows is not None
        needs = (ctx.needs_input_grad[1],) + tuple(ctx.needs_input_grad[3:6])
        want = ["loss"] + (["state_out"] if recording else []) + _want(needs)
        xx = x.detach() if x.dim() == 3 else x.detach().unsqueeze(-1)
        n = xx.shape[0] * xx.shape[1] * prog.n_out                    # elements of y: the mean is over all of them
        kw = {}
        if recording:
            kw = {"block_rows": int(block_rows)} if rings is True else {"block_rows": int(block_rows), "stream_major": bool(stream_major)}
        # the one call: the loss and every gradient asked for, dL/dy = (y - target) * 2 / n formed in the kernel
        r = _backward_call(prog, rings, stream_major, True, recording)(
            xx, target.detach().contiguous(), state.detach() if state is not None else None,
            params.detach() if params is not None else None, grad_scale=2.0 / n, want=want, **kw)
        ctx.grads = _grads(prog, r, needs, x.shape, consts)
        loss = (r["loss"].double().sum() / n).to(torch.float32)       # per-stream sums of e * e, summed over the streams in float64
        if not recording:
            return loss
        ctx.mark_non_differentiable(r["state_out"])
        return loss, r["state_out"]

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _gs=None):
        scaled = lambda t: None if t is None else t * g.to(t.device)   # noqa: E731  (the upstream scalar on what the forward launch left)
        gx, gs, gp, gc = map(scaled, ctx.grads)
        return None, gx, None, gs, gp, gc, None, None, None


def mse(prog: Program, x, target, state=None, params=None, consts=None, stream_major=False):
    """The mean squared error ((y - target) ** 2).mean() of ONE block y = run(prog, x, state, params, consts)[0], as a scalar tensor,
    differentiable in x, state, params and consts (not in target).  One launch, made in the forward (Program.run_block_loss_grad,
    include/flowz_hip.h: fz_run_block_loss_grad): y and dL/dy never cross HBM, dL/dx is computed only if x requires a gradient, and
    backward() applies the upstream scalar to the gradients that launch left.  x, state, params, consts and stream_major as for
    run(); target is laid out like y.  It covers one block and does not return the state after it: chaining blocks stays with run()."""
    _front_door(prog, x, consts, False)
    return _Mse.apply(prog, x, target, state, params, consts, bool(stream_major), False, None)


def mse_rings(prog: Program, x, target, state=None, params=None, consts=None, stream_major=False):
    """mse() for graphs with delay lines deeper than 8 samples -- and every graph mse() takes --, time-major frames: the scalar
    ((y - target) ** 2).mean() of one block, differentiable in x, state, params and consts.  One launch, made in the forward
    (Program.run_block_ring_loss_grad, include/flowz_hip.h: fz_run_block_ring_loss_grad); backward() applies the upstream scalar.
    stream_major: the tensor shapes of mse(..., stream_major=True), a [batch, time] tensor as it lies for one wire
    (Program.run_block_ring_loss_grad_stream_major)."""
    _front_door(prog, x, consts, True)
    return _Mse.apply(prog, x, target, state, params, consts, bool(stream_major), True, None)


def mse_far(prog: Program, x, target, state=None, params=None, consts=None, stream_major=False):
    """mse_rings() for graphs with delay lines deeper than 256 samples -- and every graph mse_rings() takes --, time-major frames:
    the scalar ((y - target) ** 2).mean() of one block, differentiable in x, state, params and consts.  One launch, made in the forward
    (Program.run_block_far_loss_grad, include/flowz_hip.h: fz_run_block_far_loss_grad); backward() applies the upstream scalar.
    stream_major: the tensor shapes of mse(..., stream_major=True), a [batch, time] tensor as it lies for one wire: one launch of
    Program.run_block_far_loss_grad_stream_major, no forward launch, nothing transposed."""
    _front_door(prog, x, consts, "far")
    return _Mse.apply(prog, x, target, state, params, consts, bool(stream_major), "far", None)


def mse_recording(prog: Program, x, target, state=None, params=None, consts=None, block_rows=0, stream_major=False):
    """mse() over a whole RECORDING: returns (loss, state_out).  loss is ((y - target) ** 2).mean() over all rows of x, differentiable as
    mse() is; state_out is the state after the last row, detached, so the caller can continue the stream (pass it as `state` of the
    next call).  The workspace is bounded (Program.recording_workspace_bytes: the state before every block of block_rows rows plus
    one block's checkpoints; block_rows = 0 lets the library choose), where mse() over the same rows keeps a checkpoint every few rows
    of the whole recording.  The gradients have the bits of mse()'s over the same rows.  Time-major frames need block_rows % 4 == 0."""
    _front_door(prog, x, consts, False)
    loss, state_out = _Mse.apply(prog, x, target, state, params, consts, bool(stream_major), False, int(block_rows))
    return loss, state_out.detach()


def mse_recording_rings(prog: Program, x, target, state=None, params=None, consts=None, block_rows=0, stream_major=False):
    """mse_recording() for graphs with delay lines deeper than 8 samples -- and every graph mse_recording() takes --, time-major frames:
    returns (loss, state_out) over a whole recording in bounded workspace (Program.ring_recording_workspace_bytes: the state before every
    block plus one block's checkpoints and tape; block_rows = 0 lets the library choose, otherwise a multiple of 4).  The gradients
    have the bits of mse_rings()'s over the same rows (include/flowz_hip.h: fz_run_recording_ring_loss_grad).
    stream_major: the tensor shapes of mse_recording(..., stream_major=True), a [batch, time] tensor as it lies for one wire
    (Program.run_recording_ring_loss_grad_stream_major); block_rows times n_in and n_out are then multiples of 4."""
    _front_door(prog, x, consts, True)
    loss, state_out = _Mse.apply(prog, x, target, state, params, consts, bool(stream_major), True, int(block_rows))
    return loss, state_out.detach()


def mse_recording_far(prog: Program, x, target, state=None, params=None, consts=None, block_rows=0, stream_major=False):
    """mse_recording_rings() for graphs with delay lines deeper than 256 samples -- and every graph mse_recording_rings() takes --,
    time-major frames: returns (loss, state_out) over a whole recording in bounded workspace
    (Program.far_recording_workspace_bytes: the state before every block plus one block's checkpoints, tape and adjoint ring;
    block_rows = 0 lets the library choose, otherwise a multiple of 4).  The gradients have the bits of mse_far()'s over the same rows
    (include/flowz_hip.h: fz_run_recording_far_loss_grad); state_out carries the far lines' slots and phase rows, so it is the `state`
    of the next call.
    stream_major: the tensor shapes of mse_recording(..., stream_major=True), a [batch, time] tensor as it lies for one wire
    (Program.run_recording_far_loss_grad(stream_major=True), fz_run_recording_far_loss_grad_for); block_rows times n_in and n_out are
    then multiples of 4.  The forward needs no stream-major body for rings in HBM: the recording call yields the loss and state_out
    itself, nothing is transposed."""
    _front_door(prog, x, consts, "far")
    loss, state_out = _Mse.apply(prog, x, target, state, params, consts, bool(stream_major), "far", int(block_rows))
    return loss, state_out.detach()
