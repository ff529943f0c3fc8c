#!/usr/bin/env python3
"""Example: fit_echo_feedback_recording.py from [batch, time] tensors as they lie -- the per-stream feedback gain of an ECHO with a
delay line of 300 samples, deeper than the 256 samples a ring in LDS holds, fitted with Adam to a batch of recordings of 16 384
samples, several blocks each, in bounded workspace and without a transposed copy of the frames.

y[t] = g * y[t-300] + x[t], one gain `g` per stream.  autograd.mse_recording_far(..., stream_major=True) takes x and the target as
[batch, time]: one launch of the far states kernel for stream-major buffers runs the recordings forward -- x moves through an LDS
patch, the line's ring lives in the workspace, one coalesced row per slot -- and keeps only the state before every block, then the
far loss kernel for stream-major buffers differentiates the blocks from the last to the first
(run_recording_far_loss_grad(stream_major=True)).  Neither fz_transpose_frames of x and of the target nor of dL/dx back is needed,
nor the two or three scratch buffers of the frames' size they would take; the bits are those of the time-major call on the
transposed tensors, so the figures printed are those of fit_echo_feedback_recording.py on the same draw.  The target is made once
with the layout adapter: the forward has no stream-major kernel body for rings in HBM."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zignal_amd import autograd as AG      # noqa: E402
from zignal_amd import flowz as F          # noqa: E402
from zignal_amd.flowz import _1, _2        # noqa: E402

_300 = F.placeholder(300)
prog = F.compile(~(F.param(0) * _1[_300] + _2))                # _1: the fed-back output, _2: the input wire
batch, time = 4096, 16384
gen = torch.Generator(device="cuda").manual_seed(1)
x = torch.randn((time, batch), device="cuda", generator=gen).t().contiguous()      # (the draw of fit_echo_feedback_recording.py, lying as [batch, time])
g_true = torch.rand((1, batch), device="cuda", generator=gen) * 0.7 + 0.2
y, _ = prog.run_block(F.frames_from_stream_major(x), None, g_true)
target = F.frames_to_stream_major(y)                           # [batch, time, 1]
del y

B = prog.far_recording_block_rows(time)
print(f"{time} rows in {-(-time // B)} blocks of {B}: workspace {prog.far_recording_workspace_bytes(batch, time) / 2**20:.1f} MB "
      f"against {prog.far_grad_workspace_bytes(batch, time) / 2**20:.1f} MB for one launch")
g = torch.full((1, batch), 0.5, device="cuda", requires_grad=True)
opt = torch.optim.Adam([g], lr=0.05)
for step in range(50):
    opt.zero_grad()
    loss, state_out = AG.mse_recording_far(prog, x, target, None, g, stream_major=True)
    loss.backward()
    opt.step()
    if step % 10 == 0 or step == 49:
        print(f"step {step:2d}  loss {loss.item():.6f}  mean |g - g_true| {(g.detach() - g_true).abs().mean().item():.4f}")
print("states kernel:", prog.far_states_kernel_symbol(stream_major=True), " loss kernel:", prog.far_loss_grad_kernel_symbol(stream_major=True))
