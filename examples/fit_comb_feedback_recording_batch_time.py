#!/usr/bin/env python3
"""Example: fit_comb_feedback_recording.py from a [batch, time] tensor as it lies -- the per-stream feedback gain of a comb filter with a
delay line of 23 samples, fitted with Adam to a batch of recordings of 4096 samples, several blocks each, in bounded workspace and
without a transposed copy of the frames.

y[t] = g * y[t-23] + x[t], one gain `g` per stream.  autograd.mse_recording_rings(..., stream_major=True) takes x and the target as
[batch, time]: one launch of the ring states kernel for stream-major buffers runs the recordings forward and keeps only the state before
every block, then the stream-major ring loss kernel differentiates the blocks from the last to the first
(run_recording_ring_loss_grad_stream_major).  The workspace is that of the time-major recording call -- the block starts and ONE
block's tape --, where the one-launch mse_rings(..., stream_major=True) keeps the tape of every row; and neither fz_transpose_frames of
x and of the target nor of dL/dx back is needed.  The draws are those of fit_comb_feedback_recording.py, transposed once up front, and
the bits are those of the time-major call on the transposed tensors: the two examples print the same loss curve."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zignal_amd import autograd as AG      # noqa: E402
from zignal_amd import flowz as F          # noqa: E402
from zignal_amd.flowz import _1, _2        # noqa: E402

_23 = F.placeholder(23)
prog = F.compile(~(F.param(0) * _1[_23] + _2))                 # _1: the fed-back output, _2: the input wire
batch, time = 4096, 4096
gen = torch.Generator(device="cuda").manual_seed(1)
x = torch.randn((time, batch), device="cuda", generator=gen).t().contiguous()      # [batch, time]
g_true = torch.rand((1, batch), device="cuda", generator=gen) * 0.7 + 0.2
target, _ = prog.run_block_stream_major(x, None, g_true)       # [batch, time, 1]

B = prog.ring_recording_block_rows(time)
print(f"{time} rows in {-(-time // B)} blocks of {B}: workspace {prog.ring_recording_workspace_bytes(batch, time) / 2**20:.1f} MB "
      f"against {prog.ring_grad_workspace_bytes(batch, time) / 2**20:.1f} MB for the one-launch call")
g = torch.full((1, batch), 0.5, device="cuda", requires_grad=True)
opt = torch.optim.Adam([g], lr=0.05)
for step in range(50):
    opt.zero_grad()
    loss, state_out = AG.mse_recording_rings(prog, x, target, None, g, stream_major=True)
    loss.backward()
    opt.step()
    if step % 10 == 0 or step == 49:
        print(f"step {step:2d}  loss {loss.item():.6f}  mean |g - g_true| {(g.detach() - g_true).abs().mean().item():.4f}")
print("states kernel:", prog.ring_states_kernel_symbol(stream_major=True), " loss kernel:", prog.ring_loss_grad_kernel_symbol(stream_major=True))
