#!/usr/bin/env python3
"""Example: fit_echo_feedback.py over a whole recording -- the per-stream feedback gain of an ECHO with a delay line of 300 samples,
deeper than the 256 samples a ring in LDS holds, fitted with Adam to recordings of 16 384 samples, several blocks each, in bounded
workspace.

y[t] = g * y[t-300] + x[t], one gain `g` per stream.  autograd.mse_recording_far() is mse_far() over a recording: one launch of the
far states kernel runs the recording forward -- the line's ring lives in the workspace, in the caller's own slot format -- and keeps
only the state before every block, then the far loss kernel differentiates the blocks from the last to the first
(run_recording_far_loss_grad).  The loss and the gradients have the bits of mse_far() over the same rows; the workspace holds the
block starts and ONE block's tape, where mse_far() keeps the tape of every row.  A block start costs the line's 300 slots and its
phase row, so the blocks are long.  It also returns the state after the recording -- slots and phase --, so the stream can be
continued.  Time-major frames [time, streams]."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zignal_amd import autograd as AG      # noqa: E402
from zignal_amd import flowz as F          # noqa: E402
from zignal_amd.flowz import _1, _2        # noqa: E402

_300 = F.placeholder(300)
prog = F.compile(~(F.param(0) * _1[_300] + _2))                # _1: the fed-back output, _2: the input wire
time, streams = 16384, 4096
gen = torch.Generator(device="cuda").manual_seed(1)
x = torch.randn((time, streams), device="cuda", generator=gen)
g_true = torch.rand((1, streams), device="cuda", generator=gen) * 0.7 + 0.2
target, _ = prog.run_block(x, None, g_true)                    # [time, streams, 1]

B = prog.far_recording_block_rows(time)
print(f"{time} rows in {-(-time // B)} blocks of {B}: workspace {prog.far_recording_workspace_bytes(streams, time) / 2**20:.1f} MB "
      f"against {prog.far_grad_workspace_bytes(streams, time) / 2**20:.1f} MB for one launch")
g = torch.full((1, streams), 0.5, device="cuda", requires_grad=True)
opt = torch.optim.Adam([g], lr=0.05)
for step in range(50):
    opt.zero_grad()
    loss, state_out = AG.mse_recording_far(prog, x, target, None, g)
    loss.backward()
    opt.step()
    if step % 10 == 0 or step == 49:
        print(f"step {step:2d}  loss {loss.item():.6f}  mean |g - g_true| {(g.detach() - g_true).abs().mean().item():.4f}")
print("states kernel:", prog.far_states_kernel_symbol(), " loss kernel:", prog.far_loss_grad_kernel_symbol())
