#!/usr/bin/env python3
"""Example: fit per-stream one-pole coefficients to whole recordings of many blocks, with Adam, in bounded workspace.

y[t] = a * y[t-1] + x[t], one coefficient `a` per recording, [batch, time] tensors as in fit_one_pole_batch_time.py -- but the
recordings are 4096 samples long.  autograd.mse over all of them would keep a checkpoint every 16 rows of the whole recording;
autograd.mse_recording runs the recording forward once keeping only the state before every block, then differentiates block by block
from the last to the first (run_recording_loss_grad): the same loss and the same gradient bits, a fraction of the workspace.  It also
returns the state after the last sample, so a longer stream can be fitted piece by piece."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zignal_amd import autograd as AG      # noqa: E402
from zignal_amd import flowz as F          # noqa: E402
from zignal_amd.flowz import _1, _2        # noqa: E402

prog = F.compile(~(F.param(0) * _1[_1] + _2))                  # _1: the fed-back output, _2: the input wire
batch, time = 4096, 4096
gen = torch.Generator(device="cuda").manual_seed(1)
x = torch.randn((batch, time), device="cuda", generator=gen)   # [batch, time]: one row per recording
a_true = torch.rand((1, batch), device="cuda", generator=gen) * 0.7 + 0.2
target, _ = prog.run_block_stream_major(x, None, a_true)       # [batch, time, 1]

print(f"{time} rows in blocks of {prog.recording_block_rows(time)}: workspace {prog.recording_workspace_bytes(batch, time, stream_major=True)} bytes, "
      f"one launch over all rows {prog.grad_workspace_bytes(batch, time)}")
a = torch.full((1, batch), 0.5, device="cuda", requires_grad=True)
opt = torch.optim.Adam([a], lr=0.05)
for step in range(50):
    opt.zero_grad()
    loss, state_after = AG.mse_recording(prog, x, target, None, a, stream_major=True)
    loss.backward()
    opt.step()
    if step % 10 == 0 or step == 49:
        print(f"step {step:2d}  loss {loss.item():.6f}  mean |a - a_true| {(a.detach() - a_true).abs().mean().item():.4f}")
print("states kernel:", prog.states_kernel_symbol(stream_major=True), " adjoint kernel:", prog.loss_grad_kernel_symbol(stream_major=True))
