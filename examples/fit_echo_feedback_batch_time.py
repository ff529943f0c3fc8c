#!/usr/bin/env python3
"""Example: fit_echo_feedback.py from [batch, time] tensors as they lie -- the per-stream feedback gain of an ECHO with a delay line
of 300 samples, fitted to a batch of recordings with Adam, ONE launch per step and no transposition.

y[t] = g * y[t-300] + x[t], one gain `g` per stream.  autograd.mse_far(..., stream_major=True) takes x and the target as
[batch, time]: the far adjoint kernel for stream-major buffers (run_block_far_loss_grad_stream_major) moves the frames through an LDS
patch while the line's values and pending adjoints stay in the workspace, one coalesced row per access, so neither
fz_transpose_frames of x and of the target nor of dL/dx back is needed; the bits are those of the time-major call on the transposed
tensors.  The target is made once with the layout adapter: the forward has no stream-major kernel body for rings in HBM."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zignal_amd import autograd as AG      # noqa: E402
from zignal_amd import flowz as F          # noqa: E402
from zignal_amd.flowz import _1, _2        # noqa: E402

_300 = F.placeholder(300)
prog = F.compile(~(F.param(0) * _1[_300] + _2))                # _1: the fed-back output, _2: the input wire
batch, time = 4096, 2048
gen = torch.Generator(device="cuda").manual_seed(1)
x = torch.randn((batch, time), device="cuda", generator=gen)
g_true = torch.rand((1, batch), device="cuda", generator=gen) * 0.7 + 0.2
y, _ = prog.run_block(F.frames_from_stream_major(x), None, g_true)
target = F.frames_to_stream_major(y)                           # [batch, time, 1]

g = torch.full((1, batch), 0.5, device="cuda", requires_grad=True)
opt = torch.optim.Adam([g], lr=0.05)
for step in range(50):
    opt.zero_grad()
    loss = AG.mse_far(prog, x, target, None, g, stream_major=True)
    loss.backward()
    opt.step()
    if step % 10 == 0 or step == 49:
        print(f"step {step:2d}  loss {loss.item():.6f}  mean |g - g_true| {(g.detach() - g_true).abs().mean().item():.4f}")
print("adjoint kernel:", prog.far_loss_grad_kernel_symbol(stream_major=True))
