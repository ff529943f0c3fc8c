#!/usr/bin/env python3
"""Example: fit_comb_feedback_fused.py from [batch, time] tensors as they lie -- the per-stream feedback gain of a comb filter with a
delay line of 23 samples, fitted to a batch of recordings with Adam, ONE launch per step and no transposition.

y[t] = g * y[t-23] + x[t], one gain `g` per stream.  autograd.mse_rings(..., stream_major=True) takes x and the target as
[batch, time]: the ring adjoint kernel for stream-major buffers (run_block_ring_loss_grad_stream_major) moves the frames through an LDS
patch next to the delay line's rings, so neither fz_transpose_frames of x and of the target nor of dL/dx back is needed; the bits are
those of the time-major call on the transposed tensors."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zignal_amd import autograd as AG      # noqa: E402
from zignal_amd import flowz as F          # noqa: E402
from zignal_amd.flowz import _1, _2        # noqa: E402

_23 = F.placeholder(23)
prog = F.compile(~(F.param(0) * _1[_23] + _2))                 # _1: the fed-back output, _2: the input wire
batch, time = 4096, 512
gen = torch.Generator(device="cuda").manual_seed(1)
x = torch.randn((batch, time), device="cuda", generator=gen)
g_true = torch.rand((1, batch), device="cuda", generator=gen) * 0.7 + 0.2
target, _ = prog.run_block_stream_major(x, None, g_true)       # [batch, time, 1]

g = torch.full((1, batch), 0.5, device="cuda", requires_grad=True)
opt = torch.optim.Adam([g], lr=0.05)
for step in range(50):
    opt.zero_grad()
    loss = AG.mse_rings(prog, x, target, None, g, stream_major=True)
    loss.backward()
    opt.step()
    if step % 10 == 0 or step == 49:
        print(f"step {step:2d}  loss {loss.item():.6f}  mean |g - g_true| {(g.detach() - g_true).abs().mean().item():.4f}")
print("adjoint kernel:", prog.ring_loss_grad_kernel_symbol(stream_major=True))
