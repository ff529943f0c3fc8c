#!/usr/bin/env python3
"""Example: fit_comb_feedback.py with the loss fused into the backward -- the per-stream feedback gain of a comb filter with a delay
line of 23 samples, fitted to a batch of recordings with Adam, ONE launch per step.

y[t] = g * y[t-23] + x[t], one gain `g` per stream.  autograd.mse_rings() is mse() for graphs with delay lines deeper than 8 samples:
the ring adjoint kernel re-evaluates every row anyway, so it forms y, the error and dL/dy itself (run_block_ring_loss_grad); neither y
nor dL/dy crosses HBM, where run_rings() followed by ((y - target) ** 2).mean() is a forward launch, several elementwise kernels and the
backward launch.  Time-major frames [time, streams]."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zignal_amd import autograd as AG      # noqa: E402
from zignal_amd import flowz as F          # noqa: E402
from zignal_amd.flowz import _1, _2        # noqa: E402

_23 = F.placeholder(23)
prog = F.compile(~(F.param(0) * _1[_23] + _2))                 # _1: the fed-back output, _2: the input wire
time, streams = 512, 4096
gen = torch.Generator(device="cuda").manual_seed(1)
x = torch.randn((time, streams), device="cuda", generator=gen)
g_true = torch.rand((1, streams), device="cuda", generator=gen) * 0.7 + 0.2
target, _ = prog.run_block(x, None, g_true)                    # [time, streams, 1]

g = torch.full((1, streams), 0.5, device="cuda", requires_grad=True)
opt = torch.optim.Adam([g], lr=0.05)
for step in range(50):
    opt.zero_grad()
    loss = AG.mse_rings(prog, x, target, None, g)
    loss.backward()
    opt.step()
    if step % 10 == 0 or step == 49:
        print(f"step {step:2d}  loss {loss.item():.6f}  mean |g - g_true| {(g.detach() - g_true).abs().mean().item():.4f}")
print("adjoint kernel:", prog.ring_loss_grad_kernel_symbol())
