#!/usr/bin/env python3
"""Example: the per-stream feedback gain of an ECHO -- a delay line of 300 samples, deeper than the 256 samples a ring in LDS holds --
fitted to a batch of recordings with Adam, ONE launch per step.

y[t] = g * y[t-300] + x[t], one gain `g` per stream.  autograd.mse_far() is mse_rings() for graphs with delay lines deeper than 256
samples: the line's ring lives in HBM, the far adjoint kernel keeps its pending adjoints in a ring in the workspace, and it forms y,
the error and dL/dy itself (run_block_far_loss_grad), so neither y nor dL/dy crosses HBM.  The block is several echoes long, so that
the gain shows in the recording.  Time-major frames [time, streams]."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zignal_amd import autograd as AG      # noqa: E402
from zignal_amd import flowz as F          # noqa: E402
from zignal_amd.flowz import _1, _2        # noqa: E402

_300 = F.placeholder(300)
prog = F.compile(~(F.param(0) * _1[_300] + _2))                # _1: the fed-back output, _2: the input wire
time, streams = 2048, 4096
gen = torch.Generator(device="cuda").manual_seed(1)
x = torch.randn((time, streams), device="cuda", generator=gen)
g_true = torch.rand((1, streams), device="cuda", generator=gen) * 0.7 + 0.2
target, _ = prog.run_block(x, None, g_true)                    # [time, streams, 1]

g = torch.full((1, streams), 0.5, device="cuda", requires_grad=True)
opt = torch.optim.Adam([g], lr=0.05)
for step in range(50):
    opt.zero_grad()
    loss = AG.mse_far(prog, x, target, None, g)
    loss.backward()
    opt.step()
    if step % 10 == 0 or step == 49:
        print(f"step {step:2d}  loss {loss.item():.6f}  mean |g - g_true| {(g.detach() - g_true).abs().mean().item():.4f}")
print("adjoint kernel:", prog.far_loss_grad_kernel_symbol())
