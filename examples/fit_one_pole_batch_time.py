#!/usr/bin/env python3
"""Example: fit per-stream one-pole coefficients to a batch of recordings held as [batch, time] tensors, with Adam.

y[t] = a * y[t-1] + x[t], one coefficient `a` per recording.  The tensors stay stream-major from end to end, and a step is one
launch: autograd.mse(..., stream_major=True) runs the stream-major adjoint kernel that forms y, the error against the target and
dL/dy itself (run_block_loss_grad_stream_major).  Nothing is transposed, and neither y nor dL/dy is written to memory."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zignal_amd import autograd as AG      # noqa: E402
from zignal_amd import flowz as F          # noqa: E402
from zignal_amd.flowz import _1, _2        # noqa: E402

prog = F.compile(~(F.param(0) * _1[_1] + _2))                  # _1: the fed-back output, _2: the input wire
batch, time = 4096, 256
gen = torch.Generator(device="cuda").manual_seed(1)
x = torch.randn((batch, time), device="cuda", generator=gen)   # [batch, time]: one row per recording
a_true = torch.rand((1, batch), device="cuda", generator=gen) * 0.7 + 0.2
target, _ = prog.run_block_stream_major(x, None, a_true)       # [batch, time, 1]

a = torch.full((1, batch), 0.5, device="cuda", requires_grad=True)
opt = torch.optim.Adam([a], lr=0.05)
for step in range(50):
    opt.zero_grad()
    loss = AG.mse(prog, x, target, None, a, stream_major=True)
    loss.backward()
    opt.step()
    if step % 10 == 0 or step == 49:
        print(f"step {step:2d}  loss {loss.item():.6f}  mean |a - a_true| {(a.detach() - a_true).abs().mean().item():.4f}")
print("adjoint kernel:", prog.loss_grad_kernel_symbol(stream_major=True))
