#!/usr/bin/env python3
"""Times the backward of a block (fz_run_block_grad, the adjoint kernel) against its forward on the MI355X.

Not part of bench.py.  For df1_cascade_params(6) and the Moog ladder at 65 536 x 4096 and 1 048 576 x 1024 (streams x samples): the
forward is Program.run_block on the library's default plan, the backward Program.run_block_grad with every gradient and the default
checkpoint stride.  HIP events around each launch after warm-up; printed per leg: ms (median), the ratio backward / forward, the
adjoint kernel's registers, and its HBM traffic per the formula of DESIGN.md (4 (2 n_in + n_out + n_in) + 8 n_state / C bytes per
stream-sample, plus the coefficient rows) as a fraction of 8 TB/s.

usage: tools/grad_bench.py [--warmup W] [--steps K] [--legs small|large|all]
"""
import argparse
import datetime
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from zignal_amd import flowz as F  # noqa: E402
from zignal_amd import workloads as W  # noqa: E402

GRAPHS = {"df1_cascade_params6": lambda: W.df1_cascade_params(6), "moog_ladder": W.moog_ladder}
SHAPES = {"small": [(65536, 4096)], "large": [(1 << 20, 1024)]}
HBM = 8e12


def params_for(name, prog, ns, torch):
    rng = np.random.default_rng(1)
    if name == "moog_ladder":
        p = rng.uniform(0.05, 0.5, (1, ns))
    else:
        p = np.repeat(np.tile(np.asarray(W.STABLE, np.float64), prog.n_param // 5)[:, None], ns, 1) * rng.uniform(0.9, 1.0, (prog.n_param, ns))
    return torch.from_numpy(p.astype(np.float32)).cuda()


def timed(fn, warmup, steps, torch):
    times = []
    for k in range(warmup + steps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        if k >= warmup:
            times.append(t0.elapsed_time(t1))
    return float(np.median(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--legs", choices=("small", "large", "all"), default="all")
    a = ap.parse_args()
    import torch

    torch.cuda.set_device(0)
    props = torch.cuda.get_device_properties(0)
    print(f"# backward vs forward of one block, HIP events, median of {a.steps} launches after {a.warmup} warm-up")
    print(f"# date {datetime.date.today().isoformat()}, board {props.name or 'unnamed'} ({getattr(props, 'gcnArchName', '?')})")
    print(f"{'graph':20s} {'streams x T':>16s} {'fwd ms':>9s} {'bwd ms':>9s} {'bwd/fwd':>8s} {'C':>3s} {'vgprs':>6s} {'bwd B/s / 8TB/s':>16s}  adjoint kernel")
    shapes = SHAPES["small"] + SHAPES["large"] if a.legs == "all" else SHAPES[a.legs]
    for ns, T in shapes:
        x = torch.empty((T, ns, 1), dtype=torch.float32, device="cuda")
        F.synth_fill(x, seed=W.SEED)
        gy = torch.empty_like(x)
        F.synth_fill(gy, seed=W.SEED + 1)
        y = torch.empty_like(x)
        for name, fn in GRAPHS.items():
            prog = F.compile(F.from_sexpr(fn()))
            pp = params_for(name, prog, ns, torch)
            s0 = torch.zeros((prog.n_state, ns), dtype=torch.float32, device="cuda")
            st = s0.clone()

            def fwd():
                st.copy_(s0)
                prog.run_block(x, state=st, params=pp, out=y)
            fwd_ms = timed(fwd, a.warmup, a.steps, torch)
            # (the state copy is inside the forward's window: n_state rows, < 1 % of a block's bytes)
            bwd_ms = timed(lambda: prog.run_block_grad(x, gy, s0, pp, state_grad=s0), a.warmup, a.steps, torch)
            res = prog.grad_resources()
            C = res["unroll"]
            nbytes = 4.0 * ns * T * (2 * prog.n_in + prog.n_out + prog.n_in) + 8.0 * ns * T * prog.n_state / C \
                + 4.0 * ns * (2 * prog.n_state + prog.n_param * 2 + prog.n_const * 2)
            print(f"{name:20s} {f'{ns} x {T}':>16s} {fwd_ms:9.3f} {bwd_ms:9.3f} {bwd_ms / fwd_ms:8.2f} {C:3d} {res['vgprs'] + res['agprs']:6d} "
                  f"{nbytes / (bwd_ms / 1e3) / HBM:16.3f}  {prog.grad_kernel_symbol()}", flush=True)
            del pp, s0, st
        del x, gy, y
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
