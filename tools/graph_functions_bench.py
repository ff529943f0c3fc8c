#!/usr/bin/env python3
"""Times the graph-function workloads (zignal_amd.workloads: moog_ladder, soft_clip_cascade, envelope_follower, pm_operator, wavefolder,
log_compressor) on the MI355X.

Not part of bench.py.  Each graph runs at 1 048 576 streams x 4096 samples on the library's default plan (no variant), with HIP events
around each block after warm-up.  Printed per graph: ms per block (median of the timed blocks), GSamples/s, the bytes a block moves
(input and output frames, per-stream coefficients, state in and out) per second as a fraction of 8 TB/s, and the VALU instructions per
step of the kernel from tools/isa_stats.py (valu_per_step, at the default plan's streams per lane; two or four streams share a packed
instruction).

usage: tools/graph_functions_bench.py [--streams N] [--samples T] [--warmup W] [--steps K]
"""
import argparse
import datetime
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402

import isa_stats  # noqa: E402
from zignal_amd import flowz as F  # noqa: E402
from zignal_amd import workloads as W  # noqa: E402

GRAPHS = {"moog_ladder": W.moog_ladder, "soft_clip_cascade": W.soft_clip_cascade, "envelope_follower": W.envelope_follower,
          "pm_operator": W.pm_operator, "wavefolder": W.wavefolder, "log_compressor": W.log_compressor}
HBM = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=1 << 20)
    ap.add_argument("--samples", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    a = ap.parse_args()
    import torch

    torch.cuda.set_device(0)
    ns, T = a.streams, a.samples
    print(f"# graph functions: {ns} streams x {T} samples, default plan, HIP events, median of {a.steps} blocks after {a.warmup} warm-up")
    props = torch.cuda.get_device_properties(0)
    print(f"# date {datetime.date.today().isoformat()}, board {props.name or 'unnamed'} ({getattr(props, 'gcnArchName', '?')})")
    x = torch.empty((T, ns, 1), dtype=torch.float32, device="cuda")
    F.synth_fill(x, seed=W.SEED)
    out = torch.empty_like(x)
    print(f"{'graph':20s} {'kernel':44s} {'ms/block':>9s} {'GS/s':>8s} {'B/s / 8TB/s':>12s} {'VALU/step':>10s}")
    for name, fn in GRAPHS.items():
        e = fn()
        prog = F.compile(F.from_sexpr(e))
        params = torch.from_numpy((0.05 + 0.6 * np.random.default_rng(1).random((max(prog.n_param, 1), ns))).astype(np.float32)).cuda()
        pp = params[:prog.n_param] if prog.n_param else None
        state = torch.zeros((max(prog.n_state, 1), ns), dtype=torch.float32, device="cuda")
        kname = prog.kernel_name(None, ns, T)
        times = []
        for k in range(a.warmup + a.steps):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            prog.run_block(x, state=state, params=pp, out=out)
            t1.record()
            torch.cuda.synchronize()
            if k >= a.warmup:
                times.append(t0.elapsed_time(t1))
        ms = float(np.median(times))
        nbytes = 4.0 * ns * (T * (prog.n_in + prog.n_out) + prog.n_param + 2 * prog.n_state)
        P = prog.plan(ns).streams_per_lane or int(kname.split("_p")[1].split("u")[0])
        valu = isa_stats.valu_per_step(e, P)
        print(f"{name:20s} {kname:44s} {ms:9.3f} {ns * T / ms / 1e6:8.2f} {nbytes / (ms / 1e3) / HBM:12.3f} {valu:10.1f}  (P={P}, {P} streams per lane)")


if __name__ == "__main__":
    main()
