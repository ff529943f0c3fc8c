#!/usr/bin/env python3
"""Times blocks with 16-bit PCM frames (fz_run_block_pcm16) against the library's float32 default on the MI355X.

Not part of bench.py.  The 6-biquad cascade (zignal_amd/workloads.py) at 1 048 576 x 4096 and 65 536 x 4096 (streams x samples),
four cases on the same signal: int16 -> int16, int16 -> float32, float32 -> int16 (Program.run_block_pcm16) and float32 -> float32
(Program.run_block, the library's default plan).  One process, cases interleaved: the float32 default runs for at least 100 ms first
(the boards are power-managed), then every case is timed --steps times in a forward and again in a backward pass over the list, HIP
events around each launch.  Printed per case: ms per block (median; min .. max), GSamples/s, the fraction of 8 TB/s on that case's OWN
algorithmic bytes (streams x samples x (n_in x bytes in + n_out x bytes out)), the ratio of its samples/s to the float32 default of
the same run, and the kernel.

The host path the same way: Bank.process_host_pcm16 against Bank.process_host on pinned host frames, alternating.

--layout stream-major times the same cases on stream-major buffers [stream][row][wire] (a [batch, time] tensor as it lies):
Program.run_block_pcm16_stream_major against Program.run_block_stream_major, Bank.process_host_pcm16_stream_major against
Bank.process_host_stream_major; uniform noise at half of full scale as the signal; the record goes to
profiles/r10/pcm16_stream_major.txt.  Without the option nothing changes.

usage: tools/pcm16_bench.py [--steps K] [--shapes large|small|all] [--host-rows T] [--layout time-major|stream-major] [--out FILE]
"""
import argparse
import datetime
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from zignal_amd import flowz as F  # noqa: E402
from zignal_amd import workloads as W  # noqa: E402

SHAPES = {"large": [(1 << 20, 4096)], "small": [(65536, 4096)]}
HBM = 8e12
CASES = (("i16->i16", "int16", "int16"), ("i16->f32", "int16", "float32"), ("f32->i16", "float32", "int16"), ("f32->f32", "float32", "float32"))
SIZE = {"int16": 2, "float32": 4}

_lines = []


def say(s=""):
    print(s, flush=True)
    _lines.append(s)


def samples(fn, steps, torch):
    out = []
    for _ in range(steps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        out.append(t0.elapsed_time(t1))
    return out


def device_cases(a, torch, prog):
    say(f"# device path: one block per launch, HIP events, {a.steps} launches per case and pass, a forward and a backward pass over the cases")
    say(f"{'streams x T':>16s} {'case':>9s} {'ms':>8s} {'min':>8s} {'max':>8s} {'GSamples/s':>11s} {'B/sample':>9s} {'of 8 TB/s':>10s} {'vs f32':>7s}  kernel")
    shapes = SHAPES["large"] + SHAPES["small"] if a.shapes == "all" else SHAPES[a.shapes]
    sm = a.layout == "stream-major"
    for ns, T in shapes:
        shape = (ns, T, 1) if sm else (T, ns, 1)
        xf = torch.empty(shape, dtype=torch.float32, device="cuda")
        xq = torch.empty(shape, dtype=torch.int16, device="cuda")
        if sm:
            torch.manual_seed(W.SEED)
            step = 16384                                     # streams per slice
            for i in range(0, ns, step):
                xf[i:i + step].uniform_(-0.5, 0.5)
        else:
            F.synth_fill(xf, seed=W.SEED)
            step = 256                                       # rows per slice
        for t0 in range(0, shape[0], step):                  # the same signal on both sides: q = round(32767 x), x = q / 32768
            xq[t0:t0 + step] = torch.round(xf[t0:t0 + step] * 32767.0).to(torch.int16)
            xf[t0:t0 + step] = xq[t0:t0 + step].to(torch.float32) * (1.0 / 32768.0)
        yf = torch.empty(shape, dtype=torch.float32, device="cuda")
        yq = torch.empty(shape, dtype=torch.int16, device="cuda")
        s0 = torch.zeros((prog.n_state, ns), dtype=torch.float32, device="cuda")
        legs, names = {}, {}
        for case, it, ot in CASES:
            x, y = (xq if it == "int16" else xf), (yq if ot == "int16" else yf)
            if case == "f32->f32" and sm:
                legs[case] = lambda x=x, y=y: prog.run_block_stream_major(x, state=s0, out=y)
                names[case] = prog.kernel_symbol(F.make_variant(0, 0, 0, F.C.FZ_VF_STREAM_MAJOR), ns, T)
            elif sm:
                legs[case] = lambda x=x, y=y, ot=ot: prog.run_block_pcm16_stream_major(x, state=s0, out=y, out_dtype=ot)
                names[case] = prog.pcm16_stream_major_kernel_symbol(it, ot)
            elif case == "f32->f32":
                legs[case] = lambda x=x, y=y: prog.run_block(x, state=s0, out=y)
                names[case] = prog.kernel_symbol(None, ns, T)
            else:
                legs[case] = lambda x=x, y=y, ot=ot: prog.run_block_pcm16(x, state=s0, out=y, out_dtype=ot)
                names[case] = prog.pcm16_kernel_symbol(it, ot, ns)
        for f in legs.values():                              # code objects, allocator
            f()
        torch.cuda.synchronize()
        t_end = time.time() + 0.1
        while time.time() < t_end:                           # at least 100 ms of the default before the first timing
            legs["f32->f32"]()
            torch.cuda.synchronize()
        got = {k: [] for k in legs}
        for order in (list(legs), list(legs)[::-1]):
            for k in order:
                got[k] += samples(legs[k], a.steps, torch)
        med = {k: float(np.median(v)) for k, v in got.items()}
        for case, it, ot in CASES:
            bps = prog.n_in * SIZE[it] + prog.n_out * SIZE[ot]
            rate = ns * T / (med[case] / 1e3)
            say(f"{f'{ns} x {T}':>16s} {case:>9s} {med[case]:8.3f} {min(got[case]):8.3f} {max(got[case]):8.3f} {rate / 1e9:11.1f} {bps:9d} "
                f"{rate * bps / HBM:10.3f} {med['f32->f32'] / med[case]:7.3f}  {names[case]}")
        say("#   all timings ms: " + "; ".join(f"{k} " + " ".join(f"{t:.3f}" for t in v) for k, v in got.items()))
        del xf, xq, yf, yq, s0, legs
        torch.cuda.empty_cache()


def host_cases(a, torch, prog):
    ns, T = 65536, a.host_rows
    say()
    say(f"# host path: pinned host frames in and out, wall clock around each call (it returns when the output is on the host), {a.steps} calls each, alternating")
    say(f"{'streams x T':>16s} {'call':>20s} {'ms':>9s} {'min':>9s} {'max':>9s} {'GSamples/s':>11s} {'PCIe B/sample':>14s} {'vs float32':>11s}")
    sm = a.layout == "stream-major"
    shape = (ns, T, 1) if sm else (T, ns, 1)
    q = torch.from_numpy(np.random.default_rng(1).integers(-32768, 32768, shape, dtype=np.int16)).pin_memory()
    x = (q.to(torch.float32) * (1.0 / 32768.0)).pin_memory()
    oq = torch.empty(shape, dtype=torch.int16).pin_memory()
    of = torch.empty(shape, dtype=torch.float32).pin_memory()
    bq, bf = prog.bank(ns), prog.bank(ns)
    if sm:
        legs = {"process_host": lambda: bf.process_host_stream_major(x, out=of), "process_host_pcm16": lambda: bq.process_host_pcm16_stream_major(q, out=oq)}
    else:
        legs = {"process_host": lambda: bf.process_host(x, out=of), "process_host_pcm16": lambda: bq.process_host_pcm16(q, out=oq)}
    for f in legs.values():
        f()
    got = {k: [] for k in legs}
    for _ in range(a.steps):
        for k, f in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            got[k].append((time.perf_counter() - t0) * 1e3)
    med = {k: float(np.median(v)) for k, v in got.items()}
    for k, nbytes in (("process_host", 8), ("process_host_pcm16", 4)):
        say(f"{f'{ns} x {T}':>16s} {k:>20s} {med[k]:9.2f} {min(got[k]):9.2f} {max(got[k]):9.2f} {ns * T / (med[k] / 1e3) / 1e9:11.2f} {nbytes:14d} "
            f"{med['process_host'] / med[k]:11.3f}")
    say("#   all timings ms: " + "; ".join(f"{k} " + " ".join(f"{t:.2f}" for t in v) for k, v in got.items()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--shapes", choices=("large", "small", "all"), default="all")
    ap.add_argument("--host-rows", type=int, default=2048)
    ap.add_argument("--layout", choices=("time-major", "stream-major"), default="time-major")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sm = a.layout == "stream-major"
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "r10", "pcm16_stream_major.txt") if sm else os.path.join(ROOT, "profiles", "r09", "pcm16.txt")
    import torch

    assert torch.cuda.is_available(), "pcm16_bench needs an MI355X: there is nothing to time without one"
    torch.cuda.set_device(0)
    props = torch.cuda.get_device_properties(0)
    prog = F.compile(F.from_sexpr(W.df1_cascade(6)))
    say(f"# 16-bit PCM frames against the float32 default: the 6-biquad cascade, {'stream-major buffers' if sm else 'time-major frames'} (tools/pcm16_bench.py{' --layout stream-major' if sm else ''})")
    say(f"# date {datetime.date.today().isoformat()}, board {props.name or 'unnamed'} ({getattr(props, 'gcnArchName', '?')})")
    for it, ot in (("int16", "int16"), ("int16", "float32"), ("float32", "int16")):
        r = prog.pcm16_stream_major_resources(it, ot) if sm else prog.pcm16_resources(it, ot, 1 << 20)
        say(f"# {prog.pcm16_stream_major_kernel_symbol(it, ot) if sm else prog.pcm16_kernel_symbol(it, ot, 1 << 20)}: {r['vgprs'] + r['agprs']} vgprs, {r['sgprs']} sgprs, {r['lds_bytes']} B LDS, {r['scratch_bytes']} B scratch, chunks of {r['unroll']} rows")
    device_cases(a, torch, prog)
    host_cases(a, torch, prog)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(_lines) + "\n")


if __name__ == "__main__":
    main()
