#!/usr/bin/env python3
"""Dev tool (GPU box): the forward of graphs with delay lines in HBM on [batch, time] buffers -- fz_run_block_far_stream_major against
the route a caller had before it: fz_transpose_frames of x, fz_run_block, fz_transpose_frames of y back.  Both legs run in this
process, interleaved, ten times each after a warm-up; the medians are compared, the route's own spread (max - min over its ten) is
what "slower" is held against, and before anything is timed the two outputs and states are compared bit for bit.  Per stream-sample
the new call moves 4 n_in + 4 n_out + 4 n_far_lines + 4 n_far_reads bytes (its fraction of the 8 TB/s peak is printed); the route
moves 8 (n_in + n_out) more.

The last two default shapes have 28 rows behind the last whole chunk (R = 32): the tail reads its far values in front of each row.
The route's three calls sit inside one event pair; their host time is part of the route's figure.

    python tools/far_sm_forward_bench.py [--out profiles/r21/far_sm_forward.txt] [--reps 10] [--shapes 1048576x1024,65536x4096]"""
import argparse
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import far_grad_graphs as FG  # noqa: E402
from zignal_amd import flowz as F  # noqa: E402
from zignal_amd import workloads as W  # noqa: E402

PEAK = 8e12                                               # bytes per second, MI355X HBM3E
GRAPHS = {"far_comb": W.far_comb, "comb2000": lambda: W.far_comb(2000), "far_mixed": FG.far_mixed}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def measure(name, ns, T, reps, say):
    prog = F.compile(F.from_sexpr(GRAPHS[name]()))
    src = prog.far_stream_major_source()
    nfr, nfw = (int(re.search(r"#define %s (\d+)" % k, src).group(1)) for k in ("FZ_NFR", "FZ_NFW"))
    x = torch.randn((ns, T, prog.n_in), device="cuda") * 0.1
    par = torch.rand((prog.n_param, ns), device="cuda") * 0.5 + 0.3 if prog.n_param else None
    out, out_r = torch.zeros((ns, T, prog.n_out), device="cuda"), torch.zeros((ns, T, prog.n_out), device="cuda")
    fr, yf = torch.empty((T, ns, prog.n_in), device="cuda"), torch.empty((T, ns, prog.n_out), device="cuda")
    st, st_r = torch.zeros((prog.n_state, ns), device="cuda"), torch.zeros((prog.n_state, ns), device="cuda")

    def new():
        prog.run_block_far_stream_major(x, state=st, params=par, out=out)

    def route():
        F.frames_from_stream_major(x, 0, out=fr)
        prog.run_block(fr, state=st_r, params=par, out=yf)
        F.frames_to_stream_major(yf, out=out_r)

    new()
    route()
    torch.cuda.synchronize()
    equal = bool(torch.equal(out.view(torch.int32), out_r.view(torch.int32)) and torch.equal(st.view(torch.int32), st_r.view(torch.int32)))
    new()                                                 # (warm-up: the second launch of each)
    route()
    a, b = [], []
    for _ in range(reps):                                 # interleaved legs
        a.append(timed(new))
        b.append(timed(route))
    ma, mb = statistics.median(a), statistics.median(b)
    bytes_new = ns * T * 4 * (prog.n_in + prog.n_out + nfw + nfr)
    say(f"# {name}, {ns} streams x {T} rows, kernel {prog.far_stream_major_kernel_symbol()}, bits equal: {equal}")
    say(f"  new call  median {ma:8.3f} ms  (min {min(a):.3f} max {max(a):.3f})  {bytes_new / 1e9:6.2f} GB  {bytes_new / ma / 1e9:7.1f} TB/s  "
        f"{bytes_new / (ma * 1e-3) / PEAK:.3f} of peak")
    say(f"  route     median {mb:8.3f} ms  (min {min(b):.3f} max {max(b):.3f}, spread {max(b) - min(b):.3f})")
    say(f"  new / route {ma / mb:.3f}   {'SLOWER than the route beyond its spread' if ma > mb + (max(b) - min(b)) else 'not slower than the route'}")
    return equal


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--shapes", default="1048576x1024,65536x4096,1048576x1052,65536x4124")
    ap.add_argument("--graphs", default=",".join(GRAPHS))
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say(f"# tools/far_sm_forward_bench.py: fz_run_block_far_stream_major against transpose + fz_run_block + transpose; interleaved, medians of {args.reps}")
    ok = True
    for shape in args.shapes.split(","):
        ns, T = (int(v) for v in shape.split("x"))
        for name in args.graphs.split(","):
            ok = measure(name, ns, T, args.reps, say) and ok
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
