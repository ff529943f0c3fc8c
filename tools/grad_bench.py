#!/usr/bin/env python3
"""Times the backward of a block (fz_run_block_grad, the adjoint kernel) against its forward on the MI355X.

Not part of bench.py.  For df1_cascade_params(6) and the Moog ladder at 65 536 x 4096 and 1 048 576 x 1024 (streams x samples): the
forward is Program.run_block on the library's default plan, the backward Program.run_block_grad with every gradient and the default
checkpoint stride.  HIP events around each launch after warm-up; printed per leg: ms (median), the ratio backward / forward, the
adjoint kernel's registers, and its HBM traffic per the formula of DESIGN.md (4 (2 n_in + n_out + n_in) + 8 n_state / C bytes per
stream-sample, plus the coefficient rows) as a fraction of 8 TB/s.

--layout stream-major: the same table for stream-major buffers [n_streams, T, wire] (run_block_stream_major against
run_block_grad_stream_major, the stream-major adjoint kernel).

--layout compare: the stream-major backward against the route a caller with stream-major buffers had before it existed, end to end:
fz_transpose_frames of x and of dL/dy to time-major, fz_run_block_grad, fz_transpose_frames of dL/dx back (every buffer allocated
beforehand).  Same process, legs interleaved: the time-major backward runs for at least 100 ms first (the boards are power-managed),
then every leg is timed --steps times in a forward and again in a backward pass over the list.  Printed per line: the median of
each leg, the yardstick's spread (max - min over its own repeats: the noise), and the ratio to the time-major backward alone.

--loss: one training step under a mean squared error, fused against the route before it, in both layouts.  fused: ONE launch of
run_block_loss_grad (fz_run_block_loss_grad: y, the error and dL/dy formed in the adjoint kernel; every gradient and the per-stream
loss).  route: the forward launch, torch's ((y - target) ** 2).mean() and its derivative 2 (y - target) / n, run_block_grad -- on the
same buffers, same process, legs interleaved as for --layout compare (100 ms of the route first, then --steps launches per leg in a
forward and again in a backward pass over the legs).  The table goes to stdout and to profiles/r10/loss_grad.txt.

--recording: the squared-error backward of a whole RECORDING, run_recording_loss_grad (fz_run_recording_loss_grad: one block-start-states
launch, then the loss kernel per block in reverse), against two alternatives on the same buffers, interleaved in one process as --loss
does.  one: the one-launch run_block_loss_grad over all rows, where its workspace fits the board's free memory.  route: what a caller
had before -- run_block per block into a scratch y (only to get the state before every block), then run_block_loss_grad per block from
the last to the first, chained through state0_grad and the accumulators.  1 048 576 x 4096 and 65 536 x 16 384, both layouts; printed
with each route's workspace bytes.  The table goes to stdout and to profiles/r11/recording.txt.

--rings: the forward / backward table for graphs with delay lines deeper than 8 samples, run_block against run_block_ring_grad
(fz_run_block_ring_grad: the ring adjoint kernel) with every gradient and the default checkpoint stride -- workloads.lds_ring_comb (lines
of 40 and 23 samples) and one deep single comb, ~(0.5 * _1[_256] + _2), at 1 048 576 x 1024 and 65 536 x 4096, time-major.  Same process,
legs interleaved as --loss does (100 ms of the forward first, then --steps launches per leg in a forward and again in a backward pass:
medians of 2 x --steps HIP-event timings per leg).  HBM traffic by the formula of DESIGN.md 9.6 (counted from the code, not measured) as a
fraction of 8 TB/s.  There is no pass mark.  The table goes to stdout and to profiles/r12/ring_grad.txt.

--rings --loss: one training step under a mean squared error for those graphs and shapes, fused against the route a caller had before
it.  fused: ONE launch of run_block_ring_loss_grad (fz_run_block_ring_loss_grad: every gradient and the per-stream loss).  route:
run_block, torch's ((y - target) ** 2).mean() and 2 (y - target) / n, run_block_ring_grad.  Same buffers, same process, legs interleaved
and timed as --loss does; the two legs must agree on the loss.  The pass mark is fused no slower than the route, the margin the route's own
spread in that run.  The table goes to stdout and to profiles/r13/ring_loss_grad.txt.

--rings --recording: the squared-error backward of a whole recording of those graphs, run_recording_ring_loss_grad
(fz_run_recording_ring_loss_grad: one ring states launch, then the ring loss kernel per block in reverse), against two alternatives on the
same buffers, interleaved in one process and timed as --recording does.  one: the one-launch run_block_ring_loss_grad over all rows, where
its workspace fits the board's free memory.  route: what a caller had before -- run_block per block into a scratch y (only to get the
state before every block), then run_block_ring_loss_grad per block from the last to the first, with the same B.  65 536 x 16 384 and
1 048 576 x 4096, time-major; the three legs must agree on the loss bit for bit.  The mark is rec no slower than the route, the margin the
route's own spread in that run; a line that misses it says so.  The table goes to stdout and to profiles/r14/ring_recording.txt.

--rings --layout compare [--loss]: the ring backward on stream-major buffers, run_block_ring_grad_stream_major
(fz_run_block_ring_grad_stream_major; with --loss run_block_ring_loss_grad_stream_major), against the route a caller with stream-major
buffers had before it: fz_transpose_frames of x and of dL/dy (or the target) to time-major, the time-major ring call, fz_transpose_frames
of dL/dx back (every frame buffer allocated beforehand).  Those graphs and shapes; same buffers, same process, legs interleaved (100 ms of
the route first, then --steps launches per leg in a forward and again in a backward pass: medians of 2 x --steps HIP-event timings).  The
two legs must agree bit for bit -- dL/dx, the state gradient, the loss -- before a time is printed.  There is no pass mark: a line slower
than the route says so.  The table goes to stdout and to profiles/r15/ring_stream_major.txt (the --loss table is appended to it).

--rings --recording --layout stream-major|compare [--loss]: the backward of a whole recording of those graphs on stream-major buffers,
run_recording_ring_grad_stream_major (fz_run_recording_ring_grad_stream_major; with --loss run_recording_ring_loss_grad_stream_major).
stream-major: that call alone.  compare: against the route a caller with [batch, time] buffers had before it -- fz_transpose_frames of x
and of dL/dy (or the target) to time-major, the time-major ring recording, fz_transpose_frames of dL/dx back (every frame buffer and both
workspaces allocated beforehand).  65 536 x 16 384 and 1 048 576 x 4096; same buffers, same process, legs interleaved (100 ms of the route
first, then --steps calls per leg in a forward and again in a backward pass: medians of 2 x --steps HIP-event timings, ten at the default).
The two legs must agree bit for bit -- dL/dx, the state gradient, the loss -- before a time is printed.  There is no pass mark: a line slower
than the route beyond the route's own spread says so.  The table goes to stdout and to profiles/r16/ring_sm_recording.txt (the --loss table
is appended to it).

--far: the forward / backward table for graphs with delay lines deeper than 256 samples, run_block against run_block_far_grad
(fz_run_block_far_grad: the far adjoint kernel, rings in HBM) with every gradient and the default checkpoint stride -- workloads.far_comb
(300 samples), a 2000-sample comb and far_tap1 (~(0.4*_1[_300] + 0.3*_1[_1] + 0.2*_1[_20] + _2): the per-row path) -- and next to them, in
the same run, the LDS ring kernel on ~(0.5 * _1[_256] + _2), the nearest yardstick.  1 048 576 x 1024 and 65 536 x 4096, time-major; the
method of --rings (one process, legs interleaved, medians of 2 x --steps HIP-event timings per leg).  Before a time is printed the backward
at the default stride agrees bit for bit with the one at C = 1 (another chunking, and for far_tap1 the other path).  HBM traffic by the
formula of DESIGN.md 9.11 (counted from the code, not measured) as a fraction of 8 TB/s.  There is no pass mark.  The table goes to stdout
and to profiles/r17/far_grad.txt.

--far --layout compare [--loss]: the far backward on stream-major buffers, run_block_far_grad_stream_major
(fz_run_block_far_grad_stream_major; with --loss run_block_far_loss_grad_stream_major), against the route a caller with stream-major
buffers had before it existed, with the legs, the method and the mark of --rings --layout compare: workloads.far_comb, the 2000-sample
comb and far_tap1.  The table goes to stdout and to profiles/r19/far_stream_major.txt.

--far --recording: the squared-error backward of a whole recording of graphs with delay lines deeper than 256 samples,
run_recording_far_loss_grad (fz_run_recording_far_loss_grad: one far states launch, then the far loss kernel per block in reverse), with
the legs, the shapes, the method and the mark of --rings --recording: one = the one-launch run_block_far_loss_grad where its workspace
fits; route = run_block per block for the states, copying the state rows before each block, then run_block_far_loss_grad per block in
reverse at the same B.  workloads.far_comb (300 samples) and ~(0.5*_1[_2000] + _2).  The table, the workspaces and B go to stdout and to
profiles/r18/far_recording.txt.

--far --recording --layout stream-major|compare [--loss]: the backward of a whole recording of such graphs on stream-major buffers,
run_recording_far_grad(stream_major=True) (fz_run_recording_far_grad_for with FZ_GRAD_STREAM_MAJOR; with --loss
run_recording_far_loss_grad), with the legs, the shapes, the method and the mark of --rings --recording --layout compare: route =
fz_transpose_frames of x and of dL/dy (or the target), the time-major far recording at the same B, fz_transpose_frames of dL/dx back.
workloads.far_comb, the 2000-sample comb and far_tap1.  The table goes to stdout and to profiles/r20/far_sm_recording.txt (the --loss
table is appended to it).

usage: tools/grad_bench.py [--warmup W] [--steps K] [--legs small|large|all] [--layout time-major|stream-major|compare] [--loss] [--recording] [--rings] [--far]
       (--far takes --recording, or --layout compare, alone or with --loss; --far --recording takes --layout stream-major|compare, alone or with --loss)
       (--rings takes --layout compare, alone or with --loss; --rings --recording takes --layout stream-major|compare, alone or with --loss)
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


def compare(a, torch):
    """the stream-major backward against transpose + time-major backward + transpose, interleaved in one process"""
    import time
    print(f"# stream-major backward vs the transposing route, HIP events, {a.steps} launches per leg and pass, a forward and a backward pass over the legs")
    print(f"{'graph':20s} {'streams x T':>16s} {'route ms':>9s} {'spread':>7s} {'sm ms':>9s} {'tm ms':>9s} {'sm/route':>9s} {'sm/tm':>6s} {'vgprs':>6s} {'lds':>6s}  stream-major adjoint kernel")
    shapes = SHAPES["small"] + SHAPES["large"] if a.legs == "all" else SHAPES[a.legs]
    for ns, T in shapes:
        x_sm = torch.empty((ns, T, 1), dtype=torch.float32, device="cuda")
        F.synth_fill(x_sm, seed=W.SEED)
        gy_sm = torch.empty_like(x_sm)
        F.synth_fill(gy_sm, seed=W.SEED + 1)
        gx_sm, gx_back = torch.empty_like(x_sm), torch.empty_like(x_sm)
        x_tm, gy_tm = (torch.empty((T, ns, 1), dtype=torch.float32, device="cuda") for _ in range(2))
        for name, fn in GRAPHS.items():
            prog = F.compile(F.from_sexpr(fn()))
            pp = params_for(name, prog, ns, torch)
            s0 = torch.zeros((prog.n_state, ns), dtype=torch.float32, device="cuda")

            def route():
                F.frames_from_stream_major(x_sm, 0, out=x_tm)
                F.frames_from_stream_major(gy_sm, 0, out=gy_tm)
                r = prog.run_block_grad(x_tm, gy_tm, s0, pp, state_grad=s0)
                F.frames_to_stream_major(r["x"], out=gx_back)

            def sm():
                prog.run_block_grad_stream_major(x_sm, gy_sm, s0, pp, state_grad=s0, in_grad=gx_sm)

            def tm():
                prog.run_block_grad(x_tm, gy_tm, s0, pp, state_grad=s0)
            legs = {"route": route, "sm": sm, "tm": tm}
            for f in legs.values():                            # JIT, allocator
                f()
            torch.cuda.synchronize()
            t_end = time.time() + 0.1
            while time.time() < t_end:                          # at least 100 ms of the default before the first timing
                tm()
                torch.cuda.synchronize()
            got = {k: [] for k in legs}
            for order in (list(legs), list(legs)[::-1]):
                for k in order:
                    got[k] += samples(legs[k], a.steps, torch)
            med = {k: float(np.median(v)) for k, v in got.items()}
            res = prog.grad_resources(stream_major=True)
            print(f"{name:20s} {f'{ns} x {T}':>16s} {med['route']:9.3f} {max(got['route']) - min(got['route']):7.3f} {med['sm']:9.3f} {med['tm']:9.3f} "
                  f"{med['sm'] / med['route']:9.3f} {med['sm'] / med['tm']:6.3f} {res['vgprs'] + res['agprs']:6d} {res['lds_bytes']:6d}  "
                  f"{prog.grad_kernel_symbol(stream_major=True)}", flush=True)
            print("#   all timings ms: " + "; ".join(f"{k} " + " ".join(f"{t:.3f}" for t in v) for k, v in got.items()), flush=True)
            del pp, s0
        del x_sm, gy_sm, gx_sm, gx_back, x_tm, gy_tm
        torch.cuda.empty_cache()


def loss_bench(a, torch):
    """one step under a mean squared error: the fused launch against forward + torch MSE and derivative + backward, both layouts"""
    import time
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)
    props = torch.cuda.get_device_properties(0)
    say(f"# command: tools/grad_bench.py --loss --steps {a.steps} --legs {a.legs}")
    say(f"# date {datetime.date.today().isoformat()}, board {props.name or 'unnamed'} ({getattr(props, 'gcnArchName', '?')})")
    say(f"# fused = one run_block_loss_grad launch; route = run_block + torch ((y - target)**2).mean() and 2 (y - target) / n + run_block_grad;")
    say(f"# HIP events, {a.steps} launches per leg and pass, a forward and a backward pass over the legs; spread = max - min of the route's own repeats")
    say(f"{'graph':20s} {'layout':>12s} {'streams x T':>16s} {'route ms':>9s} {'spread':>7s} {'fused ms':>9s} {'fused/route':>11s} {'vgprs':>6s} {'lds':>6s}  loss kernel")
    shapes = SHAPES["small"] + SHAPES["large"] if a.legs == "all" else SHAPES[a.legs]
    for ns, T in shapes:
        for sm in (False, True):
            x = torch.empty((ns, T, 1) if sm else (T, ns, 1), dtype=torch.float32, device="cuda")
            F.synth_fill(x, seed=W.SEED)
            target = torch.empty_like(x)
            F.synth_fill(target, seed=W.SEED + 1)
            y, gy, gx = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
            n = float(ns) * T
            for name, fn in GRAPHS.items():
                prog = F.compile(F.from_sexpr(fn()))
                pp = params_for(name, prog, ns, torch)
                s0 = torch.zeros((prog.n_state, ns), dtype=torch.float32, device="cuda")
                st = s0.clone()
                fwd = prog.run_block_stream_major if sm else prog.run_block
                bwd = prog.run_block_grad_stream_major if sm else prog.run_block_grad
                kw = {"in_grad": gx} if sm else {}

                def route():
                    st.copy_(s0)
                    fwd(x, state=st, params=pp, out=y)
                    loss = ((y - target) ** 2).mean()
                    torch.mul(y - target, 2.0 / n, out=gy)
                    bwd(x, gy, s0, pp, **kw)
                    return loss

                def fused():
                    f = prog.run_block_loss_grad_stream_major if sm else prog.run_block_loss_grad
                    r = f(x, target, s0, pp, grad_scale=2.0 / n, want=("x", "state", "params", "consts", "loss"), **kw)
                    return r["loss"].double().sum() / n
                legs = {"route": route, "fused": fused}
                vals = {k: float(f()) for k, f in legs.items()}        # JIT, allocator; and the two routes agree on the loss
                assert abs(vals["route"] - vals["fused"]) <= 1e-3 * abs(vals["route"]), vals    # (a sanity check, not the test: float32 sums in two orders)
                torch.cuda.synchronize()
                t_end = time.time() + 0.1
                while time.time() < t_end:                          # at least 100 ms of the yardstick before the first timing
                    route()
                    torch.cuda.synchronize()
                got = {k: [] for k in legs}
                for order in (list(legs), list(legs)[::-1]):
                    for k in order:
                        got[k] += samples(legs[k], a.steps, torch)
                med = {k: float(np.median(v)) for k, v in got.items()}
                res = prog.loss_grad_resources(stream_major=sm)
                say(f"{name:20s} {'stream-major' if sm else 'time-major':>12s} {f'{ns} x {T}':>16s} {med['route']:9.3f} {max(got['route']) - min(got['route']):7.3f} "
                    f"{med['fused']:9.3f} {med['fused'] / med['route']:11.3f} {res['vgprs'] + res['agprs']:6d} {res['lds_bytes']:6d}  "
                    f"{prog.loss_grad_kernel_symbol(stream_major=sm)}")
                say("#   all timings ms: " + "; ".join(f"{k} " + " ".join(f"{t:.3f}" for t in v) for k, v in got.items()))
                del pp, s0, st
            del x, target, y, gy, gx
            torch.cuda.empty_cache()
    out = os.path.join(ROOT, "profiles", "r10", "loss_grad.txt")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


REC_SHAPES = {"large": [(1 << 20, 4096)], "small": [(65536, 16384)]}


def recording_bench(a, torch):
    """the backward of a whole recording under a mean squared error: the recording call, the one-launch call, and blocks chained by hand"""
    import time
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)
    props = torch.cuda.get_device_properties(0)
    say(f"# command: tools/grad_bench.py --recording --steps {a.steps} --legs {a.legs}")
    say(f"# date {datetime.date.today().isoformat()}, board {props.name or 'unnamed'} ({getattr(props, 'gcnArchName', '?')})")
    say("# rec = one run_recording_loss_grad call; one = one run_block_loss_grad launch over all rows (where its workspace fits);")
    say("# route = run_block per block into a scratch y for the states, then run_block_loss_grad per block in reverse (same B as rec)")
    say(f"# HIP events, {a.steps} calls per leg and pass, a forward and a backward pass over the legs; spread = max - min of a leg's own repeats")
    say(f"{'graph':20s} {'layout':>12s} {'streams x T':>16s} {'B':>5s} {'route ms':>9s} {'spread':>7s} {'rec ms':>9s} {'spread':>7s} {'one ms':>9s} {'spread':>7s} "
        f"{'rec/route':>9s} {'rec/one':>8s} {'ws rec MB':>10s} {'ws route MB':>11s} {'ws one MB':>10s}  states kernel")
    shapes = REC_SHAPES["small"] + REC_SHAPES["large"] if a.legs == "all" else REC_SHAPES[a.legs]
    want = ("x", "state", "params", "consts", "loss")
    for ns, T in shapes:
        for sm in (False, True):
            x = torch.empty((ns, T, 1) if sm else (T, ns, 1), dtype=torch.float32, device="cuda")
            F.synth_fill(x, seed=W.SEED)
            target = torch.empty_like(x)
            F.synth_fill(target, seed=W.SEED + 1)
            gx = torch.empty_like(x)
            n = float(ns) * T
            for name, fn in GRAPHS.items():
                prog = F.compile(F.from_sexpr(fn()))
                pp = params_for(name, prog, ns, torch)
                s0 = torch.zeros((prog.n_state, ns), dtype=torch.float32, device="cuda")
                B = prog.recording_block_rows(T)
                nb = (T + B - 1) // B
                ws_rec, ws_one = prog.recording_workspace_bytes(ns, T, stream_major=sm), prog.grad_workspace_bytes(ns, T)
                # the route keeps the state before every block itself, a scratch y of one block, and one block's checkpoints
                ws_route = nb * prog.n_state * ns * 4 + B * ns * prog.n_out * 4 + prog.grad_workspace_bytes(ns, B)
                ws = torch.empty(ws_rec // 4, dtype=torch.float32, device="cuda")
                states = torch.empty((nb + 1, prog.n_state, ns), dtype=torch.float32, device="cuda")
                y = torch.empty_like(x) if sm else torch.empty((B, ns, 1), dtype=torch.float32, device="cuda")
                if sm:
                    ws_route += (T - B) * ns * prog.n_out * 4     # (a stream-major window writes into a buffer of all rows)

                def rec():
                    r = prog.run_recording_loss_grad(x, target, s0, pp, grad_scale=2.0 / n, want=want, stream_major=sm, in_grad=gx if sm else None, workspace=ws)
                    return r["loss"].double().sum() / n

                def route():
                    states[0].copy_(s0)
                    for k in range(nb):
                        rows = min(B, T - k * B)
                        states[k + 1].copy_(states[k])
                        if sm:
                            prog.run_block_stream_major(x, state=states[k + 1], params=pp, out=y, row0=k * B, n_samples=rows)
                        else:
                            prog.run_block(x[k * B:k * B + rows], state=states[k + 1], params=pp, out=y[:rows])
                    acc, sg = {}, None
                    for k in range(nb - 1, -1, -1):
                        rows = min(B, T - k * B)
                        if sm:
                            r = prog.run_block_loss_grad_stream_major(x, target, states[k], pp, state_grad=sg, grad_scale=2.0 / n, want=want, accum=acc,
                                                                      row0=k * B, n_samples=rows, in_grad=gx)
                        else:
                            r = prog.run_block_loss_grad(x[k * B:k * B + rows], target[k * B:k * B + rows], states[k], pp, state_grad=sg, grad_scale=2.0 / n,
                                                         want=want, accum=acc)
                        # (the accumulators the next launch adds to: only those the graph has rows of)
                        acc, sg = {k: r[k] for k, rows_k in (("params", prog.n_param), ("consts", prog.n_const), ("loss", 1)) if rows_k}, r["state"]
                    return acc["loss"].double().sum() / n

                def one():
                    f = prog.run_block_loss_grad_stream_major if sm else prog.run_block_loss_grad
                    r = f(x, target, s0, pp, grad_scale=2.0 / n, want=want, **({"in_grad": gx} if sm else {}))
                    return r["loss"].double().sum() / n
                legs = {"route": route, "rec": rec}
                if ws_one + (4 << 30) < torch.cuda.mem_get_info()[0]:
                    legs["one"] = one
                vals = {k: float(f()) for k, f in legs.items()}        # JIT, allocator; and the legs agree on the loss
                assert all(v == vals["rec"] for v in vals.values()), vals     # (bit for bit: the same per-stream sums)
                torch.cuda.synchronize()
                t_end = time.time() + 0.1
                while time.time() < t_end:                          # at least 100 ms of the yardstick before the first timing
                    route()
                    torch.cuda.synchronize()
                got = {k: [] for k in legs}
                for order in (list(legs), list(legs)[::-1]):
                    for k in order:
                        got[k] += samples(legs[k], a.steps, torch)
                med = {k: float(np.median(v)) for k, v in got.items()}
                sp = {k: max(v) - min(v) for k, v in got.items()}
                one_s = f"{med['one']:9.3f} {sp['one']:7.3f}" if "one" in med else f"{'-':>9s} {'-':>7s}"
                ratio_one = f"{med['rec'] / med['one']:8.3f}" if "one" in med else f"{'-':>8s}"
                say(f"{name:20s} {'stream-major' if sm else 'time-major':>12s} {f'{ns} x {T}':>16s} {B:5d} {med['route']:9.3f} {sp['route']:7.3f} "
                    f"{med['rec']:9.3f} {sp['rec']:7.3f} {one_s} {med['rec'] / med['route']:9.3f} {ratio_one} {ws_rec / 2**20:10.1f} {ws_route / 2**20:11.1f} "
                    f"{ws_one / 2**20:10.1f}  {prog.states_kernel_symbol(sm)}")
                say("#   all timings ms: " + "; ".join(f"{k} " + " ".join(f"{t:.3f}" for t in v) for k, v in got.items()))
                del pp, s0, ws, states, y
                torch.cuda.empty_cache()
            del x, target, gx
            torch.cuda.empty_cache()
    out = os.path.join(ROOT, "profiles", "r11", "recording.txt")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


RING_GRAPHS = {"lds_ring_comb": W.lds_ring_comb, "comb256": lambda: W.fb(W.add(W.mul(W.lit(0.5), W.DEL(1, 256)), W.IN(2)))}


def rings_bench(a, torch):
    """forward against the ring backward of graphs with delay lines in LDS, interleaved in one process"""
    import time
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)
    props = torch.cuda.get_device_properties(0)
    say(f"# command: tools/grad_bench.py --rings --steps {a.steps} --legs {a.legs}")
    say(f"# date {datetime.date.today().isoformat()}, board {props.name or 'unnamed'} ({getattr(props, 'gcnArchName', '?')})")
    say(f"# fwd = run_block (library default plan); bwd = run_block_ring_grad, every gradient, default checkpoint stride; time-major frames;")
    say(f"# HIP events, {a.steps} launches per leg and pass, a forward and a backward pass over the legs; spread = max - min of the forward's own repeats;")
    say("# bytes: fwd 4 (n_in + n_out), bwd 4 (3 n_in + n_out) + 8 n_register_state / C + 4 n_ring_lines + 4 n_ring_reads per stream-sample -- counted from the code")
    say(f"{'graph':16s} {'streams x T':>16s} {'fwd ms':>9s} {'spread':>7s} {'bwd ms':>9s} {'bwd/fwd':>8s} {'fwd /8TB/s':>10s} {'bwd /8TB/s':>10s} {'C':>3s} {'vgprs':>6s} {'lds':>6s}  ring adjoint kernel")
    shapes = SHAPES["large"] + SHAPES["small"] if a.legs == "all" else SHAPES[a.legs]
    for ns, T in shapes:
        x = torch.empty((T, ns, 1), dtype=torch.float32, device="cuda")
        F.synth_fill(x, seed=W.SEED)
        gy = torch.empty_like(x)
        F.synth_fill(gy, seed=W.SEED + 1)
        y = torch.empty_like(x)
        for name, fn in RING_GRAPHS.items():
            prog = F.compile(F.from_sexpr(fn()))
            s0 = torch.zeros((prog.n_state, ns), dtype=torch.float32, device="cuda")
            st = s0.clone()

            def fwd():
                st.copy_(s0)
                prog.run_block(x, state=st, out=y)

            def bwd():
                prog.run_block_ring_grad(x, gy, s0, None, state_grad=s0)
            legs = {"fwd": fwd, "bwd": bwd}
            for f in legs.values():                            # JIT, allocator
                f()
            torch.cuda.synchronize()
            t_end = time.time() + 0.1
            while time.time() < t_end:                          # at least 100 ms of the yardstick before the first timing
                fwd()
                torch.cuda.synchronize()
            got = {k: [] for k in legs}
            for order in (list(legs), list(legs)[::-1]):
                for k in order:
                    got[k] += samples(legs[k], a.steps, torch)
            med = {k: float(np.median(v)) for k, v in got.items()}
            res = prog.ring_grad_resources()
            C = res["unroll"]
            depths = [d for _, d in prog.lines()]
            n_reg, n_rl = sum(d for d in depths if d <= 8), sum(1 for d in depths if d > 8)
            n_rr = len({(k, a_, b_) for k, a_, b_, _ in prog.ir() if k == "delay" and dict(prog.lines()).get(a_, 0) > 8})
            fbytes = 4.0 * ns * T * (prog.n_in + prog.n_out)
            bbytes = ns * T * (4.0 * (3 * prog.n_in + prog.n_out) + 8.0 * n_reg / C + 4.0 * n_rl + 4.0 * n_rr)
            say(f"{name:16s} {f'{ns} x {T}':>16s} {med['fwd']:9.3f} {max(got['fwd']) - min(got['fwd']):7.3f} {med['bwd']:9.3f} {med['bwd'] / med['fwd']:8.2f} "
                f"{fbytes / (med['fwd'] / 1e3) / HBM:10.3f} {bbytes / (med['bwd'] / 1e3) / HBM:10.3f} {C:3d} {res['vgprs'] + res['agprs']:6d} {res['lds_bytes']:6d}  "
                f"{prog.ring_grad_kernel_symbol()}")
            say("#   all timings ms: " + "; ".join(f"{k} " + " ".join(f"{t:.3f}" for t in v) for k, v in got.items()))
            del s0, st
        del x, gy, y
        torch.cuda.empty_cache()
    out = os.path.join(ROOT, "profiles", "r12", "ring_grad.txt")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


def _comb(depth):
    return lambda: W.fb(W.add(W.mul(W.lit(0.5), W.DEL(1, depth)), W.IN(2)))


FAR_GRAPHS = {"far_comb": W.far_comb, "comb2000": _comb(2000),
              "far_tap1": lambda: W.fb(W.add(W.add(W.add(W.mul(W.lit(0.4), W.DEL(1, 300)), W.mul(W.lit(0.3), W.DEL(1, 1))), W.mul(W.lit(0.2), W.DEL(1, 20))), W.IN(2))),
              "comb256": _comb(256)}


def far_bench(a, torch):
    """forward against the far backward of graphs with delay lines in HBM, and the LDS ring kernel on a 256-sample comb next to them,
    interleaved in one process"""
    import time
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)
    props = torch.cuda.get_device_properties(0)
    say(f"# command: tools/grad_bench.py --far --steps {a.steps} --legs {a.legs}")
    say(f"# date {datetime.date.today().isoformat()}, board {props.name or 'unnamed'} ({getattr(props, 'gcnArchName', '?')})")
    say("# fwd = run_block (library default plan); bwd = run_block_far_grad, every gradient, default checkpoint stride; time-major frames;")
    say(f"# HIP events, {a.steps} launches per leg and pass, a forward and a backward pass over the legs; spread = max - min of the forward's own repeats;")
    say("# the backward at the default stride agrees bit for bit with the one at C = 1 (dL/dx, the state gradient) before a time is printed;")
    say("# bytes per stream-sample: fwd 4 (n_in + n_out + n_far_lines + n_far_reads); bwd 4 (3 n_in + n_out) + 8 n_register_state / C")
    say("#   + 4 (n_ring_lines + n_far_lines) + 4 n_ring_reads + 8 n_far_reads (values) + 4 n_far_lines + 8 n_far_reads - 4 n_full_depth_reads (adjoint ring;")
    say("#   the per-row path stores rule 2's reset as well: + 4 n_far_lines),")
    say("#   + 16 (sum of the far depths) / T once per block -- counted from the code")
    say(f"{'graph':16s} {'streams x T':>16s} {'fwd ms':>9s} {'spread':>7s} {'bwd ms':>9s} {'bwd/fwd':>8s} {'fwd /8TB/s':>10s} {'bwd /8TB/s':>10s} {'C':>3s} {'path':>7s} {'vgprs':>6s} {'sgpr spills':>11s} {'lds':>6s}  adjoint kernel")
    shapes = SHAPES["large"] + SHAPES["small"] if a.legs == "all" else SHAPES[a.legs]
    for ns, T in shapes:
        x = torch.empty((T, ns, 1), dtype=torch.float32, device="cuda")
        F.synth_fill(x, seed=W.SEED)
        gy = torch.empty_like(x)
        F.synth_fill(gy, seed=W.SEED + 1)
        y = torch.empty_like(x)
        for name, fn in FAR_GRAPHS.items():
            prog = F.compile(F.from_sexpr(fn()))
            s0 = torch.zeros((prog.n_state, ns), dtype=torch.float32, device="cuda")
            st = s0.clone()

            def fwd():
                st.copy_(s0)
                prog.run_block(x, state=st, out=y)

            def bwd(c=0):
                return prog.run_block_far_grad(x, gy, s0, None, state_grad=s0, checkpoint_rows=c)
            fwd()                                              # JIT, allocator; and the two strides agree bit for bit
            r0 = bwd()
            r1 = bwd(1)
            torch.cuda.synchronize()
            for key in ("x", "state"):
                assert torch.equal(r0[key].view(torch.int32), r1[key].view(torch.int32)), f"{name} {ns} x {T}: {key} at the default stride and at C = 1 differs"
            del r0, r1
            torch.cuda.empty_cache()
            legs = {"fwd": fwd, "bwd": bwd}
            t_end = time.time() + 0.1
            while time.time() < t_end:                          # at least 100 ms of the yardstick before the first timing
                fwd()
                torch.cuda.synchronize()
            got = {k: [] for k in legs}
            for order in (list(legs), list(legs)[::-1]):
                for k in order:
                    got[k] += samples(legs[k], a.steps, torch)
            med = {k: float(np.median(v)) for k, v in got.items()}
            res, src = prog.far_grad_resources(), prog.far_grad_source()
            C = res["unroll"]
            depth = dict(prog.lines())
            depths = list(depth.values())
            n_reg, n_rl, n_fl = sum(d for d in depths if d <= 8), sum(1 for d in depths if 8 < d <= 256), sum(1 for d in depths if d > 256)
            reads = {(a_, b_) for k, a_, b_, _ in prog.ir() if k == "delay"}
            n_rr = sum(1 for a_, _ in reads if 8 < depth[a_] <= 256)
            n_fr, n_full = sum(1 for a_, _ in reads if depth[a_] > 256), sum(1 for a_, b_ in reads if depth[a_] > 256 and b_ == depth[a_])
            far_slots = sum(d for d in depths if d > 256)
            fbytes = 4.0 * ns * T * (prog.n_in + prog.n_out + n_fl + n_fr)
            path = "-" if not n_fl else "fast" if "#define FZ_FAR_FAST 1 " in src.split("// ==== fz_graph_body.h ====")[0] else "per-row"
            bbytes = ns * T * (4.0 * (3 * prog.n_in + prog.n_out) + 8.0 * n_reg / C + 4.0 * (n_rl + n_fl) + 4.0 * n_rr + 8.0 * n_fr
                               + 4.0 * n_fl * (2 if path == "per-row" else 1) + 8.0 * n_fr - 4.0 * n_full) + 16.0 * far_slots * ns
            say(f"{name:16s} {f'{ns} x {T}':>16s} {med['fwd']:9.3f} {max(got['fwd']) - min(got['fwd']):7.3f} {med['bwd']:9.3f} {med['bwd'] / med['fwd']:8.2f} "
                f"{fbytes / (med['fwd'] / 1e3) / HBM:10.3f} {bbytes / (med['bwd'] / 1e3) / HBM:10.3f} {C:3d} {path:>7s} {res['vgprs'] + res['agprs']:6d} {res['sgpr_spills']:11d} "
                f"{res['lds_bytes']:6d}  {prog.far_grad_kernel_symbol()}")
            say("#   all timings ms: " + "; ".join(f"{k} " + " ".join(f"{t:.3f}" for t in v) for k, v in got.items()))
            del s0, st
            torch.cuda.empty_cache()
        del x, gy, y
        torch.cuda.empty_cache()
    out = os.path.join(ROOT, "profiles", "r17", "far_grad.txt")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


def rings_compare_bench(a, torch, far=False):
    """the ring backward on stream-major buffers (plain, or with a.loss under the squared-error loss) against transpose + the time-major
    ring call + transpose, interleaved in one process; the two legs agree bit for bit before a time is printed.  far: the same for
    graphs with delay lines in HBM, through the far family's calls"""
    import time
    lines = []
    fam = "far" if far else "ring"

    def say(line):
        print(line, flush=True)
        lines.append(line)
    props = torch.cuda.get_device_properties(0)
    loss = bool(a.loss)
    call = f"run_block_{fam}_loss_grad" if loss else f"run_block_{fam}_grad"
    say(f"# command: tools/grad_bench.py {'--far' if far else '--rings'} --layout compare{' --loss' if loss else ''} --steps {a.steps} --legs {a.legs}")
    say(f"# date {datetime.date.today().isoformat()}, board {props.name or 'unnamed'} ({getattr(props, 'gcnArchName', '?')})")
    say(f"# sm = one {call}_stream_major launch on [n_streams, T] buffers; route = fz_transpose_frames of x and of {'the target' if loss else 'dL/dy'}, {call}, fz_transpose_frames of dL/dx back;")
    say(f"# every gradient, default checkpoint stride; HIP events, {a.steps} launches per leg and pass, a forward and a")
    say("# backward pass over the legs; spread = max - min of the route's own repeats; the legs agree bit for bit (dL/dx, the state gradient" + (", the loss" if loss else "") + ") before a time is printed")
    say(f"{'graph':16s} {'streams x T':>16s} {'route ms':>9s} {'spread':>7s} {'sm ms':>9s} {'sm/route':>9s} {'slower':>6s} {'C':>3s} {'R':>3s} {'lanes':>5s} {'vgprs':>6s} {'sgpr spills':>11s} {'lds':>6s}  stream-major {fam} kernel")
    shapes = SHAPES["large"] + SHAPES["small"] if a.legs == "all" else SHAPES[a.legs]
    graphs = {k: v for k, v in FAR_GRAPHS.items() if k != "comb256"} if far else RING_GRAPHS
    for ns, T in shapes:
        x_sm = torch.empty((ns, T, 1), dtype=torch.float32, device="cuda")
        F.synth_fill(x_sm, seed=W.SEED)
        yt_sm = torch.empty_like(x_sm)                         # dL/dy, or the target
        F.synth_fill(yt_sm, seed=W.SEED + 1)
        gx_sm, gx_back = torch.empty_like(x_sm), torch.empty_like(x_sm)
        x_tm, yt_tm = (torch.empty((T, ns, 1), dtype=torch.float32, device="cuda") for _ in range(2))
        n = float(ns) * T
        want = ("x", "state", "params", "consts") + (("loss",) if loss else ())
        for name, fn in graphs.items():
            prog = F.compile(F.from_sexpr(fn()))
            s0 = torch.zeros((prog.n_state, ns), dtype=torch.float32, device="cuda")
            tm_call, sm_call = getattr(prog, call), getattr(prog, call + "_stream_major")

            def route():
                F.frames_from_stream_major(x_sm, 0, out=x_tm)
                F.frames_from_stream_major(yt_sm, 0, out=yt_tm)
                if loss:
                    r = tm_call(x_tm, yt_tm, s0, None, state_grad=s0, grad_scale=2.0 / n, want=want)
                else:
                    r = tm_call(x_tm, yt_tm, s0, None, state_grad=s0)
                F.frames_to_stream_major(r["x"], out=gx_back)
                return r

            def sm():
                if loss:
                    return sm_call(x_sm, yt_sm, s0, None, state_grad=s0, grad_scale=2.0 / n, want=want, in_grad=gx_sm)
                return sm_call(x_sm, yt_sm, s0, None, state_grad=s0, in_grad=gx_sm)
            legs = {"route": route, "sm": sm}
            first = {k: f() for k, f in legs.items()}           # JIT, allocator; and the legs agree bit for bit
            torch.cuda.synchronize()
            same = lambda u, v: torch.equal(u.view(torch.int32), v.view(torch.int32))   # noqa: E731
            assert same(gx_sm, gx_back), f"{name} {ns} x {T}: dL/dx of the two legs differs"
            for key in ("state",) + (("loss",) if loss else ()):
                assert same(first["sm"][key], first["route"][key]), f"{name} {ns} x {T}: {key} of the two legs differs"
            del first
            t_end = time.time() + 0.1
            while time.time() < t_end:                          # at least 100 ms of the yardstick before the first timing
                route()
                torch.cuda.synchronize()
            got = {k: [] for k in legs}
            for order in (list(legs), list(legs)[::-1]):
                for k in order:
                    got[k] += samples(legs[k], a.steps, torch)
            med = {k: float(np.median(v)) for k, v in got.items()}
            spread = max(got["route"]) - min(got["route"])
            res = getattr(prog, f"{fam}_loss_grad_resources" if loss else f"{fam}_grad_resources")(0, stream_major=True)
            sym = getattr(prog, f"{fam}_loss_grad_kernel_symbol" if loss else f"{fam}_grad_kernel_symbol")(0, stream_major=True)
            R, lanes = int(sym.split("_g")[0].split("r")[-1].split("b")[0]), int(sym.split("_g")[0].split("b")[-1])
            say(f"{name:16s} {f'{ns} x {T}':>16s} {med['route']:9.3f} {spread:7.3f} {med['sm']:9.3f} {med['sm'] / med['route']:9.3f} "
                f"{'YES' if med['sm'] > med['route'] + spread else 'no':>6s} {res['unroll']:3d} {R:3d} {lanes:5d} {res['vgprs'] + res['agprs']:6d} "
                f"{res['sgpr_spills']:11d} {res['lds_bytes']:6d}  {sym}")
            say("#   all timings ms: " + "; ".join(f"{k} " + " ".join(f"{t:.3f}" for t in v) for k, v in got.items()))
            del s0
            torch.cuda.empty_cache()
        del x_sm, yt_sm, gx_sm, gx_back, x_tm, yt_tm
        torch.cuda.empty_cache()
    out = os.path.join(ROOT, "profiles", "r19", "far_stream_major.txt") if far else os.path.join(ROOT, "profiles", "r15", "ring_stream_major.txt")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "a" if loss and os.path.exists(out) else "w") as f:
        f.write("\n".join(lines) + "\n")


def rings_loss_bench(a, torch):
    """one step under a mean squared error for graphs with delay lines in LDS: the fused launch against forward + torch MSE and
    derivative + ring backward, interleaved in one process"""
    import time
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)
    props = torch.cuda.get_device_properties(0)
    say(f"# command: tools/grad_bench.py --rings --loss --steps {a.steps} --legs {a.legs}")
    say(f"# date {datetime.date.today().isoformat()}, board {props.name or 'unnamed'} ({getattr(props, 'gcnArchName', '?')})")
    say("# fused = one run_block_ring_loss_grad launch; route = run_block + torch ((y - target)**2).mean() and 2 (y - target) / n + run_block_ring_grad;")
    say(f"# time-major frames; HIP events, {a.steps} launches per leg and pass, a forward and a backward pass over the legs; spread = max - min of the route's own repeats;")
    say("# pass = fused median <= route median + spread")
    say(f"{'graph':16s} {'streams x T':>16s} {'route ms':>9s} {'spread':>7s} {'fused ms':>9s} {'fused/route':>11s} {'pass':>5s} {'C':>3s} {'vgprs':>6s} {'sgpr spills':>11s} {'lds':>6s}  ring loss kernel")
    shapes = SHAPES["large"] + SHAPES["small"] if a.legs == "all" else SHAPES[a.legs]
    for ns, T in shapes:
        x = torch.empty((T, ns, 1), dtype=torch.float32, device="cuda")
        F.synth_fill(x, seed=W.SEED)
        target = torch.empty_like(x)
        F.synth_fill(target, seed=W.SEED + 1)
        y, gy = torch.empty_like(x), torch.empty_like(x)
        n = float(ns) * T
        for name, fn in RING_GRAPHS.items():
            prog = F.compile(F.from_sexpr(fn()))
            s0 = torch.zeros((prog.n_state, ns), dtype=torch.float32, device="cuda")
            st = s0.clone()

            def route():
                st.copy_(s0)
                prog.run_block(x, state=st, out=y)
                loss = ((y - target) ** 2).mean()
                torch.mul(y - target, 2.0 / n, out=gy)
                prog.run_block_ring_grad(x, gy, s0, None)
                return loss

            def fused():
                r = prog.run_block_ring_loss_grad(x, target, s0, None, grad_scale=2.0 / n, want=("x", "state", "params", "consts", "loss"))
                return r["loss"].double().sum() / n
            legs = {"route": route, "fused": fused}
            vals = {k: float(f()) for k, f in legs.items()}        # JIT, allocator; and the two legs agree on the loss
            assert abs(vals["route"] - vals["fused"]) <= 1e-3 * abs(vals["route"]), vals    # (a sanity check, not the test: float32 sums in two orders)
            torch.cuda.synchronize()
            t_end = time.time() + 0.1
            while time.time() < t_end:                          # at least 100 ms of the yardstick before the first timing
                route()
                torch.cuda.synchronize()
            got = {k: [] for k in legs}
            for order in (list(legs), list(legs)[::-1]):
                for k in order:
                    got[k] += samples(legs[k], a.steps, torch)
            med = {k: float(np.median(v)) for k, v in got.items()}
            spread = max(got["route"]) - min(got["route"])
            res = prog.ring_loss_grad_resources()
            say(f"{name:16s} {f'{ns} x {T}':>16s} {med['route']:9.3f} {spread:7.3f} {med['fused']:9.3f} {med['fused'] / med['route']:11.3f} "
                f"{'yes' if med['fused'] <= med['route'] + spread else 'NO':>5s} {res['unroll']:3d} {res['vgprs'] + res['agprs']:6d} {res['sgpr_spills']:11d} "
                f"{res['lds_bytes']:6d}  {prog.ring_loss_grad_kernel_symbol()}")
            say("#   all timings ms: " + "; ".join(f"{k} " + " ".join(f"{t:.3f}" for t in v) for k, v in got.items()))
            say(f"#   loss: route {vals['route']:.9g}, fused {vals['fused']:.9g}")
            del s0, st
        del x, target, y, gy
        torch.cuda.empty_cache()
    out = os.path.join(ROOT, "profiles", "r13", "ring_loss_grad.txt")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


FAR_REC_GRAPHS = {"far_comb": W.far_comb, "comb2000": _comb(2000)}


def rings_recording_bench(a, torch, far=False):
    """the squared-error backward of a whole recording of graphs with delay lines in LDS: the recording call, the one-launch call, and
    blocks chained by hand.  far: the same for graphs with delay lines in HBM, through the far family's calls"""
    import time
    lines = []
    fam = "far" if far else "ring"
    call = lambda prog, what: getattr(prog, what.replace("ring", fam))   # noqa: E731  (the family's method of that name)

    def say(line):
        print(line, flush=True)
        lines.append(line)
    props = torch.cuda.get_device_properties(0)
    say(f"# command: tools/grad_bench.py {'--far' if far else '--rings'} --recording --steps {a.steps} --legs {a.legs}")
    say(f"# date {datetime.date.today().isoformat()}, board {props.name or 'unnamed'} ({getattr(props, 'gcnArchName', '?')})")
    say(f"# rec = one run_recording_{fam}_loss_grad call; one = one run_block_{fam}_loss_grad launch over all rows (where its workspace fits);")
    say(f"# route = run_block per block into a scratch y for the states, then run_block_{fam}_loss_grad per block in reverse (same B as rec); time-major frames")
    say(f"# HIP events, {a.steps} calls per leg and pass, a forward and a backward pass over the legs; spread = max - min of a leg's own repeats;")
    say("# mark = rec median <= route median + the route's spread")
    say(f"{'graph':16s} {'streams x T':>16s} {'B':>5s} {'route ms':>9s} {'spread':>7s} {'rec ms':>9s} {'spread':>7s} {'one ms':>9s} {'spread':>7s} "
        f"{'rec/route':>9s} {'rec/one':>8s} {'mark':>5s} {'ws rec MB':>10s} {'ws route MB':>11s} {'ws one MB':>10s}  {fam} states kernel")
    shapes = REC_SHAPES["small"] + REC_SHAPES["large"] if a.legs == "all" else REC_SHAPES[a.legs]
    want = ("x", "state", "params", "consts", "loss")
    for ns, T in shapes:
        x = torch.empty((T, ns, 1), dtype=torch.float32, device="cuda")
        F.synth_fill(x, seed=W.SEED)
        target = torch.empty_like(x)
        F.synth_fill(target, seed=W.SEED + 1)
        n = float(ns) * T
        for name, fn in (FAR_REC_GRAPHS if far else RING_GRAPHS).items():
            prog = F.compile(F.from_sexpr(fn()))
            s0 = torch.zeros((prog.n_state, ns), dtype=torch.float32, device="cuda")
            B = call(prog, "ring_recording_block_rows")(T)
            nb = (T + B - 1) // B
            ws_rec, ws_one = call(prog, "ring_recording_workspace_bytes")(ns, T), call(prog, "ring_grad_workspace_bytes")(ns, T)
            # the route keeps the state before every block itself, a scratch y of one block, and one block's ring workspace
            ws_route = nb * prog.n_state * ns * 4 + B * ns * prog.n_out * 4 + call(prog, "ring_grad_workspace_bytes")(ns, B)
            ws = torch.empty(ws_rec // 4, dtype=torch.float32, device="cuda")
            states = torch.empty((nb + 1, prog.n_state, ns), dtype=torch.float32, device="cuda")
            y = torch.empty((B, ns, 1), dtype=torch.float32, device="cuda")

            def rec():
                r = call(prog, "run_recording_ring_loss_grad")(x, target, s0, None, grad_scale=2.0 / n, want=want, workspace=ws)
                return r["loss"].double().sum() / n

            def route():
                states[0].copy_(s0)
                for k in range(nb):
                    rows = min(B, T - k * B)
                    states[k + 1].copy_(states[k])
                    prog.run_block(x[k * B:k * B + rows], state=states[k + 1], out=y[:rows])
                acc, sg = {}, None
                for k in range(nb - 1, -1, -1):
                    rows = min(B, T - k * B)
                    r = call(prog, "run_block_ring_loss_grad")(x[k * B:k * B + rows], target[k * B:k * B + rows], states[k], None, state_grad=sg,
                                                               grad_scale=2.0 / n, want=want, accum=acc)
                    # (the accumulators the next launch adds to: only those the graph has rows of)
                    acc, sg = {k: r[k] for k, rows_k in (("params", prog.n_param), ("consts", prog.n_const), ("loss", 1)) if rows_k}, r["state"]
                return acc["loss"].double().sum() / n

            def one():
                r = call(prog, "run_block_ring_loss_grad")(x, target, s0, None, grad_scale=2.0 / n, want=want)
                return r["loss"].double().sum() / n
            legs = {"route": route, "rec": rec}
            if ws_one + (4 << 30) < torch.cuda.mem_get_info()[0]:
                legs["one"] = one
            vals = {k: float(f()) for k, f in legs.items()}        # JIT, allocator; and the legs agree on the loss
            assert all(v == vals["rec"] for v in vals.values()), vals     # (bit for bit: the same per-stream sums)
            torch.cuda.synchronize()
            t_end = time.time() + 0.1
            while time.time() < t_end:                          # at least 100 ms of the yardstick before the first timing
                route()
                torch.cuda.synchronize()
            got = {k: [] for k in legs}
            for order in (list(legs), list(legs)[::-1]):
                for k in order:
                    got[k] += samples(legs[k], a.steps, torch)
            med = {k: float(np.median(v)) for k, v in got.items()}
            sp = {k: max(v) - min(v) for k, v in got.items()}
            one_s = f"{med['one']:9.3f} {sp['one']:7.3f}" if "one" in med else f"{'-':>9s} {'-':>7s}"
            ratio_one = f"{med['rec'] / med['one']:8.3f}" if "one" in med else f"{'-':>8s}"
            say(f"{name:16s} {f'{ns} x {T}':>16s} {B:5d} {med['route']:9.3f} {sp['route']:7.3f} {med['rec']:9.3f} {sp['rec']:7.3f} {one_s} "
                f"{med['rec'] / med['route']:9.3f} {ratio_one} {'yes' if med['rec'] <= med['route'] + sp['route'] else 'NO':>5s} {ws_rec / 2**20:10.1f} "
                f"{ws_route / 2**20:11.1f} {ws_one / 2**20:10.1f}  {call(prog, 'ring_states_kernel_symbol')()}")
            say("#   all timings ms: " + "; ".join(f"{k} " + " ".join(f"{t:.3f}" for t in v) for k, v in got.items()))
            del s0, ws, states, y
            torch.cuda.empty_cache()
        del x, target
        torch.cuda.empty_cache()
    out = os.path.join(ROOT, "profiles", "r18", "far_recording.txt") if far else os.path.join(ROOT, "profiles", "r14", "ring_recording.txt")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


def rings_recording_sm_bench(a, torch, far=False):
    """the backward of a whole recording of graphs with delay lines in LDS on stream-major buffers (plain, or with a.loss under the
    squared-error loss), alone (--layout stream-major) or against transpose + the time-major ring recording + transpose (--layout
    compare), interleaved in one process; the two legs agree bit for bit before a time is printed.  far: the same for graphs with delay
    lines in HBM, the far family's calls"""
    import time
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)
    props = torch.cuda.get_device_properties(0)
    loss, both = bool(a.loss), a.layout == "compare"
    call = "run_recording_" + ("far" if far else "ring") + ("_loss_grad" if loss else "_grad")
    sm_call = call + "(stream_major=True)" if far else call + "_stream_major"
    say(f"# command: tools/grad_bench.py {'--far' if far else '--rings'} --recording --layout {a.layout}{' --loss' if loss else ''} --steps {a.steps} --legs {a.legs}")
    say(f"# date {datetime.date.today().isoformat()}, board {props.name or 'unnamed'} ({getattr(props, 'gcnArchName', '?')})")
    say(f"# sm = one {sm_call} call on [n_streams, T] buffers; route = fz_transpose_frames of x and of {'the target' if loss else 'dL/dy'}, {call}, fz_transpose_frames of dL/dx back;")
    say(f"# every gradient, default checkpoint stride and B; HIP events, {a.steps} calls per leg and pass, a forward and a backward pass over the legs;")
    say("# spread = max - min of the route's own repeats; the legs agree bit for bit (dL/dx, the state gradient" + (", the loss" if loss else "") + ") before a time is printed;")
    say("# slower = sm median > route median + the route's spread")
    say(f"{'graph':16s} {'streams x T':>16s} {'B':>5s} {'route ms':>9s} {'spread':>7s} {'sm ms':>9s} {'sm/route':>9s} {'slower':>6s} {'ws MB':>9s} {'U':>3s} {'R':>3s} {'lanes':>5s} {'vgprs':>6s} "
        f"{'sgpr spills':>11s} {'lds':>6s}  stream-major {'far' if far else 'ring'} states kernel")
    shapes = REC_SHAPES["small"] + REC_SHAPES["large"] if a.legs == "all" else REC_SHAPES[a.legs]
    for ns, T in shapes:
        x_sm = torch.empty((ns, T, 1), dtype=torch.float32, device="cuda")
        F.synth_fill(x_sm, seed=W.SEED)
        yt_sm = torch.empty_like(x_sm)                         # dL/dy, or the target
        F.synth_fill(yt_sm, seed=W.SEED + 1)
        gx_sm = torch.empty_like(x_sm)
        if both:
            gx_back = torch.empty_like(x_sm)
            x_tm, yt_tm = (torch.empty((T, ns, 1), dtype=torch.float32, device="cuda") for _ in range(2))
        n = float(ns) * T
        want = ("x", "state", "params", "consts") + (("loss",) if loss else ())
        for name, fn in ({k: v for k, v in FAR_GRAPHS.items() if k != "comb256"} if far else RING_GRAPHS).items():
            prog = F.compile(F.from_sexpr(fn()))
            s0 = torch.zeros((prog.n_state, ns), dtype=torch.float32, device="cuda")
            if far:
                B, ws_bytes = prog.far_recording_block_rows(T), prog.far_recording_workspace_bytes(ns, T)
            else:
                B, ws_bytes = prog.ring_recording_block_rows(T), prog.ring_recording_workspace_bytes(ns, T)
            ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device="cuda")
            kw = dict(grad_scale=2.0 / n) if loss else {}

            def route():
                F.frames_from_stream_major(x_sm, 0, out=x_tm)
                F.frames_from_stream_major(yt_sm, 0, out=yt_tm)
                r = getattr(prog, call)(x_tm, yt_tm, s0, None, state_grad=s0, want=want, workspace=ws, **kw)
                F.frames_to_stream_major(r["x"], out=gx_back)
                return r

            def sm():
                if far:
                    return getattr(prog, call)(x_sm, yt_sm, s0, None, state_grad=s0, want=want, in_grad=gx_sm, workspace=ws, stream_major=True, **kw)
                return getattr(prog, call + "_stream_major")(x_sm, yt_sm, s0, None, state_grad=s0, want=want, in_grad=gx_sm, workspace=ws, **kw)
            legs = {"route": route, "sm": sm} if both else {"sm": sm}
            first = {k: f() for k, f in legs.items()}           # JIT, allocator; and the legs agree bit for bit
            torch.cuda.synchronize()
            if both:
                same = lambda u, v: torch.equal(u.view(torch.int32), v.view(torch.int32))   # noqa: E731
                assert same(gx_sm, gx_back), f"{name} {ns} x {T}: dL/dx of the two legs differs"
                for key in ("state",) + (("loss",) if loss else ()):
                    assert same(first["sm"][key], first["route"][key]), f"{name} {ns} x {T}: {key} of the two legs differs"
            del first
            yard = legs["route" if both else "sm"]
            t_end = time.time() + 0.1
            while time.time() < t_end:                          # at least 100 ms of the yardstick before the first timing
                yard()
                torch.cuda.synchronize()
            got = {k: [] for k in legs}
            for order in (list(legs), list(legs)[::-1]):
                for k in order:
                    got[k] += samples(legs[k], a.steps, torch)
            med = {k: float(np.median(v)) for k, v in got.items()}
            res, sym = (prog.far_states_resources if far else prog.ring_states_resources)(stream_major=True), \
                (prog.far_states_kernel_symbol if far else prog.ring_states_kernel_symbol)(stream_major=True)
            R, lanes = int(sym.split("_g")[0].split("r")[-1].split("b")[0]), int(sym.split("_g")[0].split("b")[-1])
            if both:
                spread = max(got["route"]) - min(got["route"])
                vs = f"{med['route']:9.3f} {spread:7.3f} {med['sm']:9.3f} {med['sm'] / med['route']:9.3f} {'YES' if med['sm'] > med['route'] + spread else 'no':>6s}"
            else:
                vs = f"{'-':>9s} {'-':>7s} {med['sm']:9.3f} {'-':>9s} {'-':>6s}"
            say(f"{name:16s} {f'{ns} x {T}':>16s} {B:5d} {vs} {ws_bytes / 2**20:9.1f} {res['unroll']:3d} {R:3d} {lanes:5d} {res['vgprs'] + res['agprs']:6d} "
                f"{res['sgpr_spills']:11d} {res['lds_bytes']:6d}  {sym}")
            say("#   all timings ms: " + "; ".join(f"{k} " + " ".join(f"{t:.3f}" for t in v) for k, v in got.items()))
            del s0, ws
            torch.cuda.empty_cache()
        del x_sm, yt_sm, gx_sm
        if both:
            del gx_back, x_tm, yt_tm
        torch.cuda.empty_cache()
    out = os.path.join(ROOT, "profiles", "r20", "far_sm_recording.txt") if far else os.path.join(ROOT, "profiles", "r16", "ring_sm_recording.txt")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "a" if loss and os.path.exists(out) else "w") as f:
        f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--legs", choices=("small", "large", "all"), default="all")
    ap.add_argument("--layout", choices=("time-major", "stream-major", "compare"), default="time-major")
    ap.add_argument("--loss", action="store_true", help="the fused squared-error backward against forward + torch MSE + backward, both layouts")
    ap.add_argument("--recording", action="store_true", help="the backward of a whole recording against the one-launch call and blocks chained by hand")
    ap.add_argument("--rings", action="store_true", help="forward against the ring backward of graphs with delay lines deeper than 8 samples; with --loss: their fused squared-error backward against the route; with --recording: the backward of a whole recording of them")
    ap.add_argument("--far", action="store_true", help="forward against the far backward of graphs with delay lines deeper than 256 samples, the LDS ring kernel on a 256-sample comb next to them; with --recording: the backward of a whole recording of them against the one-launch call and blocks chained by hand")
    a = ap.parse_args()
    import torch

    torch.cuda.set_device(0)
    if a.far and a.recording and a.layout != "time-major":
        return rings_recording_sm_bench(a, torch, far=True)
    if a.far and a.recording:
        return rings_recording_bench(a, torch, far=True)
    if a.far and a.layout == "compare":
        return rings_compare_bench(a, torch, far=True)
    if a.far:
        return far_bench(a, torch)
    if a.rings and a.recording and a.layout != "time-major":
        return rings_recording_sm_bench(a, torch)
    if a.rings and a.recording:
        return rings_recording_bench(a, torch)
    if a.rings and a.layout == "compare":
        return rings_compare_bench(a, torch)
    if a.rings and a.loss:
        return rings_loss_bench(a, torch)
    if a.loss:
        return loss_bench(a, torch)
    if a.recording:
        return recording_bench(a, torch)
    if a.rings:
        return rings_bench(a, torch)
    props = torch.cuda.get_device_properties(0)
    if a.layout == "compare":
        print(f"# date {datetime.date.today().isoformat()}, board {props.name or 'unnamed'} ({getattr(props, 'gcnArchName', '?')})")
        return compare(a, torch)
    sm = a.layout == "stream-major"
    print(f"# backward vs forward of one block, HIP events, median of {a.steps} launches after {a.warmup} warm-up")
    print(f"# date {datetime.date.today().isoformat()}, board {props.name or 'unnamed'} ({getattr(props, 'gcnArchName', '?')})")
    print(f"{'graph':20s} {'streams x T':>16s} {'fwd ms':>9s} {'bwd ms':>9s} {'bwd/fwd':>8s} {'C':>3s} {'vgprs':>6s} {'bwd B/s / 8TB/s':>16s}  adjoint kernel")
    shapes = SHAPES["small"] + SHAPES["large"] if a.legs == "all" else SHAPES[a.legs]
    for ns, T in shapes:
        x = torch.empty((ns, T, 1) if sm else (T, ns, 1), dtype=torch.float32, device="cuda")
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
                (prog.run_block_stream_major if sm else prog.run_block)(x, state=st, params=pp, out=y)
            fwd_ms = timed(fwd, a.warmup, a.steps, torch)
            # (the state copy is inside the forward's window: n_state rows, < 1 % of a block's bytes)
            bwd = prog.run_block_grad_stream_major if sm else prog.run_block_grad
            bwd_ms = timed(lambda: bwd(x, gy, s0, pp, state_grad=s0), a.warmup, a.steps, torch)
            res = prog.grad_resources(stream_major=sm)
            C = res["unroll"]
            nbytes = 4.0 * ns * T * (2 * prog.n_in + prog.n_out + prog.n_in) + 8.0 * ns * T * prog.n_state / C \
                + 4.0 * ns * (2 * prog.n_state + prog.n_param * 2 + prog.n_const * 2)
            print(f"{name:20s} {f'{ns} x {T}':>16s} {fwd_ms:9.3f} {bwd_ms:9.3f} {bwd_ms / fwd_ms:8.2f} {C:3d} {res['vgprs'] + res['agprs']:6d} "
                  f"{nbytes / (bwd_ms / 1e3) / HBM:16.3f}  {prog.grad_kernel_symbol(stream_major=sm)}", flush=True)
            del pp, s0, st
        del x, gy, y
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
