"""Every stream and every sample of the full-size bench workloads against the compiled oracle (MI355X).

One test per group of tests/full_legs.py: its legs (frame layouts of one workload, seed and stream range) run the library's static default
(FLOWZ_HIP_AUTOTUNE=0, FLOWZ_HIP_NO_PLAN_CACHE=1), each asserts its kernel name and that its final state equals an explicitly chosen
second variant's, then tests/full_check.py compares the whole output of every leg with one oracle pass, bit for bit.  The sampled and
variant-equality checks of test_gpu_parity.py stay as they are; these add the streams between the samples."""
import time

import numpy as np
import pytest

import full_check as FC
import full_legs as FL
from zignal_amd import flowz as F

pytestmark = pytest.mark.gpu

GiB = 1 << 30
DEVICE_BUDGET = 100 * GiB                       # a group's peak device memory: its kept outputs plus one input at a time
SENTINEL = -3.0e38                              # what an output holds before the launch: a stream the kernel skips cannot pass


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    torch.cuda.set_device(0)
    return torch


@pytest.fixture(autouse=True)
def static_default(monkeypatch):
    monkeypatch.setenv("FLOWZ_HIP_AUTOTUNE", "0")              # the static choice, whatever a first launch would measure on this board
    monkeypatch.setenv("FLOWZ_HIP_NO_PLAN_CACHE", "1")


def device_input(torch, workload, seed, layout, ns, T, tile):
    """the leg's input frames from the device generator (or the dirac drive); stream-major buffers are filled a chunk of streams at a
    time, so that no second full-size copy exists"""
    n_in, drive = FL.WORKLOADS[workload][2:4]
    if layout == "sm":
        x = torch.empty((ns, T, n_in), dtype=torch.float32, device="cuda")
        if drive == "dirac":
            x.zero_()
            x[:, 0] = 1.0
            return x
        ch = 1 << 16
        tmp = torch.empty((T, ch, n_in), dtype=torch.float32, device="cuda")
        for c0 in range(0, ns, ch):
            c = min(ch, ns - c0)
            t = tmp[:, :c] if c == ch else torch.empty((T, c, n_in), dtype=torch.float32, device="cuda")
            F.synth_fill(t, seed, stream0=c0)
            F.frames_to_stream_major(t, out=x[c0:c0 + c])
        return x
    x = torch.empty((ns // tile, T, tile, n_in) if tile else (T, ns, n_in), dtype=torch.float32, device="cuda")
    if drive == "dirac":
        x.zero_()
        (x[:, 0] if tile else x[0]).fill_(1.0)
    else:
        F.synth_fill(x, seed)
    return x


def input_slice(torch, workload, seed, T):
    """fetch_input of a leg: the device generator's frames of streams [s0, s1), stream-major (the leg's own input is freed after its launch)"""
    n_in, drive = FL.WORKLOADS[workload][2:4]

    def f(s0, s1):
        x = torch.zeros((T, s1 - s0, n_in), dtype=torch.float32, device="cuda")
        if drive == "dirac":
            x[0] = 1.0
        else:
            F.synth_fill(x, seed, stream0=s0)
        return x.permute(1, 0, 2).contiguous().cpu().numpy()
    return f


def launch(prog, layout, x, out, state, params, v):
    if layout == "sm":
        prog.run_block_stream_major(x, state=state, params=params, out=out, variant=F.make_variant(*v) if v else None)
    else:
        prog.run_block(x, state=state, params=params, out=out, variant=F.make_variant(*v) if v else None)


def run_group(torch, group):
    """run the group's legs on the device and check every output -> (Report, final states that differ from the second variant's,
    seconds on the device, peak device bytes)"""
    name, _, workload, seed, ns, T, legs = group
    prog = FL.program(workload)
    pfn = FL.WORKLOADS[workload][5]
    t0 = time.perf_counter()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    checked, state_diffs = [], []
    x = y = st = st2 = params = None
    try:
        params = torch.from_numpy(pfn(seed, np.arange(ns))).cuda() if pfn else None
        for layout, tile, kernel in legs:
            assert FL.kernel_name(prog, layout, ns, T, tile) == kernel, (name, layout)
            x = device_input(torch, workload, seed, layout, ns, T, tile)
            oshape = (ns, T, prog.n_out) if layout == "sm" else ((ns // tile, T, tile, prog.n_out) if tile else (T, ns, prog.n_out))
            y = torch.empty(oshape, dtype=torch.float32, device="cuda")
            st2 = torch.zeros((max(prog.n_state, 1), ns), dtype=torch.float32, device="cuda")
            launch(prog, layout, x, y, st2, params, FL.SECOND[layout])           # the second variant first, into the same output buffer
            y.fill_(SENTINEL)
            st = torch.zeros_like(st2)
            launch(prog, layout, x, y, st, params, None)                         # the library's static default
            torch.cuda.synchronize()
            if not torch.equal(st.view(torch.int32), st2.view(torch.int32)):
                state_diffs.append(f"{name} {layout} [{kernel}]: final state differs from {FL.kernel_name(prog, layout, ns, T, tile, FL.SECOND[layout])}'s")
            x = st = st2 = None                                                  # (inputs go before the next leg's: 64 GiB each for config 3)
            fetch = FC.stream_major(y) if layout == "sm" else (FC.tiles(y) if tile else FC.rows(y))
            checked.append(FC.Leg(f"{name} {layout}", kernel, fetch, input_slice(torch, workload, seed, T)))
        t_dev = time.perf_counter() - t0
        tiles = [t for _, t, _ in legs if t]
        k = FC.slice_streams(T, max(FL.WORKLOADS[workload][2], prog.n_out), min(tiles) if tiles else 0)
        rep = FC.check(checked, FL.reference(workload, seed, T), ns, k)
        for r in rep.legs:
            r.leg = FC.Leg(r.leg.name, r.leg.kernel, None)                       # (the report keeps names, not device buffers)
        return rep, state_diffs, t_dev, torch.cuda.max_memory_allocated()
    finally:                                                                     # (a failure's traceback keeps this frame, not the buffers)
        x = y = st = st2 = params = None
        checked.clear()
        torch.cuda.empty_cache()


@pytest.mark.parametrize("group", FL.GROUPS, ids=[g[0] for g in FL.GROUPS])
def test_full_output_vs_oracle(torch_cuda, group):
    t0 = time.perf_counter()
    rep, state_diffs, t_dev, peak = run_group(torch_cuda, group)
    name, _, _, _, ns, T, legs = group
    print(f"\n[full-output] {name}: {len(legs)} legs, {ns} streams x {T}: {time.perf_counter() - t0:.1f} s ({t_dev:.1f} s on the device), "
          f"{rep.n_threads} threads, {rep.slice_streams} streams per slice, peak device memory {peak / GiB:.1f} GiB")
    assert rep.ok, str(rep)
    assert not state_diffs, state_diffs
    assert peak <= DEVICE_BUDGET, (name, peak / GiB)
