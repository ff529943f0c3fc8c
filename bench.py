#!/usr/bin/env python3
"""Headline benchmark: 6-stage biquad (DF1) cascade, 1 M streams x 4096-sample blocks per GPU.

Contract (driver): `python bench.py --gpus N --steps K --warmup W`; for N > 1 it is launched by
torch.distributed.run with one rank per GPU.  One "step" = one fz_run_block launch = one
4096-sample block of every stream of this rank (state carried from step to step), input frames
already resident in HBM.  Rank 0 prints ONE JSON line.

A plain run does only what the headline needs: set-up and plan selection, the warm-up and the K timed steps,
--dump-outputs, the line.  Everything else the line can carry -- oracle parity, the sustained run, the row-walk and copy
yardsticks, the CPU baseline, the other configs and layouts -- is measured with --full (every --no-* option but --no-autotune
trims it there).

  value      whole-job Msamples/s = streams(all ranks) * 4096 * K / max-over-ranks wall time
  roofline   dominant kernel fz_block_kernel: algorithmic bytes per launch / its average launch
             duration = HIP-event time over the K back-to-back launches of the timed region / K,
             events recorded on the launch stream (torch's current stream, which run_block uses);
             peak = 8000 GB/s (HBM3E spec, /opt/skills/guides/MI355X_MICROARCH.md);
             traffic = PMC bytes of THIS kernel symbol on THIS workload (profiles/pmc_traffic.json,
             collected by tools/profile_bench.sh, keyed by the kernel's code id), null when that code was not profiled;
             measured_row_walk_GBs / measured_copy_GBs (--full) = the identity graph and a plain copy on the same frames;
             sustained (--full) = the same launches back to back for >= 2 s (power-managed clocks settle), with
             sustained.board = package power / power cap / shader clock sampled through rocm-smi meanwhile
             (this workload runs at the board's power cap: profiles/r03/power_and_clocks.txt)
  cpu_baseline  (--full) the compiled scalar oracle (one closure per stream, one call per sample: what
             the reference's compile()-callable does) timed on this box's host cores on a
             bounded sample of the same workload, rank 0, N == 1 only (buffers pre-touched, threads
             pinned); the oracle also checks the GPU output of >= 1024 random streams bit for bit.
  config2/3/4   (--full) the other single-GPU BASELINE configs at full size in the same run (rank 0, N == 1):
             library-default and tuned plan, roofline fraction, oracle parity on >= 1024 random streams.

--dump-outputs DIR writes what the headline's last timed step returned (rank 0's shard) as float32 .npy files, at most
64 MB in all: see dump_outputs().  The inputs are seeded, so two builds run with the same arguments can be compared file by file.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
# every run measures for itself: plans persisted by an earlier process on this board (plans.txt of the kernel cache) would
# turn "library_default" into "whatever was tuned last time"
os.environ.setdefault("FLOWZ_HIP_NO_PLAN_CACHE", "1")

HBM_PEAK_GBS = 8000.0
PARITY_STREAMS = 1024
PARITY_STREAMS_OTHER_RANKS = 128
DUMP_BYTES = 64 << 20                                        # --dump-outputs: bytes of all files together
DUMP_SEED = 5


def load_oracle():
    """The compiled oracle that the parity checks and the CPU baseline call: oracle/libflowz_oracle.so and libflowz_oracle_std.so, which
    build() makes.  coracle would make a missing one in place, which fails in a tree that cannot be written; bench.py compiles it with
    oracle/Makefile into a temporary directory instead and hands coracle the loaded library."""
    import ctypes
    import shutil
    import subprocess
    import tempfile

    from oracle import coracle

    here = os.path.join(ROOT, "oracle")
    missing = [n for n in ("libflowz_oracle.so", "libflowz_oracle_std.so") if not os.path.exists(os.path.join(here, n))]
    if not missing:
        return
    tmp = tempfile.mkdtemp(prefix="bench_oracle_")
    try:
        subprocess.check_call(["make", "-s", "-C", tmp, "-f", os.path.join(here, "Makefile"), "VPATH=" + here] + missing)
        libs = {n: ctypes.CDLL(os.path.join(tmp, n)) for n in missing}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)                # (a loaded library stays mapped)
    coracle._LIB = libs.get("libflowz_oracle.so", coracle._LIB)
    coracle._LIB_STD = libs.get("libflowz_oracle_std.so", coracle._LIB_STD)


# ---- CPU baseline --------------------------------------------------------------------------------------------------
def cpu_topology():
    """(logical cpus this process may use, one logical cpu per physical core among them, cgroup CPU quota in cores or None)."""
    avail = sorted(os.sched_getaffinity(0))
    core_of = {}
    try:
        cpu = phys = core = None
        for ln in open("/proc/cpuinfo"):
            k, _, v = ln.partition(":")
            k = k.strip()
            if k == "processor":
                cpu, phys, core = int(v), 0, None
            elif k == "physical id":
                phys = int(v)
            elif k == "core id":
                core = int(v)
                core_of[cpu] = (phys, core)
    except OSError:
        pass
    seen, one_per_core = set(), []
    for c in avail:
        key = core_of.get(c, ("?", c))
        if key not in seen:
            seen.add(key)
            one_per_core.append(c)
    # a container may be allowed fewer CPU-seconds per second than it sees CPUs (cgroup v2 cpu.max / v1 cfs quota): more
    # runnable threads than that only get throttled
    quota = None
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            quota = float(q) / float(per)
    except (OSError, ValueError):
        try:
            q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0:
                quota = q / per
        except (OSError, ValueError):
            pass
    return avail, one_per_core, quota


def _cpu_threads_run(coracle, coefs, cpus, per_thread, n_samples, seed, reps=1, soa=False):
    """One pinned thread per entry of `cpus`; every thread generates and first-touches its own buffers, then all
    start together.  Returns (wall seconds of the timed part, outputs of thread 0)."""
    import threading

    import numpy as np

    n = len(cpus)
    gate = threading.Barrier(n)
    t_begin, t_end, outs, errs = [0.0] * n, [0.0] * n, [None] * n, []

    def work(i):
        try:
            try:
                os.sched_setaffinity(0, {cpus[i]})           # pid 0 = the calling thread
            except OSError:
                pass
            if soa:                                          # "Mode B": time-major SoA frames [T, streams]
                x = coracle.synth_fill(seed, i * per_thread, per_thread, n_samples)
            else:                                            # one contiguous buffer per stream (the CPU-friendly layout)
                x = coracle.synth_fill(seed, i * per_thread, per_thread, n_samples, stream_major=True)
            y = np.empty_like(x)
            y.fill(0.0)                                      # pages mapped by the thread that will write them
            gate.wait()
            t_begin[i] = time.perf_counter()
            for _ in range(reps):
                if soa:
                    coracle.df1_cascade_soa(coefs, x, out=y)
                else:
                    coracle.df1_cascade(coefs, x, stream_major=True, out=y)
            t_end[i] = time.perf_counter()
            outs[i] = y if i == 0 else None
        except Exception as e:                               # pragma: no cover
            errs.append(e)
            try:
                gate.abort()
            except Exception:
                pass

    ths = [threading.Thread(target=work, args=(i,)) for i in range(n)]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    if errs:
        raise errs[0]
    return max(t_end) - min(t_begin), outs[0]


def cpu_baseline(n_samples, seed, coefs):
    """Time the compiled oracle on the host cores (SURVEY 8d Mode A, plus Mode B next to it)."""
    import numpy as np

    from oracle import coracle

    logical, physical, quota = cpu_topology()
    # single-thread calibration (pre-touched buffers): sizes the sample and is the per-thread yardstick
    x0 = coracle.synth_fill(seed, 0, 64, n_samples, stream_major=True)
    y0 = np.zeros_like(x0)
    y0.fill(0.0)
    coracle.df1_cascade(coefs, x0, stream_major=True, out=y0)
    t0 = time.perf_counter()
    coracle.df1_cascade(coefs, x0, stream_major=True, out=y0)
    rate1 = 64 * n_samples / (time.perf_counter() - t0)
    per_thread = 1024                                        # streams per thread (32 MiB of frames in + out), passed `reps` times
    reps = max(1, int(round(2.5 * rate1 / (per_thread * n_samples))))               # ~2.5 s per thread
    # How many threads can this box actually RUN?  Containers often see every CPU of the host but are granted far fewer
    # CPU-seconds per second (cgroup quota, or an over-committed VM): runnable threads beyond that are only throttled
    # and depress the per-thread figure.  Read the quota where it is published, and probe the scaling in any case:
    # short runs with 1, 2, 4 ... threads (one per physical core) until the aggregate rate stops growing.
    probe_reps = max(1, int(round(0.3 * rate1 / (per_thread * n_samples))))
    scaling, n_eff, best_rate, n = {}, 1, 0.0, 1
    cap = len(physical) if quota is None else max(1, min(len(physical), int(quota)))
    while n <= cap:
        wall, _ = _cpu_threads_run(coracle, coefs, physical[:n], per_thread, n_samples, seed, reps=probe_reps)
        rate = n * per_thread * n_samples * probe_reps / wall
        scaling[n] = round(rate / 1e6, 1)
        if rate < best_rate * 1.15:
            break
        n_eff, best_rate = n, rate
        if n == cap:
            break
        n = min(cap, n * 2)
    plans = [(f"{n_eff}_pinned_threads_on_distinct_physical_cores", physical[:n_eff])]
    if n_eff < len(physical):
        plans.append(("one_thread_per_physical_core", physical))
    elif len(logical) > len(physical):
        plans.append(("one_thread_per_logical_cpu", logical))
    runs = {}
    for label, cpus in plans:
        r = max(1, int(reps * min(1.0, n_eff / len(cpus))))                          # bounded: ~2.5 s wall either way
        wall, _ = _cpu_threads_run(coracle, coefs, cpus, per_thread, n_samples, seed, reps=r)
        tot = len(cpus) * per_thread * n_samples * r
        runs[label] = {"threads": len(cpus), "Msamples_per_s": round(tot / wall / 1e6, 1),
                       "Msamples_per_s_per_thread": round(tot / wall / 1e6 / len(cpus), 3), "wall_s": round(wall, 2),
                       "streams": len(cpus) * per_thread, "passes": r}
    best = max(runs, key=lambda k: runs[k]["Msamples_per_s"])
    b = runs[best]
    # `cores` = the cores the reported run could actually OCCUPY: its threads, capped by the CPU-seconds per second the cgroup
    # grants (256 logical CPUs under a quota of 16 are 16 cores' worth of work however many threads are runnable); the per-core
    # rate is the aggregate over those, so that it stays comparable with the single-thread calibration
    cores = b["threads"] if quota is None else max(1, min(b["threads"], int(round(quota))))
    base = {"value": b["Msamples_per_s"], "unit": "Msamples/s", "cores": cores, "kind": "port",
            "Msamples_per_s_per_core": round(b["Msamples_per_s"] / cores, 3), "threads": b["threads"],
            "single_thread_calibration_Msamples_per_s": round(rate1 / 1e6, 3),
            "physical_cores": len(physical), "logical_cpus": len(logical), "cgroup_cpu_quota": quota, "thread_scaling_probe_Msamples_per_s": scaling,
            "threads_pinned": True, "runs": runs,
            "sample": f"{b['streams']} streams x {n_samples} samples x {b['passes']} passes ({best}: {b['threads']} pinned threads on {cores} cores' worth of CPU time), 6-stage DF1 cascade, "
                      f"scalar closure per stream, one call per sample (oracle/flowz_oracle.c, gcc -O3 -ffp-contract=off), "
                      f"buffers allocated and first-touched by their thread before the timed region, {b['wall_s']:.2f} s wall"}
    # "Mode B" (SURVEY 8d): the same closures vectorised ACROSS streams by the compiler (SoA state, avx2/avx512
    # clones) -- a CPU stronger than the reference's scalar closure, reported next to it
    try:
        vec_streams, reps_v = 1024, 12                         # per thread: 16 MiB of frames
        xv = coracle.synth_fill(seed, 0, 256, n_samples)
        ok_vec = bool(np.array_equal(coracle.df1_cascade_soa(coefs, xv).view(np.uint32), coracle.df1_cascade(coefs, xv).view(np.uint32)))
        cpus = dict(plans)[best]
        reps = max(1, int(reps_v * min(1.0, n_eff / len(cpus))))
        wall_v, _ = _cpu_threads_run(coracle, coefs, cpus, vec_streams, n_samples, seed, reps=reps, soa=True)
        base["vectorised_across_streams"] = {
            "value": round(len(cpus) * vec_streams * reps * n_samples / wall_v / 1e6, 1), "unit": "Msamples/s",
            "cores": len(cpus) if quota is None else max(1, min(len(cpus), int(round(quota)))), "threads": len(cpus),
            "bitwise_equal_to_scalar": ok_vec,
            "note": "same arithmetic per stream, SoA state, compiler-vectorised (stronger than the reference's scalar closure)"}
    except Exception as e:                                  # never let the extra figure break the bench line
        base["vectorised_across_streams"] = {"error": str(e)[:200]}
    # The reference's OWN code next to the port, one thread: six of its hand-written DF1 closures in series (test/benchmark.cpp:35-47, its coefficients :18-23),
    # compiled from the reference sources by oracle/build_ref.sh into oracle/_ref/ (the checker's library: it travels with the tree, the sources do not).
    # Not the compile()-callable either -- that needs Boost -- but reference code: it shows what the port's single-thread figure is worth.
    try:
        import ctypes
        so = os.path.join(ROOT, "oracle", "_ref", "libzignal_ref.so")
        if os.path.exists(so):
            ref = ctypes.CDLL(so)
            ref.zref_df1x6.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
            xr = np.ascontiguousarray(x0[:, :, 0] * np.float32(1e-3))                # [64 streams][n_samples]; small: the reference's coefficient set has a pole at z = -1
            yr = np.zeros_like(xr)
            run = lambda: [ref.zref_df1x6(xr[s].ctypes.data, yr[s].ctypes.data, n_samples) for s in range(xr.shape[0])]   # noqa: E731
            run()
            t0, n = time.perf_counter(), 0
            while time.perf_counter() - t0 < 0.5:
                run()
                n += 1
            base["reference_code_single_thread"] = {
                "value": round(n * xr.shape[0] * n_samples / (time.perf_counter() - t0) / 1e6, 3), "unit": "Msamples/s", "cores": 1,
                "what": "six of the reference's hand-written DF1 closures in series (test/benchmark.cpp:35-47 built by oracle/build_ref.sh), one call per sample; "
                        "the port's single-thread figure is single_thread_calibration_Msamples_per_s"}
    except Exception as e:
        base["reference_code_single_thread"] = {"error": str(e)[:200]}
    return base

# ---- GPU side helpers ----------------------------------------------------------------------------------------------
def frames(torch, dev, ns, T, w, tile):
    return torch.empty((ns // tile, T, tile, w) if tile else (T, ns, w), dtype=torch.float32, device=dev)


def pick_tile(ns, tile):
    return tile if tile and ns % tile == 0 and tile < ns else 0


def event_ms(torch, fn, reps):
    """HIP events on the launch stream around `reps` back-to-back launches -> ms per launch."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def rocm_smi_card_of(torch, dev_index):
    """rocm-smi's card index of torch's LOGICAL device `dev_index`: under HIP_VISIBLE_DEVICES / ROCR_VISIBLE_DEVICES (leased boxes)
    the two differ, so the board is found by its PCI bus id (rocm-smi --showbus).  None when it cannot be told."""
    import re
    import shutil
    import subprocess

    exe = shutil.which("rocm-smi") or ("/opt/rocm/bin/rocm-smi" if os.path.exists("/opt/rocm/bin/rocm-smi") else None)
    if not exe:
        return None, None
    try:
        p = torch.cuda.get_device_properties(dev_index)
        want = f"{getattr(p, 'pci_domain_id', 0):04x}:{p.pci_bus_id:02x}:{p.pci_device_id:02x}".lower()
        o = json.loads(subprocess.run([exe, "--showbus", "--json"], capture_output=True, text=True, timeout=10).stdout)
        cards = []
        for card, c in o.items():
            m = re.match(r"card(\d+)", card)
            bus = next((str(v).lower() for k, v in c.items() if "PCI Bus" in k), "")
            if m:
                cards.append(int(m.group(1)))
                if bus.startswith(want):
                    return exe, int(m.group(1))
        if len(cards) == 1:                                   # one visible board: nothing to confuse
            return exe, cards[0]
    except Exception:  # noqa: BLE001
        pass
    return exe, None


class PowerSampler:
    """Board power and shader clock (rocm-smi) sampled in a thread while a sustained leg runs: the 6-biquad cascade at 1 M streams
    sits at the package power cap and the firmware lowers the clock until it fits (profiles/r03/power_and_clocks.txt), so a run's
    number is also a statement about the board.  The board is torch's device mapped to rocm-smi's card by PCI bus id; one sample
    per second (a rocm-smi process each).  Best effort: None when rocm-smi is missing, the board cannot be told or it prints
    something else."""

    def __init__(self, torch, device_index=0, period=1.0):
        import threading
        self.exe, self.card = rocm_smi_card_of(torch, device_index)
        self.period, self.rows, self._stop = period, [], False
        self.thread = threading.Thread(target=self._run, daemon=True) if (self.exe and self.card is not None) else None

    def _run(self):
        import re
        import subprocess
        while not self._stop:
            try:
                o = subprocess.run([self.exe, "-d", str(self.card), "--showpower", "--showclocks", "--showmaxpower", "--json"],
                                   capture_output=True, text=True, timeout=5).stdout
                c = next(iter(json.loads(o).values()))
                watts = [float(v) for k, v in c.items() if "Power (W)" in k and "Max" not in k]
                cap = [float(v) for k, v in c.items() if "Max" in k and "Power (W)" in k]
                sclk = [int(re.search(r"(\d+)", v).group(1)) for k, v in c.items() if k.startswith("sclk clock speed")]
                if watts and sclk:
                    self.rows.append((time.perf_counter(), watts[0], cap[0] if cap else None, sclk[0]))
            except Exception:  # noqa: BLE001 -- a sampler must never take the bench down
                pass
            t_end = time.perf_counter() + self.period
            while not self._stop and time.perf_counter() < t_end:
                time.sleep(0.05)

    def start(self):
        if self.thread:
            self.thread.start()
        self.t0 = time.perf_counter()

    def stop(self, settle=0.5):
        self._stop = True
        if self.thread:
            self.thread.join(timeout=6)
        rows = [r for r in self.rows if r[0] - self.t0 >= settle] or self.rows
        if not rows:
            return None
        med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
        watts, cap = med([r[1] for r in rows]), rows[0][2]
        return {"package_W": watts, "cap_W": cap, "at_power_cap": bool(cap and watts >= 0.98 * cap), "sclk_MHz": med([r[3] for r in rows]),
                "samples": len(rows), "rocm_smi_card": self.card,
                "source": "rocm-smi --showpower --showclocks of the board with torch's PCI bus id, median over the sustained leg"}


def sustained_run(torch, fn, ms_est, dev_index, seconds=2.0, min_batch=1):
    """fn back to back for >= `seconds` of GPU time in batches of ~0.25 s (one HIP-event pair each), board power sampled meanwhile"""
    batch = max(min_batch, int(math.ceil(250.0 / max(ms_est, 1e-3))))
    n, ms_tot = 0, 0.0
    sampler = PowerSampler(torch, dev_index)
    sampler.start()
    while ms_tot < seconds * 1e3 and n < 4_000_000:
        ms_tot += event_ms(torch, fn, batch) * batch
        n += batch
    return n, ms_tot, sampler.stop()


def sample_ids(ns, k, seed):
    import numpy as np

    rng = np.random.default_rng(seed)
    edge = [i for i in (0, 1, 63, 64, ns - 1) if 0 <= i < ns]
    return np.unique(np.concatenate([edge, rng.integers(0, ns, k)]))


def dump_stream_ids(ns, k):
    """--dump-outputs: the fixed, seeded sample of k of the ns streams (sorted local indices; all of them when k >= ns)"""
    import numpy as np

    if k >= ns:
        return np.arange(ns)
    return np.sort(np.random.default_rng(DUMP_SEED).choice(ns, k, replace=False))


def dump_outputs(torch, path, y, state, tile):
    """What one run_block call returned -- out frames y and state -- as float32 .npy files under `path`:
      out_last_sample.npy  [streams, n_out]     the block's last sample of every stream (a seeded sample of the streams beyond 16 MB)
      out_streams.npy      [T, k, n_out]        every sample of the block for the seeded sample dump_stream_ids(ns, k)
      state_streams.npy    [n_state, k]         the state those k streams carry into the next block
    k is as many streams as fit in half of DUMP_BYTES."""
    import numpy as np

    ns, T, n_out = (y.shape[0] * y.shape[2], y.shape[1], y.shape[3]) if tile else (y.shape[1], y.shape[0], y.shape[2])
    last = (y[:, -1] if tile else y[-1]).reshape(ns, n_out)
    n_last = min(ns, DUMP_BYTES // 4 // (4 * n_out))
    if n_last < ns:
        last = last[torch.as_tensor(dump_stream_ids(ns, n_last), device=y.device)]
    k = max(1, min(ns, DUMP_BYTES // 2 // (4 * (T * n_out + state.shape[0]))))
    ids = dump_stream_ids(ns, k)
    arrays = {"out_last_sample": last.cpu().numpy(),
              "out_streams": gather(torch, y, ids, "tiled" if tile else "time_major", tile),
              "state_streams": state[:, torch.as_tensor(ids, device=state.device)].cpu().numpy()}
    if sum(a.nbytes for a in arrays.values()) > DUMP_BYTES:
        raise SystemExit(f"--dump-outputs: {T}-sample blocks do not fit in {DUMP_BYTES >> 20} MB")
    os.makedirs(path, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(path, name + ".npy"), np.ascontiguousarray(a, np.float32))


def ndiff_bits(a, b):
    import numpy as np

    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape, (a.shape, b.shape)
    return int((a.view(np.uint32) != b.view(np.uint32)).sum())


def parity_string(nd, n_streams, T):
    return f"bitwise-equal on {n_streams} random streams x {T} samples" if nd == 0 else f"MISMATCH {nd} samples"


def _profile_table(name):
    path = os.path.join(ROOT, "profiles", name)
    return json.load(open(path)) if os.path.exists(path) else {}


def counters_of(code_id, workload_key):
    """Counter-derived figures of EXACTLY this code on this workload, or ({}, None): profiles/pmc_traffic.json and sq_issue_share.json
    are keyed '<code id>|<workload>', the code id being the hash of (generated source, build options, compiler) that names the kernel's
    code object (fz_program_kernel_code_id) -- a kernel whose body changed since the counter passes has another id and reports null,
    never last week's numbers.  Returns ({"traffic": bytes per block, "issue_share": x}, "file(s) @ commit the passes ran on")."""
    out, src = {}, []
    for name, field in (("pmc_traffic.json", "traffic"), ("sq_issue_share.json", "issue_share")):
        e = _profile_table(name).get(f"{code_id}|{workload_key}")
        if isinstance(e, dict) and "value" in e:
            out[field] = e["value"]
            src.append(f"profiles/{name} ({e.get('batch', '?')} @ {e.get('commit', '?')})")
    return out, ("; ".join(src) if src else None)


def limiter_of(issue_share, board, frac_of_row_walk):
    """What holds a kernel back, as far as the run itself can tell: "issue" when the counter passes show its waves issuing
    in >= 60 % of their cycles (the lone wave of a SIMD: nothing left to overlap), "power" when the board sat at its package cap during the sustained
    run and the kernel is more than 3 % slower than the arithmetic-free row walk measured on the same box (the cap took the
    clock the arithmetic needed), else "hbm"."""
    if issue_share is not None and issue_share >= 0.60:
        return "issue"
    if board and board.get("at_power_cap") and frac_of_row_walk is not None and frac_of_row_walk < 0.97:
        return "power"
    return "hbm"



# ---- the line the driver parses ------------------------------------------------------------------------------------------
LINE_LIMIT = 4096                                            # bytes: the driver keeps the tail of stdout; round 4's 31 KB line did not survive it
CONTRACT_KEYS = ("metric", "value", "unit", "per_gpu", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                 "dtype", "data")
SHORT = {"config2_65536_streams": "config2", "cascade6_32768_streams": "cascade6_32768", "cascade6_16384_streams": "cascade6_16384",
         "config3_par4_sum": "config3", "config3_par4_sum_fanout": "config3_fanout", "config4_osc_chain": "config4",
         "ragged_counts": "ragged", "reference_benchmark_topologies": "ref", "next_rows": "", "other_shapes": "", "stream_major_layout": "stream_major",
         "tiled_layout": "tiled", "time_major_layout": "time_major"}


def flatten_legs(d, prefix=""):
    """(name, leg) for every leg object (a dict holding `library_default` or `forced`) below `d`, depth first; names are the
    path of keys, shortened by SHORT, joined with '_'"""
    out = []
    for k, v in d.items():
        if not isinstance(v, dict):
            continue
        name = SHORT.get(k, k)
        path = "_".join(x for x in (prefix, name) if x)
        if "library_default" in v or "forced" in v:
            # an object with sub-layouts names its own layout too: config2 -> config2_tiled, config2_time_major, config2_stream_major
            subs = {kk: vv for kk, vv in v.items() if kk in ("time_major", "stream_major", "other_shapes")}
            out.append((path + "_" + v.get("layout", "tiled") if ("time_major" in subs or "stream_major" in subs) else path, v))
            out += flatten_legs(subs, path)
        else:
            out += flatten_legs(v, path)
    return out


def compact_line(full, details_path=None):
    """The ONE line of stdout: the driver's contract keys, config, roofline, cpu_baseline, parity and one flat `summary` map
    {object: library-default fraction of the HBM peak}; everything else lives in bench_details.json.  Always < LINE_LIMIT bytes."""
    line = {k: full[k] for k in CONTRACT_KEYS if k in full}
    c = full.get("config", {})
    line["config"] = {k: c[k] for k in ("workload", "layout", "streams_per_gpu", "block_samples", "streams_total", "parallelism") if k in c}
    r = full.get("roofline", {})
    line["roofline"] = {k: r.get(k) for k in ("bound", "achieved", "peak", "unit", "frac", "kernel", "code_id", "workload_key", "algorithmic_bytes_per_launch", "avg_launch_ms", "traffic",
                                             "traffic_source", "limiter", "issue_share", "measured_row_walk_GBs", "frac_of_row_walk", "measured_copy_GBs")}
    sus = r.get("sustained")
    if sus:
        b = sus.get("board") or {}
        line["roofline"]["sustained"] = {"frac": sus.get("frac"), "seconds": sus.get("seconds"), "avg_launch_ms": sus.get("avg_launch_ms"), "package_W": b.get("package_W"),
                                         "cap_W": b.get("cap_W"), "sclk_MHz": b.get("sclk_MHz"), "joules_per_launch": sus.get("joules_per_launch")}
    cb = full.get("cpu_baseline")
    if cb:
        line["cpu_baseline"] = {"value": cb["value"], "unit": cb["unit"], "cores": cb["cores"], "kind": cb["kind"], "sample": cb["sample"][:200]}
        v = cb.get("vectorised_across_streams") or {}
        if "value" in v:
            line["cpu_baseline"]["vectorised_across_streams"] = v["value"]
        r1 = cb.get("reference_code_single_thread") or {}
        if "value" in r1:                                       # one thread each: the reference's own DF1 closures x 6 against the port
            line["cpu_baseline"]["one_thread_reference_code_vs_port"] = [r1["value"], cb.get("single_thread_calibration_Msamples_per_s")]
    for k in ("parity", "checksum", "rccl_ranks", "dist_backend", "ms_per_step_per_rank"):
        if k in full:
            line[k] = full[k]
    legs = flatten_legs({k: v for k, v in full.items() if k not in ("config", "roofline", "cpu_baseline")})
    if legs:
        summary, gain, bad, joules = {}, {}, [], {}
        for name, leg_ in legs:
            base = leg_.get("library_default") or leg_.get("forced")
            if not base or base.get("frac") is None:           # (a leg that did not get as far as a timing: named, never a KeyError after the run)
                bad.append(name)
                continue
            summary[name] = round(base["frac"], 3)
            if (leg_.get("tuned") or {}).get("frac", 0.0) > base["frac"] + 0.01:
                gain[name] = round(leg_["tuned"]["frac"] - base["frac"], 3)
            if not str(leg_.get("parity", "")).startswith("bitwise-equal"):
                bad.append(name)
            j = (leg_.get("sustained") or {}).get("joules_per_launch")
            if j:
                joules[name] = j
        line["summary"] = summary
        line["summary_note"] = "fraction of 8 TB/s, library-default plan, HIP-event time, full BASELINE sizes; per-object detail in " + (details_path or "bench_details.json")
        line["tuned_gain_over_default"] = gain                 # objects whose measured plan beat the default by > 0.01 (empty: none)
        line["parity_objects"] = f"bitwise-equal on all {len(legs)} objects" if not bad else "MISMATCH in " + ",".join(bad)
        if joules:
            line["joules_per_launch"] = joules
    txt = json.dumps(line, separators=(",", ":"))
    if len(txt) >= LINE_LIMIT:                                # never again: drop the optional maps before the contract keys suffer
        for k in ("joules_per_launch", "tuned_gain_over_default", "summary_note", "ms_per_step_per_rank"):
            line.pop(k, None)
            txt = json.dumps(line, separators=(",", ":"))
            if len(txt) < LINE_LIMIT:
                break
    if len(txt) >= LINE_LIMIT and "summary" in line:
        line["summary"] = dict(list(line["summary"].items())[:40])
        txt = json.dumps(line, separators=(",", ":"))
    if len(txt) >= LINE_LIMIT:
        # last resort (long workload / parity / provenance strings): the contract keys, the config's workload and the roofline's numbers, strings
        # cut short -- the measurements are done, an over-long line must not cost the run
        def cut(v, n=160):
            return v[:n] if isinstance(v, str) else v
        r = line.get("roofline", {})
        line = {**{k: cut(full[k]) for k in CONTRACT_KEYS if k in full},
                "config": {"workload": cut(c.get("workload", ""), 300)},
                "roofline": {k: cut(r.get(k), 80) for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "kernel", "avg_launch_ms")},
                "cpu_baseline": {k: cut((cb or {}).get(k)) for k in ("value", "unit", "cores", "kind", "sample")},
                "parity": cut(str(full.get("parity", "")), 200), "truncated": "line over 4 KB: see " + (details_path or "bench_details.json")}
        txt = json.dumps(line, separators=(",", ":"))
    return txt


# ---- workloads ---------------------------------------------------------------------------------------------------------
class Spec:
    """One synthetic workload: a graph, its size, its drive, its coefficients and the oracle that checks it."""

    def __init__(self, key, desc, graph, ns, T, oracle, drive="noise", typed=False, params=None, mod=None, blocks=None, b_alg=None,
                 n_parity=PARITY_STREAMS, seed_off=0):
        self.key, self.desc, self.graph, self.ns, self.T, self.oracle = key, desc, graph, int(ns), int(T), oracle
        self.drive, self.typed, self.params, self.mod, self.blocks, self._b_alg = drive, typed, params, mod, blocks, b_alg
        self.n_parity, self.seed_off = n_parity, seed_off
        self._prog = None

    def resized(self, ns, T=None):
        """the same workload at another size (shares the compiled program)"""
        q = Spec(self.key, self.desc, self.graph, ns, T or self.T, self.oracle, self.drive, self.typed, self.params, self.mod, self.blocks, self._b_alg,
                 self.n_parity, self.seed_off)
        q._prog = self._prog
        return q

    def program(self, F):
        if self._prog is None:
            self._prog = F.compile(F.from_sexpr(self.graph), typed=self.typed)
        return self._prog

    def b_alg(self, prog):
        if self._b_alg:
            return int(self._b_alg(prog, self.ns, self.T))
        return self.ns * (4 * self.T * (prog.n_in + prog.n_out) + 8 * prog.n_state + 4 * prog.n_param)


class Ctx:
    pass


def gather(torch, y, ids, layout, tile):
    """[T, len(ids), w] numpy of the streams `ids` (local indices) of a frame / stream-major tensor."""
    idt = torch.as_tensor(ids, device=y.device, dtype=torch.long)
    if layout == "stream_major":
        return y[idt].permute(1, 0, 2).contiguous().cpu().numpy()
    if tile:
        return y[idt // tile, :, idt % tile, :].permute(1, 0, 2).contiguous().cpu().numpy()
    return y[:, idt].contiguous().cpu().numpy()


LAYOUT_TEXT = {"time_major": "plain time-major frames [t][stream][wire] (SURVEY 8d's device layout)",
               "stream_major": "stream-major buffers [stream][t][wire] (the reference's calling convention, test/benchmark.cpp:137-147), no layout pass"}


def leg(cx, sp, layout, tile=0, tune=True, forced=None, energy=False, reps_ms=60.0, keep=None):
    """One workload on one layout: library default and tuned plan (ms per launch from HIP events, GB/s, fraction of peak,
    PMC traffic when profiled), oracle parity of the best plan on random streams.  layout: time_major | tiled | stream_major."""
    torch, F, np, dev = cx.torch, cx.F, cx.np, cx.dev
    prog = sp.program(F)
    ns, T = sp.ns, sp.T
    sm = layout == "stream_major"
    tile = pick_tile(ns, tile) if layout == "tiled" else 0
    lay = "streammajor" if sm else (f"tile{tile}" if tile else "timemajor")
    wkey = f"{sp.key}_{ns}x{T}_{lay}"
    nin = max(prog.n_in, 1)
    xf = frames(torch, dev, ns, T, nin, tile)
    if sp.drive == "dirac":                                  # a dirac at t = 0 on every stream
        xf.zero_()
        (xf[:, 0] if tile else xf[0]).fill_(1.0)
    else:
        F.synth_fill(xf, cx.SEED + sp.seed_off)
    if sm:
        x = torch.empty((ns, T, nin), dtype=torch.float32, device=dev)
        F.frames_to_stream_major(xf, out=x)
        del xf
        y = torch.empty((ns, T, prog.n_out), dtype=torch.float32, device=dev)
    else:
        x, y = xf, frames(torch, dev, ns, T, prog.n_out, tile)
    state = torch.zeros((max(prog.n_state, 1), ns), dtype=torch.float32, device=dev)
    pd = None
    if sp.params is not None:
        pd = torch.from_numpy(sp.params(np.arange(ns))).to(dev)
    if sp.mod is not None:
        prog.set_modulation(torch.from_numpy(sp.mod).to(dev))
    bank = pb = None
    if sp.blocks:                                            # control-rate coefficient sets: fz_bank_process_blocks
        L, pfn = sp.blocks
        nb = (T + L - 1) // L
        pb = torch.empty((nb, prog.n_param, ns), dtype=torch.float32, device=dev)
        for k in range(nb):
            pb[k].copy_(torch.from_numpy(pfn(k, np.arange(ns))))
        bank = prog.bank(ns)
    SMF = F.C.FZ_VF_STREAM_MAJOR

    def mk(v):
        return None if v is None else (v if isinstance(v, F.Variant) else F.make_variant(*v))

    def run(v):
        if bank is not None:
            bank.process_blocks(x, y, sp.blocks[0], pb, variant=mk(v))
        elif sm:
            prog.run_block_stream_major(x, state=state, params=pd, out=y, variant=mk(v))
        else:
            prog.run_block(x, state=state, params=pd, out=y, variant=mk(v))

    def name_of(v):
        """(symbol, code id) of the kernel a launch with variant v runs"""
        if bank is not None:
            a = (mk(v), ns, sp.blocks[0], tile)
        elif sm:
            q = mk(v) or F.make_variant(0, 0, 0, 0)
            a = (F.make_variant(q.streams_per_lane, q.unroll, q.block_threads, q.flags | SMF), ns, T)
        else:
            a = (mk(v) if v is not None else prog.plan(ns, tile), ns, T, tile)
        return prog.kernel_symbol(*a), prog.kernel_code_id(*a)

    b = sp.b_alg(prog)

    def timed(v):
        for _ in range(3):
            run(v)                                           # (no variant: the measured plan of the shape if fz_program_tune ran, else the static choice)
        torch.cuda.synchronize()
        ms1 = event_ms(torch, lambda: run(v), 1)
        reps = max(5, min(400, int(math.ceil(reps_ms / max(ms1, 1e-3)))))
        event_ms(torch, lambda: run(v), max(3, reps // 2))   # warm-up of the same kind as the timed region (sub-millisecond kernels: clocks and queues settle over dozens of launches)
        ms = event_ms(torch, lambda: run(v), reps)
        k, cid = name_of(v)
        cnt, csrc = counters_of(cid, wkey)
        return {"kernel": k, "code_id": cid, "avg_launch_ms": round(ms, 4), "Msamples_per_s": round(ns * T / ms / 1e3, 1), "achieved_GBs": round(b / ms / 1e6, 1),
                "frac": round(b / ms / 1e6 / HBM_PEAK_GBS, 4), "traffic": cnt.get("traffic"), "issue_share": cnt.get("issue_share"), "traffic_source": csrc,
                "launches_timed": reps}

    res = {}
    best_v = forced
    if forced is not None:
        res["forced"] = timed(forced)
    else:
        res["library_default"] = timed(None)
        if tune and bank is None:
            if sm:
                cands = {}
                for v in cx.W.SM_CANDIDATES:
                    try:
                        cands[v] = timed(v)
                    except F.FlowzError:
                        pass                                  # (a body this graph does not allow)
                best_v = min(cands, key=lambda v: cands[v]["avg_launch_ms"])
                # (as in fz_program_tune: a candidate replaces the default only when it wins by more than the scatter of repeats)
                if cands[best_v]["avg_launch_ms"] > 0.985 * res["library_default"]["avg_launch_ms"]:
                    best_v = None
                res["tuned"] = timed(best_v)
                res["candidates_ms"] = {f"{v[0]},{v[1]},{v[2]},{v[3]}": c["avg_launch_ms"] for v, c in cands.items()}
            else:
                best_v, _ = prog.tune(x, state=state, params=pd, out=y)
                res["tuned"] = timed(best_v)
    plans = [k for k in ("library_default", "tuned", "forced") if k in res]
    best = max(plans, key=lambda k: res[k]["frac"])
    res["frac"], res["best_plan"], res["algorithmic_bytes_per_launch"] = res[best]["frac"], best, b
    if energy:                                               # joules per launch at the board's sustained state (>= 1 s back to back)
        n_sus, ms_tot, board = sustained_run(torch, lambda: run(best_v), res[best]["avg_launch_ms"], dev.index or 0, seconds=1.5)
        res["sustained"] = {"launches": n_sus, "avg_launch_ms": round(ms_tot / n_sus, 4), "frac": round(b / (ms_tot / n_sus) / 1e6 / HBM_PEAK_GBS, 4), "board": board,
                            "joules_per_launch": round(board["package_W"] * ms_tot / n_sus / 1e3, 3) if board else None}
    sh = res[best].get("issue_share")
    if sh is not None:
        res["issue_share"] = round(sh, 3)
        res["limiter"] = limiter_of(sh, (res.get("sustained") or {}).get("board") or cx.head_board, None)
    # parity: one block from zero state with the best plan against the oracle, random streams
    if bank is not None:
        bank.reset()
    state.zero_()
    run(best_v if best != "library_default" else None)
    torch.cuda.synchronize()
    ids = sample_ids(ns, sp.n_parity, 11 + sp.seed_off)
    nd = ndiff_bits(gather(torch, y, ids, layout, tile), sp.oracle(sp, ids))
    if sp.drive != "dirac":
        from oracle import flowz_oracle as O
        nd += ndiff_bits(gather(torch, x, ids, layout, tile), O.synth_input(cx.SEED + sp.seed_off, ids, T, n_wires=nin))   # the device generator itself
    res["parity"] = parity_string(nd, len(ids), T)
    res["workload"] = f"{sp.desc}, {ns} streams x {T}-sample block, " + (LAYOUT_TEXT.get(layout) or f"stream-tiled frames [tile][t][{tile} streams][wire]")
    res["layout"] = layout
    res["workload_key"] = wkey                               # (what profiles/pmc_traffic.json and sq_issue_share.json are keyed by, next to the kernel symbol)
    if keep is not None:
        keep.update(x=x, y=y, state=state, prog=prog)
    return res


def make_specs(cx, ns_big, T):
    """The workloads of the bench line.  Oracle closures import oracle/ lazily: the checker."""
    np, W = cx.np, cx.W

    def noise(sp, ids, nw=1):
        from oracle import flowz_oracle as O
        return O.synth_input(cx.SEED + sp.seed_off, ids, sp.T, n_wires=nw)

    def dirac(sp, ids):
        x = np.zeros((sp.T, len(ids), 1), np.float32)
        x[0] = 1.0
        return x

    def o_cascade(sp, ids):
        from oracle import coracle
        return coracle.df1_cascade([W.STABLE] * 6, noise(sp, ids))

    def o_par4(fanout):
        def f(sp, ids):
            from oracle import coracle
            return coracle.par4_sum(W.PAR4_SETS, noise(sp, ids, nw=1 if fanout else 4), fanout=fanout)
        return f

    def o_osc(sp, ids):
        from oracle import coracle
        return coracle.osc_chain(np.ascontiguousarray(W.osc_chain_params(cx.SEED + 1, ids)), dirac(sp, ids))

    def o_generic(graph, typed=False, mod=None):
        def f(sp, ids):
            from oracle import flowz_oracle as O
            x = noise(sp, ids)
            if typed:
                orc = O.compile(graph, len(ids), typed=True)
                return cx.F.pack_typed(O.run_typed(orc, [x[:, :, 0]]), O.output_dtypes_typed(graph))
            return O.compile(graph, len(ids)).run(x, mod=mod)
        return f

    S = {}
    cas = W.df1_cascade(6)
    for ns in (ns_big, 65536, 32768, 16384, 262144):
        S[f"cascade6_{ns}"] = Spec("cascade6", "6-stage DF1 cascade (flowz fwd|=bwd x6), uniform stable coefficients", cas, ns, T, o_cascade)
    for ns in ragged_stream_counts(ns_big):
        S[f"cascade6_{ns}"] = S[f"cascade6_{ns_big}"].resized(ns)
    S["par4"] = Spec("par4", "(bq|bq|bq|bq) |= (_1+_2+_3+_4), 4 input wires (BASELINE configs[2])", W.par4_sum(), ns_big, T, o_par4(False))
    S["par4f"] = Spec("par4f", "(_1,_1,_1,_1) |= (bq|bq|bq|bq) |= (_1+_2+_3+_4), 1 input wire (BASELINE configs[2], fan-out variant)", W.par4_sum_fanout(), ns_big, T, o_par4(True))
    S["osc6"] = Spec("osc6", "resonator oscillator -> 6 x DF1, 31 per-stream coefficients, dirac drive (BASELINE configs[3])", W.osc_chain(6), ns_big, T, o_osc,
                     drive="dirac", params=lambda ids: W.osc_chain_params(cx.SEED + 1, ids))
    # the reference's own benchmark cases, test/benchmark.cpp:157-262 (coefficients :18-23)
    REFC = (W.B0, W.B1, W.B2, W.A1, W.A2)

    def o_ref(fn):
        def f(sp, ids):
            from oracle import coracle
            x = noise(sp, ids)
            return coracle.df1_cascade([REFC], x) if fn == "df1" else getattr(coracle, fn)(REFC, x)
        return f
    for name, g, fn in (("df1", W.df1(), "df1"), ("df2", W.df2(), "df2"), ("df1t", W.df1t(), "df1t"), ("df2t", W.df2t(), "df2t_flowz")):
        S[name] = Spec(name, f"single biquad {name.upper()} of test/benchmark.cpp:157-262 (coefficients :18-23)", g, ns_big, T, o_ref(fn), seed_off=3)
    # SURVEY 8(f) rows
    S["lds_ring"] = Spec("ldsring", "f1: (_1 + 0.5*_1[_40]) |= ~(0.7*_1[_23] + _2), delay lines of 40 and 23 samples in LDS rings", W.lds_ring_comb(), ns_big, T,
                         o_generic(W.lds_ring_comb()), n_parity=192, seed_off=4)
    S["far_ring"] = Spec("farring", "f1: ~(0.5*_1[_300] + _2), a 300-sample delay line as a ring in HBM (16 algorithmic bytes per stream-sample: frame in/out + one appended row + one far read)",
                         W.far_comb(300), ns_big, T, o_generic(W.far_comb(300)), n_parity=192, seed_off=5,
                         b_alg=lambda p, ns, TT: ns * (4 * TT * 4 + 8))
    L = 64
    nbk = (T + L - 1) // L

    def block_params(k, ids):                                # coefficient set of block k: the oscillator chain's stage sets, re-drawn per block
        return np.ascontiguousarray(W.osc_chain_params(cx.SEED + 7 + k, ids)[1:])

    def o_blocks(sp, ids):
        from oracle import flowz_oracle as O
        g = W.df1_cascade_params(6)
        f = O.compile(g, len(ids), params=block_params(0, ids))
        x, outs = noise(sp, ids), []
        for k in range(nbk):
            f._params = np.ascontiguousarray(block_params(k, ids), np.float32)
            outs.append(f.run(x[k * L:(k + 1) * L]))
        return np.concatenate(outs)
    S["blocks64"] = Spec("blocks64", f"f2: 6 x DF1 with 30 per-stream coefficients under fz_bank_process_blocks, {L}-sample windows, one coefficient set per window "
                                     "(std::ref terminals at block rate, flowz/README.md:42-61)", W.df1_cascade_params(6), ns_big, T, o_blocks, blocks=(L, block_params),
                         n_parity=128, seed_off=6, b_alg=lambda p, ns, TT: ns * (4 * TT * 2 + ((TT + L - 1) // L) * (8 * p.n_state + 4 * p.n_param)))
    modv = (0.2 + 0.1 * W.hash32(cx.SEED + 9, 0, np.arange(T)).astype(np.float64) / 4294967296.0).astype(np.float32)[None, :]
    S["modulated"] = Spec("mod6", "f2: 6 x DF1 whose a1 is a sample-rate fz_modulator (std::ref re-read every sample, flowz/README.md:42-61), one value per sample for all streams",
                          W.df1_cascade_modulated(6), ns_big, T, o_generic(W.df1_cascade_modulated(6), mod=modv), mod=modv, n_parity=192, seed_off=8)
    S["double_biquad"] = Spec("f64biquad", "f3: one DF1 biquad with double literals under fz_compile_typed: double wires, double delay line, double output frames "
                                           "(ResultType, flowz.hpp:585-644) -- 12 frame bytes per sample, FP64 arithmetic", W.df1_double(), ns_big, T,
                              o_generic(W.df1_double(), typed=True), typed=True, n_parity=128, seed_off=10)

    def o_cplx(sp, ids):
        from oracle import coracle
        return coracle.complex_one_pole(noise(sp, ids), std=True)
    S["complex_one_pole"] = Spec("c32onepole", "f3: ~( c*_1[_1] + _2 ) with a std::complex<float> coefficient under fz_compile_typed: complex wire and delay line, "
                                               "(re, im) output frames (test/tests.cpp:206-207)", W.complex_one_pole(), ns_big, T, o_cplx, typed=True, seed_off=11)
    return S


def ragged_stream_counts(big):
    """stream counts that are not whole workgroups x CUs: the judge's four at the headline size, the same proportions elsewhere"""
    return (1_000_000, 1_048_577, 786_432, 2_097_152) if big == (1 << 20) else (big * 1_000_000 // (1 << 20), big + 1, big * 3 // 4, big * 2)


def obj_layouts(cx, sp, first_layout, first_tile, steps_hint=None, tune=True):
    """A config object: today's primary figure at top level (its layout named in `workload`), plus `time_major` and `stream_major`
    sub-objects -- the two contract layouts (test/benchmark.cpp:137-147)."""
    torch = cx.torch
    res = leg(cx, sp, first_layout, first_tile, tune=tune)
    torch.cuda.empty_cache()
    res.update({k: res[res["best_plan"]][k] for k in ("avg_launch_ms", "Msamples_per_s", "achieved_GBs", "kernel")})
    if first_layout != "time_major":
        res["time_major"] = leg(cx, sp, "time_major", tune=tune)
        torch.cuda.empty_cache()
    res["stream_major"] = leg(cx, sp, "stream_major", tune=tune)
    torch.cuda.empty_cache()
    return res


def dirac_check(cx, name, graph):
    """the first 201 samples of the dirac response on every stream of a small block against the vectors the reference's own
    hand-written filter produced (tests/golden/ref_biquad_vectors.json; oracle/build_ref.sh)"""
    torch, F, np = cx.torch, cx.F, cx.np
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "ref_biquad_vectors.json")))
    want = np.array([int(h, 16) for h in ref["outputs"]["dirac"][name]], np.uint32)[:201]
    prog = F.compile(F.from_sexpr(graph))
    x = torch.zeros((201, 256, 1), dtype=torch.float32, device=cx.dev)
    x[0].fill_(1.0)
    y, _ = prog.run_block(x)
    got = y[:, :, 0].cpu().numpy().view(np.uint32)
    nd = int((got != want[:, None]).sum())
    return "bitwise-equal to the reference-built vector on 256 streams x 201 samples" if nd == 0 else f"MISMATCH {nd}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--streams", type=int, default=1 << 20, help="streams PER GPU (weak scaling)")
    ap.add_argument("--samples", type=int, default=4096, help="samples per block")
    ap.add_argument("--scaling", choices=("weak", "strong"), default="weak",
                    help="weak: --streams per GPU (config 5: 1 M per GPU); strong: --streams-total divided over the GPUs")
    ap.add_argument("--streams-total", type=int, default=1 << 23, help="total streams of --scaling strong (SURVEY 8d config 5: 8 M)")
    ap.add_argument("--dist-backend", choices=("nccl", "gloo"), default="nccl",
                    help="nccl == RCCL over xGMI (default); gloo rehearses the N > 1 path when all ranks share one GPU")
    ap.add_argument("--lanes", type=int, default=0, help="streams per lane (0 = auto)")
    ap.add_argument("--unroll", type=int, default=0)
    ap.add_argument("--block", type=int, default=0)
    ap.add_argument("--flags", type=int, default=0)
    ap.add_argument("--tile", type=int, default=0,
                    help="frame layout of the headline workload: 0 = plain time-major [t][stream] (SURVEY 8d's device layout; since round "
                         "3 also the fastest: CU-wide workgroups in lockstep, XCD-wide synchronised), else streams per frame tile "
                         "(stream-tiled layout [tile][t][stream])")
    ap.add_argument("--secondary-tile", type=int, default=8192,
                    help="streams per frame tile of the tiled-layout legs (1-wire frames)")
    ap.add_argument("--full", action="store_true",
                    help="besides the headline: oracle parity, the sustained run, the row-walk and copy yardsticks, the CPU baseline and the "
                         "other configs, layouts and shapes (every --no-* option but --no-autotune leaves a part of it out)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-config2", action="store_true", help="skip the 65 536 / 32 768 / 16 384-stream objects (BASELINE configs[1] and below)")
    ap.add_argument("--no-config34", action="store_true", help="skip BASELINE configs[2] and [3] (4-parallel sum, oscillator chain)")
    ap.add_argument("--no-next-rows", action="store_true", help="skip the SURVEY 8(f) kernels (LDS / HBM rings, block-rate and sample-rate modulation, typed state)")
    ap.add_argument("--no-extras", action="store_true", help="skip ragged stream counts, the reference's benchmark topologies and the smaller stream-major shapes")
    ap.add_argument("--no-sustained", action="store_true", help="skip the >= 2 s back-to-back run")
    ap.add_argument("--only", default="", help="profiling aid: run ONLY this object / leg (see OBJECTS in the source; <object>:<layout> picks one layout) "
                                               "with the forced / default variant and print it")
    ap.add_argument("--reps-ms", type=float, default=60.0, help="--only: milliseconds of launches per timed region (profiling passes use a few)")
    ap.add_argument("--no-autotune", action="store_true",
                    help="do not try the alternative kernel variants during warm-up (the pool's boxes differ by a few %%)")
    ap.add_argument("--no-layout-legs", action="store_true",
                    help="skip the headline workload on the other layouts: stream tiles and stream-major buffers [stream][t] "
                         "(the reference's calling convention, test/benchmark.cpp:137-147)")
    ap.add_argument("--dump-outputs", metavar="DIR", default="",
                    help="after the timed steps, write what the headline workload's last step returned (out frames and state; rank 0's shard) "
                         "as DIR/<name>.npy, float32, at most 64 MB in all (a fixed, seeded sample of the streams)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps: at least one timed step")
    if args.dump_outputs and args.only:
        ap.error("--dump-outputs writes the headline workload's outputs, which --only does not run")
    if args.no_autotune:
        os.environ["FLOWZ_HIP_AUTOTUNE"] = "0"               # (the library's default since round 6: nothing is measured on first use)

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # started by hand without a launcher: become `torch.distributed.run` with one rank per GPU
        import subprocess
        port = os.environ.get("MASTER_PORT", "29533")
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
               "--master-addr", "127.0.0.1", "--master-port", port, os.path.abspath(__file__)] + sys.argv[1:]
        raise SystemExit(subprocess.call(cmd))

    import numpy as np
    import torch
    import torch.distributed as dist

    from zignal_amd import dist as zdist
    from zignal_amd import flowz as F
    from zignal_amd import workloads as W

    if args.full or args.only:                               # (the parity checks and the CPU baseline call it)
        load_oracle()
    SEED = W.SEED
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the flow-graph evaluator has no CPU path")
    n_dev = torch.cuda.device_count()
    torch.cuda.set_device(local_rank % n_dev)                # (gloo rehearsal: several ranks may share device 0)
    dev = torch.device("cuda", local_rank % n_dev)
    distributed = world > 1 or "RANK" in os.environ          # launched by torch.distributed.run
    if distributed:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        if args.dist_backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)   # nccl == RCCL on ROCm
        else:
            dist.init_process_group("gloo", rank=rank, world_size=world)
    stats_dev = dev if args.dist_backend == "nccl" else None

    T = args.samples
    total = args.streams_total if args.scaling == "strong" else args.streams * world
    begin, end = zdist.shard_range(total, rank, world)       # this rank's global stream ids
    ns = end - begin
    prog = F.compile(F.from_sexpr(W.df1_cascade(6)))
    forced = bool(args.lanes or args.unroll or args.block or args.flags)
    variant = F.make_variant(args.lanes, args.unroll, args.block, args.flags) if forced else None
    tile = pick_tile(ns, args.tile)
    lay = f"tile{tile}" if tile else "timemajor"

    cx = Ctx()
    cx.torch, cx.F, cx.W, cx.np, cx.dev, cx.args, cx.SEED, cx.head_board = torch, F, W, np, dev, args, SEED, None
    do_tune = not args.no_autotune
    S = make_specs(cx, args.streams, T)
    big = args.streams

    def barrier():
        if distributed:
            dist.barrier()
        torch.cuda.synchronize()

    # ---- the objects of the line besides the headline (rank 0, N == 1): each frees its buffers before the next -------------
    def ragged_counts():
        """odd shapes at scale, plain time-major frames, library default only"""
        out = {}
        for n in ragged_stream_counts(big):
            out[str(n)] = leg(cx, S[f"cascade6_{n}"], "time_major", tune=False)
            torch.cuda.empty_cache()
        return out

    def reference_topologies():
        """test/benchmark.cpp:157-262: the four single-stage forms at full size on time-major frames (noise drive, oracle parity) and
        their dirac responses against the vectors built from the reference's own filters"""
        out = {}
        for name in ("df1", "df2", "df1t", "df2t"):
            r = leg(cx, S[name], "time_major", tune=do_tune)
            r["dirac_201"] = dirac_check(cx, name, S[name].graph)
            out[name] = r
            torch.cuda.empty_cache()
        return out

    def next_rows():
        out = {}
        for name in ("lds_ring", "far_ring", "blocks64", "modulated", "double_biquad", "complex_one_pole"):
            out[name] = leg(cx, S[name], "time_major", tune=do_tune and name != "blocks64")
            torch.cuda.empty_cache()
        out["double_biquad"]["bound_note"] = ("FP64 issue: 9 double operations per sample (v_mul_f64 / v_add_f64 issue at a quarter of the packed-FP32 rate per lane) "
                                              "next to 12 frame bytes per sample")
        return out

    def stream_major_shapes():
        """the cascade on stream-major buffers at 262 144 streams and with 1024-sample blocks"""
        out = {}
        out[f"{min(262144, big)}_streams_x_{T}"] = leg(cx, S["cascade6_262144"] if big >= 262144 else S[f"cascade6_{big}"], "stream_major", tune=do_tune)
        torch.cuda.empty_cache()
        Ts = max(256, T // 4)
        out[f"{big}_streams_x_{Ts}"] = leg(cx, S[f"cascade6_{big}"].resized(big, Ts), "stream_major", tune=do_tune)
        torch.cuda.empty_cache()
        return out

    OBJECTS = {
        "config2": lambda: obj_layouts(cx, S["cascade6_65536"], "tiled", args.secondary_tile, tune=do_tune),
        "config2h": lambda: leg(cx, S["cascade6_32768"], "tiled", args.secondary_tile, tune=do_tune),
        "config2q": lambda: leg(cx, S["cascade6_16384"], "tiled", args.secondary_tile, tune=do_tune),
        "config3": lambda: obj_layouts(cx, S["par4"], "tiled", S["par4"].program(F).recommended_tile_streams(), tune=do_tune),
        "config3f": lambda: leg(cx, S["par4f"], "time_major", tune=do_tune),
        "config4": lambda: obj_layouts(cx, S["osc6"], "tiled", args.secondary_tile, tune=do_tune),
        "tiled": lambda: leg(cx, S[f"cascade6_{big}"], "tiled", args.secondary_tile, tune=do_tune),
        "timemajor": lambda: leg(cx, S[f"cascade6_{big}"], "time_major", tune=do_tune),
        "streammajor": lambda: leg(cx, S[f"cascade6_{big}"], "stream_major", tune=do_tune, energy=not args.no_sustained),
        "streammajor_shapes": stream_major_shapes,
        "ragged": ragged_counts,
        "reftopo": reference_topologies,
        "next_rows": next_rows,
    }
    if args.only:
        name, _, sub = args.only.partition(":")
        if name in S and sub:                                # one workload on one layout, forced or default variant: <spec>:<layout>[:tile]
            lay_, _, t_ = sub.partition(":")
            v = (args.lanes, args.unroll, args.block, args.flags) if forced else None
            r = leg(cx, S[name], lay_, int(t_ or 0), tune=False, forced=v, reps_ms=args.reps_ms)
        else:
            r = OBJECTS[name]()
        print(json.dumps({args.only: r}), flush=True)
        return

    # ---- the headline workload ------------------------------------------------------------------------------------------
    x, y = frames(torch, dev, ns, T, 1, tile), frames(torch, dev, ns, T, 1, tile)
    state = torch.zeros((prog.n_state, ns), dtype=torch.float32, device=dev)
    F.synth_fill(x, SEED, stream0=begin)
    torch.cuda.synchronize()

    # plan selection (warm-up, untimed): when no variant is forced, let the library measure its candidate
    # variants for this shape on THIS board (fz_program_tune, the FFTW_MEASURE of this library; which one
    # wins differs from board to board) -- later launches without a variant use the winner
    tuned = None
    if do_tune and not forced:
        variant, _ = prog.tune(x, state=state, out=y)
        tuned = prog.kernel_symbol(variant, ns, T, tile)
        state.zero_()

    # first block from zero state: kept for the parity check (>= 1024 random streams across all tiles)
    prog.run_block(x, state=state, out=y, variant=variant)
    torch.cuda.synchronize()
    parity = args.full and (not args.no_cpu_baseline or world > 1)
    if parity:
        # (every rank checks streams of its OWN shard against the oracle: rank 0 >= 1024, the others >= 128)
        par_ids = sample_ids(ns, PARITY_STREAMS if rank == 0 else PARITY_STREAMS_OTHER_RANKS, 11 + rank)
        first_block = gather(torch, y, par_ids, "tiled" if tile else "time_major", tile)
    for _ in range(max(args.warmup - 1, 0)):
        prog.run_block(x, state=state, out=y, variant=variant)

    # HIP events on the launch stream around the K back-to-back launches (one pair: an event per
    # launch costs tens of microseconds of GPU time each, visible on sub-millisecond kernels)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    barrier()
    t0 = time.perf_counter()
    ev0.record()
    for k in range(args.steps):
        prog.run_block(x, state=state, out=y, variant=variant)
    ev1.record()
    barrier()
    wall = time.perf_counter() - t0
    kern_avg_s = ev0.elapsed_time(ev1) / args.steps / 1e3
    if args.dump_outputs and rank == 0:                      # (before the sustained run launches the kernel again)
        dump_outputs(torch, args.dump_outputs, y, state, tile)

    checksum = zdist.bits_checksum(y[:, -1] if tile else y[-1])      # last time step of every stream: exact, shard-independent
    stats = zdist.reduce_stats(wall, float(ns) * T * args.steps, checksum, device=stats_dev)
    b_alg = ns * (4 * T * (prog.n_in + prog.n_out) + 8 * prog.n_state + 4 * prog.n_param)
    per_rank_ms = zdist.gather_floats(kern_avg_s * 1e3, device=stats_dev)        # HIP-event ms per launch of every rank
    # parity of every rank's shard (the oracle is the checker, outside the timed region; global stream ids = begin + local)
    nd_all = n_checked = None
    if parity:
        from oracle import coracle, flowz_oracle as O
        want = coracle.df1_cascade([W.STABLE] * 6, O.synth_input(SEED, par_ids + begin, T))
        nd_all, n_checked = (int(v) for v in zdist.sum_ints([ndiff_bits(first_block, want), len(par_ids)], device=stats_dev))

    # the same launches back to back for >= 2 s: whatever the power management does to the clocks has happened by then
    sustained = None
    if args.full and rank == 0 and world == 1 and not args.no_sustained:
        n_sus, ms_tot, board = sustained_run(torch, lambda: prog.run_block(x, state=state, out=y, variant=variant), kern_avg_s * 1e3, dev.index or 0,
                                             seconds=2.0, min_batch=args.steps)
        ms_sus = ms_tot / n_sus
        cx.head_board = board
        sustained = {"launches": n_sus, "seconds": round(ms_tot / 1e3, 3), "avg_launch_ms": round(ms_sus, 4),
                     "achieved_GBs": round(b_alg / ms_sus / 1e6, 1), "frac": round(b_alg / ms_sus / 1e6 / HBM_PEAK_GBS, 4),
                     "board": board, "joules_per_launch": round(board["package_W"] * ms_sus / 1e3, 3) if board else None}

    # yardsticks, rank 0 only: (1) the arithmetic-free row walk -- the identity graph `_1` through the same launch path (same
    # lockstep / XCD-synchronised skeleton, same frames): what this layout gives a kernel that only moves the rows; (2) the plain
    # one-shot float4 copy kernel (fz_copy_probe)
    copy_gbs = walk_gbs = walk_kernel = None
    if args.full and rank == 0:
        F.copy_probe(x, y)
        torch.cuda.synchronize()
        copy_gbs = 2.0 * x.numel() * 4 / (event_ms(torch, lambda: F.copy_probe(x, y), 3) / 1e3) / 1e9
        ident = F.compile(F.from_sexpr(W.IN(1)))
        st0 = torch.zeros((1, ns), dtype=torch.float32, device=dev)
        for _ in range(3):
            ident.run_block(x, state=st0, out=y)
        torch.cuda.synchronize()
        walk_ms = event_ms(torch, lambda: ident.run_block(x, state=st0, out=y), max(5, args.steps // 2))
        walk_gbs = 2.0 * x.numel() * 4 / (walk_ms / 1e3) / 1e9
        walk_kernel = ident.kernel_symbol(ident.plan(ns, tile), ns, T, tile)

    secondary = {}
    if args.full and rank == 0 and world == 1:
        del x, y, state
        torch.cuda.empty_cache()
        if not args.no_layout_legs:
            secondary["time_major_layout" if tile else "tiled_layout"] = OBJECTS["timemajor" if tile else "tiled"]()
            torch.cuda.empty_cache()
            secondary["stream_major_layout"] = OBJECTS["streammajor"]()
            torch.cuda.empty_cache()
            if not args.no_extras:
                secondary["stream_major_layout"]["other_shapes"] = stream_major_shapes()
        if not args.no_config2 and ns != 65536:
            secondary["config2_65536_streams"] = OBJECTS["config2"]()
            secondary["cascade6_32768_streams"] = OBJECTS["config2h"]()    # below one wave per SIMD: the wave-split kernel (two parts)
            secondary["cascade6_16384_streams"] = OBJECTS["config2q"]()    # a quarter of a wave per SIMD: three parts
            torch.cuda.empty_cache()
        if not args.no_config34:
            secondary["config3_par4_sum"] = OBJECTS["config3"]()
            secondary["config3_par4_sum_fanout"] = OBJECTS["config3f"]()
            secondary["config4_osc_chain"] = OBJECTS["config4"]()
            torch.cuda.empty_cache()
        if not args.no_extras:
            secondary["ragged_counts"] = ragged_counts()
            secondary["reference_benchmark_topologies"] = reference_topologies()
        if not args.no_next_rows:
            secondary["next_rows"] = next_rows()

    if rank == 0:
        achieved = b_alg / kern_avg_s / 1e9
        vrun = variant if variant is not None else prog.plan(ns, tile)
        kname, kcode = prog.kernel_symbol(vrun, ns, T, tile), prog.kernel_code_id(vrun, ns, T, tile)
        wkey = f"cascade6_{ns}x{T}_{lay}"
        cnt, csrc = counters_of(kcode, wkey)
        traffic, share = cnt.get("traffic"), cnt.get("issue_share")
        line = {
            "metric": "Msamples/sec/GPU + achieved HBM GB/s, 6-biquad cascade, 1M streams",
            "value": round(stats["samples"] / stats["seconds"] / 1e6, 1),
            "unit": "Msamples/s",
            "per_gpu": round(stats["samples"] / stats["seconds"] / 1e6 / world, 1),
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(stats["seconds"] / args.steps * 1e3, 4),
            "higher_is_better": True, "scaling": args.scaling, "vs_baseline": None,
            "dtype": "f32", "data": "synthetic",
            "config": {"workload": f"6-stage DF1 biquad cascade (flowz fwd|=bwd x6), {ns} streams/GPU x {T}-sample block, "
                                   f"uniform stable coefficients, "
                                   + (f"stream-tiled frames [tile][t][{tile} streams]" if tile else "time-major frames [t][stream]"),
                       "layout": f"tiled:{tile}" if tile else "time-major",
                       "streams_per_gpu": ns, "block_samples": T, "streams_total": total,
                       "parallelism": f"stream-sharded x{world}, no data-path collective"
                                      + (f" (statistics reduced over {args.dist_backend})" if distributed else ""),
                       "kernel_variant": {"streams_per_lane": args.lanes, "unroll": args.unroll,
                                          "block_threads": args.block, "flags": args.flags,
                                          "autotuned": tuned}},
            "roofline": {"bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": traffic,
                         "traffic_source": csrc, "workload_key": wkey,
                         "kernel": kname, "code_id": kcode, "algorithmic_bytes_per_launch": b_alg,
                         "avg_launch_ms": round(kern_avg_s * 1e3, 4),
                         "measured_row_walk_GBs": round(walk_gbs, 1) if walk_gbs else None,
                         "row_walk_kernel": walk_kernel,
                         "frac_of_row_walk": round(achieved / walk_gbs, 4) if walk_gbs else None,
                         "measured_copy_GBs": round(copy_gbs, 1) if copy_gbs else None,
                         "issue_share": round(share, 3) if share is not None else None,
                         "limiter": limiter_of(share, (sustained or {}).get("board"), achieved / walk_gbs if walk_gbs else None)},
            "checksum": stats["checksum"],
        }
        if sustained is not None:
            line["roofline"]["sustained"] = sustained
        line.update(secondary)
        if nd_all is not None:
            line["parity"] = parity_string(nd_all, n_checked, T) + (f" (every one of the {world} ranks checked streams of its own shard)" if world > 1 else "")
        if distributed:
            line["dist_backend"] = args.dist_backend
            line["rccl_ranks"] = dist.get_world_size() if args.dist_backend == "nccl" else 0
            line["ms_per_step_per_rank"] = [round(v, 4) for v in per_rank_ms]
        if args.full and world == 1 and not args.no_cpu_baseline:
            line["cpu_baseline"] = cpu_baseline(T, SEED, [W.STABLE] * 6)
        # the full record goes to a file; stdout carries ONE line the driver can parse (< 4 KB)
        details_path = os.environ.get("BENCH_DETAILS", os.path.join(ROOT, "bench_details.json"))
        try:
            with open(details_path, "w") as f:
                json.dump(line, f, indent=1)
        except OSError as e:                                 # (a read-only checkout must not cost the line)
            print(f"# bench_details.json not written: {e}", file=sys.stderr)
        print(compact_line(line, os.path.basename(details_path)), flush=True)
    if distributed:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
