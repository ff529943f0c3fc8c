"""Whole-output checks: a device result against a compiled-oracle closure (oracle/coracle.py) on every stream and every sample, bit for bit
(NaNs of any payload equal, as ndiff_nan_aware counts them).

The stream range is cut into slices of a few thousand streams.  For each slice a worker thread generates the slice's input on the host,
runs the C closure on it (ctypes releases the GIL) and compares the result with the same streams of every leg: a leg is one device output
(time-major rows, stream tiles or stream-major buffers) of the workload, so the legs of one seed and stream range share one oracle pass.
Only threads: a child process of a process that has opened the GPU would count against the GPU's process limit.  Host memory stays
at a few slices per thread whatever the workload's size.

A mismatch report names the leg, its kernel, the number of mismatching streams and the first mismatching (stream, sample), and says
whether the device input of that slice equals the host-generated one (the generator or the kernel).  The input is only compared on a
mismatch, so the common path moves nothing but the outputs across PCIe."""
from __future__ import annotations

import os
import threading
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass
from typing import Callable, Optional

import numpy as np

F32 = np.float32
SLICE_BYTES = 32 << 20              # host bytes of one slice of the widest frame (input or output) a worker holds at a time


def n_threads() -> int:
    """min(16, the CPUs this process may run on, OMP_NUM_THREADS when set)"""
    n = min(16, len(os.sched_getaffinity(0)))
    omp = os.environ.get("OMP_NUM_THREADS", "")
    if omp.strip().isdigit() and int(omp) > 0:
        n = min(n, int(omp))
    return max(1, n)


def slice_streams(T: int, width: int, tile: int = 0) -> int:
    """streams per slice: SLICE_BYTES of [k, T, width] float32, a divisor of the tile (slices never straddle one) when tiles are given"""
    k = max(1, SLICE_BYTES // (4 * T * max(1, width)))
    if tile:
        k = min(k, tile)
        while tile % k:
            k -= 1
    return k


# ---- where a leg's slice comes from: stream-major [k, T, w] float32 host arrays of streams [s0, s1) ----------------------------------
_pinned = threading.local()


def _to_host(t):
    """a device (torch) or host (numpy) [k, T, w] array -> a contiguous numpy array (device slices go through a per-thread pinned buffer)"""
    if isinstance(t, np.ndarray):
        return np.ascontiguousarray(t)
    import torch
    t = t.contiguous()
    if not t.is_cuda:
        return t.numpy()
    bufs = getattr(_pinned, "bufs", None)
    if bufs is None:
        bufs = _pinned.bufs = {}
    buf = bufs.get(tuple(t.shape))
    if buf is None:
        bufs.clear()                                         # (one staging buffer per thread)
        buf = bufs[tuple(t.shape)] = torch.empty(tuple(t.shape), dtype=t.dtype, pin_memory=True)
    buf.copy_(t)
    return buf.numpy()                                       # (valid until this thread's next fetch: compared before that)


def rows(y):
    """time-major frames [T, n_streams, w]: the slice is made stream-major on the device first"""
    def fetch(s0, s1):
        sl = y[:, s0:s1]
        return _to_host(sl.transpose(1, 0, 2) if isinstance(sl, np.ndarray) else sl.permute(1, 0, 2))
    return fetch


def tiles(y):
    """stream-tiled frames [n_tiles, T, tile, w]: the [T, streams] block of each tile the slice touches"""
    tile = y.shape[2]

    def fetch(s0, s1):
        out = np.empty((s1 - s0, y.shape[1], y.shape[3]), F32)
        s = s0
        while s < s1:
            t, a = divmod(s, tile)
            b = min(tile, a + s1 - s)
            blk = y[t, :, a:b]
            out[s - s0:s - s0 + b - a] = _to_host(blk.transpose(1, 0, 2) if isinstance(blk, np.ndarray) else blk.permute(1, 0, 2))
            s += b - a
        return out
    return fetch


def stream_major(y):
    """stream-major buffers [n_streams, T, w]: the slice as it lies"""
    return lambda s0, s1: _to_host(y[s0:s1])


@dataclass
class Leg:
    """one device output of a group: fetch(s0, s1) -> its streams [s0, s1) as stream-major [k, T, w] host floats;
    fetch_input(s0, s1) -> the device input of those streams, stream-major (called on a mismatch only)"""
    name: str
    kernel: str
    fetch: Callable[[int, int], np.ndarray]
    fetch_input: Optional[Callable[[int, int], np.ndarray]] = None


@dataclass
class LegResult:
    leg: Leg
    bad_streams: int = 0
    first: Optional[tuple] = None                          # (stream, sample, slot) of the first mismatch
    input_equal: Optional[bool] = None                     # of the slice holding `first`: device input == host input
    checked_streams: int = 0

    def report(self) -> str:
        if not self.bad_streams:
            return f"{self.leg.name} [{self.leg.kernel}]: {self.checked_streams} streams equal"
        s, t, w = self.first
        inp = {None: "not compared", True: "equal", False: "DIFFERENT"}[self.input_equal]
        return (f"{self.leg.name} [{self.leg.kernel}]: {self.bad_streams} of {self.checked_streams} streams differ, the first at "
                f"stream {s} sample {t} slot {w}; the device input of that slice is {inp} to the host-generated one")


@dataclass
class Report:
    legs: list
    n_streams: int
    n_threads: int
    slice_streams: int

    @property
    def ok(self) -> bool:
        return all(r.bad_streams == 0 and r.checked_streams == self.n_streams for r in self.legs)

    def __str__(self):
        return "\n".join(r.report() for r in self.legs)


def mismatch(got, want):
    """[k, T, w] bool: differing bit patterns, NaNs of any payload equal"""
    got = np.ascontiguousarray(got, F32)
    want = np.ascontiguousarray(want, F32)
    assert got.shape == want.shape, (got.shape, want.shape)
    m = got.view(np.uint32) != want.view(np.uint32)
    if m.any():
        m &= ~(np.isnan(got) & np.isnan(want))
    return m


def _first(m, s0):
    """(bad stream count, (stream, sample, slot) of the first mismatch) of one slice's mismatch mask"""
    per = m.reshape(m.shape[0], -1).any(axis=1)
    n = int(per.sum())
    if not n:
        return 0, None
    i = int(np.argmax(per))
    t, w = np.unravel_index(int(np.argmax(m[i].ravel())), m[i].shape)
    return n, (s0 + i, int(t), int(w))


def check(legs, reference, n_streams: int, k: int, threads: Optional[int] = None) -> Report:
    """Compare every leg with the oracle on streams [0, n_streams), k streams per slice.
    reference(s0, s1) -> (x, want): the host input of the slice and the oracle's output, stream-major [k, T, w] float32."""
    threads = threads or n_threads()
    results = [LegResult(lg) for lg in legs]
    lock = threading.Lock()

    def job(s0):
        s1 = min(n_streams, s0 + k)
        x, want = reference(s0, s1)
        for r in results:
            n, first = _first(mismatch(r.leg.fetch(s0, s1), want), s0)
            ieq = None
            if n and r.leg.fetch_input is not None:
                ieq = not mismatch(r.leg.fetch_input(s0, s1), x).any()
            with lock:
                r.checked_streams += s1 - s0
                if n:
                    r.bad_streams += n
                    if r.first is None or first < r.first:
                        r.first, r.input_equal = first, ieq

    with ThreadPoolExecutor(max_workers=threads) as ex:
        for f in [ex.submit(job, s0) for s0 in range(0, n_streams, k)]:
            f.result()
    return Report(results, n_streams, threads, k)
