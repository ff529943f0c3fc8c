#!/usr/bin/env python3
"""Exhaustive check of the float graph functions exp and tanh over all 2^32 float inputs (no GPU: the numpy restatement of
tests/fn_ref.py, which the GPU tests hold the kernels to bit for bit).

Prints, per function: the largest error in ulps of the correctly rounded result (float64 reference, whose own error is far below a float
ulp), NaN agreement, and how monotone the result is over the inputs in increasing order: the number of places where the result steps
down, and the largest such step in ulps.  tanh is also checked for oddness (tanh(-x) = -tanh(x) bitwise) and |tanh| <= 1.
The numbers are the ones include/flowz_hip.h states.

usage: tools/graph_functions_exhaustive.py [--workers N]
"""
import argparse
import os
import sys
from multiprocessing import Pool

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CHUNK = 1 << 24


def _fns():
    import fn_ref as R
    return {"exp": (R.exp, np.exp), "tanh": (R.tanh, np.tanh)}


def chunk(k):
    fns = _fns()
    bits = np.arange(k * CHUNK, (k + 1) * CHUNK, dtype=np.uint64).astype(np.uint32)
    x = bits.view(np.float32)
    res = {}
    with np.errstate(all="ignore"):
        for name, (fn, ref) in fns.items():
            y = fn(x)
            r = ref(x.astype(np.float64))
            rf = r.astype(np.float32)
            nan_ok = bool(np.array_equal(np.isnan(y), np.isnan(rf)))
            fin = np.isfinite(rf) & np.isfinite(y)
            sp = np.spacing(np.abs(rf[fin])).astype(np.float64)
            err = np.abs(y[fin].astype(np.float64) - r[fin]) / sp
            inf_ok = bool(np.array_equal(y[~fin & ~np.isnan(rf)], rf[~fin & ~np.isnan(rf)]))
            # monotone over increasing inputs: positive floats in bit order; negative floats in reverse bit order
            yy = y if k < 128 else y[::-1]
            d = np.diff(yy.astype(np.float64))
            ok = ~np.isnan(d)
            down = ok & (d < 0)
            step = (-d[down] / np.spacing(np.abs(yy[1:][down])).astype(np.float64)) if down.any() else np.zeros(1)
            extra = {}
            if name == "tanh":
                extra["odd"] = bool(np.array_equal(fn(-x).view(np.uint32)[~np.isnan(y)], (-y).view(np.uint32)[~np.isnan(y)]))
                extra["bounded"] = bool(np.all(np.abs(y[~np.isnan(y)]) <= 1))
            res[name] = dict(max_ulp=float(err.max()) if err.size else 0.0, nan_ok=nan_ok, inf_ok=inf_ok, n_down=int(down.sum()),
                             max_down_ulp=float(step.max()), first=float(yy[0]), last=float(yy[-1]), **extra)
    return k, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workers", type=int, default=min(8, len(os.sched_getaffinity(0))))
    a = ap.parse_args()
    with Pool(a.workers) as pool:
        out = dict(pool.imap_unordered(chunk, range(1 << 32 >> 24)))
    for name in ("exp", "tanh"):
        rs = [out[k][name] for k in sorted(out)]
        # steps down across chunk boundaries (chunks in the order of increasing input)
        order = list(range(255, 127, -1)) + list(range(0, 128))
        seam = 0
        for u, v in zip(order, order[1:]):
            p, q = out[u][name]["last"], out[v][name]["first"]
            seam += int(not np.isnan(p) and not np.isnan(q) and q < p)
        print(f"{name}: max error {max(r['max_ulp'] for r in rs):.3f} ulp over all 2^32 float inputs; NaN where the reference is NaN: "
              f"{all(r['nan_ok'] for r in rs)}; infinities and zeros exact: {all(r['inf_ok'] for r in rs)}; steps down over increasing "
              f"inputs: {sum(r['n_down'] for r in rs) + seam} (largest {max(r['max_down_ulp'] for r in rs):.0f} ulp)"
              + (f"; odd bitwise: {all(r['odd'] for r in rs)}; |tanh| <= 1: {all(r['bounded'] for r in rs)}" if name == "tanh" else ""))


if __name__ == "__main__":
    main()
