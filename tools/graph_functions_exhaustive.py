#!/usr/bin/env python3
"""Exhaustive check of the float graph functions exp, tanh, log, sin and cos over all 2^32 float inputs (no GPU: the numpy restatements
of tests/fn_ref.py and tests/fn_ref_trig.py, which the GPU tests hold the kernels to bit for bit).

Prints, per function: the largest error in ulps of the correctly rounded result (float64 reference, whose own error is far below a float
ulp), NaN agreement, and how monotone the result is over the inputs in increasing order: the number of places where the result steps
down, and the largest such step in ulps.  tanh is also checked for oddness (tanh(-x) = -tanh(x) bitwise) and |tanh| <= 1.
sin and cos are measured over every float with |a| < 2^20 (their domain; everything else must give NaN) and checked for: sin odd and
cos even bitwise, |sin|, |cos| <= 1, sin(a) = a for |a| < 2^-13 (subnormals included).  --double-log measures the float64 log on 2^22
stratified inputs (double_log_inputs: every exponent, subnormals included, and a dense stratum [0.5, 2)) against mpmath.
The numbers are the ones include/flowz_hip.h states.

usage: tools/graph_functions_exhaustive.py [--workers N] [--functions exp,tanh,log,sin,cos] [--double-log]
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


ONLY = None     # the functions to measure (None: all)


def _fns():
    import fn_ref as R
    import fn_ref_trig as RT
    fns = {"exp": (R.exp, np.exp), "tanh": (R.tanh, np.tanh), "log": (RT.log, np.log), "sin": (RT.sin, np.sin), "cos": (RT.cos, np.cos)}
    return {k: v for k, v in fns.items() if ONLY is None or k in ONLY}


def _set_only(only):
    global ONLY
    ONLY = only


def chunk(k):
    fns = _fns()
    bits = np.arange(k * CHUNK, (k + 1) * CHUNK, dtype=np.uint64).astype(np.uint32)
    x = bits.view(np.float32)
    res = {}
    with np.errstate(all="ignore"):
        for name, (fn, ref) in fns.items():
            y = fn(x)
            r = ref(x.astype(np.float64))
            if name in ("sin", "cos"):                      # the domain rule: NaN from 2^20 on
                r = np.where(np.abs(x) < np.float32(2.0 ** 20), r, np.nan)
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
            if name in ("sin", "cos"):
                ym = fn(-x)
                sym = (-y if name == "sin" else y)
                extra["odd" if name == "sin" else "even"] = bool(np.array_equal(ym.view(np.uint32)[~np.isnan(y)], sym.view(np.uint32)[~np.isnan(y)]))
                extra["bounded"] = bool(np.all(np.abs(y[~np.isnan(y)]) <= 1))
                if name == "sin":
                    tiny = np.abs(x) < np.float32(2.0 ** -13)
                    extra["tiny"] = bool(np.array_equal(y[tiny].view(np.uint32), x[tiny].view(np.uint32)))
            res[name] = dict(max_ulp=float(err.max()) if err.size else 0.0, nan_ok=nan_ok, inf_ok=inf_ok, n_down=int(down.sum()),
                             max_down_ulp=float(step.max()), first=float(yy[0]), last=float(yy[-1]), **extra)
    return k, res


def double_log_inputs(k):
    """chunk k of 128 of the 2^22 stratified float64 inputs of log: the exponent fields [16 k, 16 k + 16) of the positive doubles with 1024
    random mantissas each (subnormals included; the infinity / NaN field left out), and 16384 values drawn uniformly from [0.5, 2), where
    e = 0 or -1 and the polynomial carries the whole result"""
    rng = np.random.default_rng(1000 + k)
    e = np.repeat(np.arange(16 * k, 16 * k + 16, dtype=np.uint64), 1024)
    x = ((e << np.uint64(52)) | rng.integers(0, 1 << 52, e.size, dtype=np.uint64)).view(np.float64)
    x = x[(x > 0) & np.isfinite(x)]
    return np.concatenate([x, rng.uniform(0.5, 2.0, 16384)])


def double_log_worst(x):
    """the largest error of the float64 log restatement on x in ulps of the correctly rounded result (mpmath)"""
    import mpmath as mp
    import fn_ref_trig as RT
    mp.mp.prec = 160
    worst = 0.0
    for xi, yi in zip(x.tolist(), RT.log(x).tolist()):
        t = mp.log(mp.mpf(xi))
        if t == 0:
            worst = max(worst, abs(yi) / 5e-324)
            continue
        worst = max(worst, float(abs(mp.mpf(yi) - t) / mp.mpf(float(np.spacing(abs(float(t)))))))
    return worst


def double_log_chunk(k):
    x = double_log_inputs(k)
    return double_log_worst(x), int(x.size)


def main():
    global ONLY
    ap = argparse.ArgumentParser()
    ap.add_argument("--workers", type=int, default=min(8, len(os.sched_getaffinity(0))))
    ap.add_argument("--functions", default="exp,tanh,log,sin,cos")
    ap.add_argument("--double-log", action="store_true", help="only the float64 log against mpmath on 2^22 stratified inputs")
    a = ap.parse_args()
    if a.double_log:
        with Pool(a.workers) as pool:
            rs = pool.map(double_log_chunk, range(128))
        print(f"log (float64): max error {max(r[0] for r in rs):.3f} ulp on {sum(r[1] for r in rs)} stratified inputs against mpmath")
        return
    ONLY = set(a.functions.split(","))
    with Pool(a.workers, initializer=_set_only, initargs=(ONLY,)) as pool:
        out = dict(pool.imap_unordered(chunk, range(1 << 32 >> 24)))
    for name in [n for n in ("exp", "tanh", "log", "sin", "cos") if n in ONLY]:
        rs = [out[k][name] for k in sorted(out)]
        # steps down across chunk boundaries (chunks in the order of increasing input)
        order = list(range(255, 127, -1)) + list(range(0, 128))
        seam = 0
        for u, v in zip(order, order[1:]):
            p, q = out[u][name]["last"], out[v][name]["first"]
            seam += int(not np.isnan(p) and not np.isnan(q) and q < p)
        print(f"{name}: max error {max(r['max_ulp'] for r in rs):.3f} ulp over all 2^32 float inputs; NaN where the reference is NaN: "
              f"{all(r['nan_ok'] for r in rs)}; infinities and zeros exact: {all(r['inf_ok'] for r in rs)}"
              + ("" if name in ("sin", "cos") else f"; steps down over increasing inputs: {sum(r['n_down'] for r in rs) + seam} "
                 f"(largest {max(r['max_down_ulp'] for r in rs):.0f} ulp)")
              + (f"; odd bitwise: {all(r['odd'] for r in rs)}; |tanh| <= 1: {all(r['bounded'] for r in rs)}" if name == "tanh" else "")
              + (f"; odd bitwise: {all(r['odd'] for r in rs)}; |sin| <= 1: {all(r['bounded'] for r in rs)}; sin(a) = a below 2^-13: "
                 f"{all(r['tiny'] for r in rs)}" if name == "sin" else "")
              + (f"; even bitwise: {all(r['even'] for r in rs)}; |cos| <= 1: {all(r['bounded'] for r in rs)}" if name == "cos" else ""))
        if name in ("sin", "cos"):
            print(f"   ({name}: measured where |a| < 2^20; NaN everywhere else: {all(r['nan_ok'] for r in rs)}; the error printed with 7 digits: "
                  f"{max(r['max_ulp'] for r in rs):.7f} ulp)")


if __name__ == "__main__":
    main()
