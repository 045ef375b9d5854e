#!/usr/bin/env python3
"""tools/int_rates.py -- i32 vs f32 and i64 vs f64 on the same shapes, in one process.

Cases: C2-like Linear 4096 knots x 4096 lanes at 1e6 queries; scalar Linear on 100 knots at 1e7 queries; Bilinear
100 x 100 x 5 at 1e6 queries; C3-like Bilinear 2048 x 2048 x 64 at 1e7 queries.  Device queries in, a device output
allocated for the call (NDI_EVAL_FRESH_OUTPUT, what interp_array does), AUTO path.  Per case: the median call time,
compulsory bytes (queries + output + the data table once: repeated operand rows come from the caches) over the time as
a fraction of 8 TB/s, and the ratio to the float sibling of the same width.  Prints one JSON document.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import load_product_package  # noqa: E402

pkg = load_product_package()
PEAK = 8e12
REPS, WARM = 7, 2


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(WARM):
        fn()
    ts = []
    for _ in range(REPS):
        torch.cuda.synchronize()
        s.record()
        fn()
        e.record()
        e.synchronize()
        ts.append(s.elapsed_time(e))
    return float(np.median(ts))


def case_1d(n, lanes, nq, dt, rng):
    dev = "cuda:0"
    x = np.arange(n, dtype=dt) * 3
    data = rng.integers(-1000, 1000, (n, lanes)).astype(dt) if lanes > 1 else rng.integers(-1000, 1000, n).astype(dt)
    interp = pkg.Interp1DBuilder.new(torch.as_tensor(data, device=dev)).x(x).strategy(pkg.Linear.new().device(0)).build()
    q = torch.as_tensor(rng.integers(0, int(x[-1]) + 1, nq).astype(dt), device=dev)
    out = torch.empty((nq, lanes), dtype=q.dtype, device=dev)
    ms = timed(lambda: interp.strategy.interp_array_into(interp, q, out, fresh=True))
    sz = np.dtype(dt).itemsize
    return ms, nq * (sz + lanes * sz) + n * lanes * sz


def case_2d(nx, ny, lanes, nq, dt, rng):
    dev = "cuda:0"
    x = np.arange(nx, dtype=dt) * 2
    y = np.arange(ny, dtype=dt) * 5
    g = rng.integers(-1000, 1000, (nx, ny, lanes)).astype(dt)
    interp = pkg.Interp2DBuilder.new(torch.as_tensor(g, device=dev)).x(x).y(y).strategy(
        pkg.Bilinear.new().device(0)).build()
    qx = torch.as_tensor(rng.integers(0, int(x[-1]) + 1, nq).astype(dt), device=dev)
    qy = torch.as_tensor(rng.integers(0, int(y[-1]) + 1, nq).astype(dt), device=dev)
    out = torch.empty((nq, lanes), dtype=qx.dtype, device=dev)
    ms = timed(lambda: interp.strategy.interp_array_into(interp, qx, qy, out, fresh=True))
    sz = np.dtype(dt).itemsize
    return ms, nq * (2 * sz + lanes * sz) + nx * ny * lanes * sz


def main():
    rng = np.random.default_rng(0)
    cases = [("C2-like Linear 4096 x 4096, 1e6 queries", case_1d, (4096, 4096, 1_000_000)),
             ("scalar Linear, 100 knots, 1e7 queries", case_1d, (100, 1, 10_000_000)),
             ("Bilinear 100 x 100 x 5, 1e6 queries", case_2d, (100, 100, 5, 1_000_000)),
             ("C3-like Bilinear 2048 x 2048 x 64, 1e7 queries", case_2d, (2048, 2048, 64, 10_000_000))]
    rows = []
    for name, fn, args in cases:
        for idt, fdt in ((np.int32, np.float32), (np.int64, np.float64)):
            r = {}
            for dt in (fdt, idt):
                ms, nbytes = fn(*args, dt, rng)
                r[np.dtype(dt).name] = {"ms": round(ms, 4), "frac_of_8TBps": round(nbytes / (ms * 1e-3) / PEAK, 3)}
                torch.cuda.empty_cache()
            r["int_over_float"] = round(r[np.dtype(idt).name]["ms"] / r[np.dtype(fdt).name]["ms"], 3)
            rows.append({"case": name, **r})
            print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    print(json.dumps({"tool": "int_rates", "device": torch.cuda.get_device_name(0), "cases": rows}, indent=1))


if __name__ == "__main__":
    main()
