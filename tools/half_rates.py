#!/usr/bin/env python3
"""tools/half_rates.py -- f16 and bf16 vs f32 on the same shapes, in one process.

Cases: C2-like Linear 4096 knots x 4096 lanes at 1e6 queries; scalar Linear on 100 knots at 1e7 queries; Bilinear
100 x 100 x 5 at 1e6 queries; C3-like Bilinear 2048 x 2048 x 64 at 1e7 queries.  Device queries in, a device output
allocated for the call (NDI_EVAL_FRESH_OUTPUT, what interp_array does), AUTO path.  Per case: the median of 7 call
times, compulsory bytes (queries + output + the data table once: repeated operand rows come from the caches) over the
time as a fraction of 8 TB/s, and the ratio to f32.  Prints one JSON document.
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
TDT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}


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


def axis(n, dt):
    """n consecutive values of T from 1.0 up (f32 takes the f16 ones): strictly rising in every type."""
    bits = torch.arange(n, dtype=torch.int32) + (0x3F80 if dt == "bf16" else 0x3C00)
    x = bits.to(torch.int16).view(torch.bfloat16 if dt == "bf16" else torch.float16)
    return x if dt != "f32" else x.float()


def queries(x, nq, t, rng):
    q = rng.uniform(float(x[0]), float(x[-1]), nq).astype(np.float32)
    return torch.as_tensor(q, device="cuda:0").to(t)


def case_1d(n, lanes, nq, dt, rng):
    dev, t = "cuda:0", TDT[dt]
    x = axis(n, dt)
    shape = (n, lanes) if lanes > 1 else (n,)
    data = torch.as_tensor(rng.uniform(-1, 1, shape).astype(np.float32), device=dev).to(t)
    interp = pkg.Interp1DBuilder.new(data).x(x).strategy(pkg.Linear.new().device(0)).build()
    q = queries(x, nq, t, rng)
    out = torch.empty((nq, lanes), dtype=t, device=dev)
    ms = timed(lambda: interp.strategy.interp_array_into(interp, q, out, fresh=True))
    sz = data.element_size()
    return ms, nq * (sz + lanes * sz) + n * lanes * sz


def case_2d(nx, ny, lanes, nq, dt, rng):
    dev, t = "cuda:0", TDT[dt]
    x, y = axis(nx, dt), axis(ny, dt)
    g = torch.as_tensor(rng.uniform(-1, 1, (nx, ny, lanes)).astype(np.float32), device=dev).to(t)
    interp = pkg.Interp2DBuilder.new(g).x(x).y(y).strategy(pkg.Bilinear.new().device(0)).build()
    qx, qy = queries(x, nq, t, rng), queries(y, nq, t, rng)
    out = torch.empty((nq, lanes), dtype=t, device=dev)
    ms = timed(lambda: interp.strategy.interp_array_into(interp, qx, qy, out, fresh=True))
    sz = g.element_size()
    return ms, nq * (2 * sz + lanes * sz) + nx * ny * lanes * sz


def main():
    rng = np.random.default_rng(0)
    cases = [("C2-like Linear 4096 x 4096, 1e6 queries", case_1d, (4096, 4096, 1_000_000), 0.6),
             ("scalar Linear, 100 knots, 1e7 queries", case_1d, (100, 1, 10_000_000), 1.25),
             ("Bilinear 100 x 100 x 5, 1e6 queries", case_2d, (100, 100, 5, 1_000_000), 1.5),
             ("C3-like Bilinear 2048 x 2048 x 64, 1e7 queries", case_2d, (2048, 2048, 64, 10_000_000), 2.0)]
    only = os.environ.get("HALF_RATES_CASES")   # e.g. "0,1": a subset of the cases
    rows = []
    for k, (name, fn, args, target) in enumerate(cases):
        if only and str(k) not in only.split(","):
            continue
        r = {"target_over_f32": target}
        for dt in ("f32", "f16", "bf16"):
            ms, nbytes = fn(*args, dt, rng)
            r[dt] = {"ms": round(ms, 4), "frac_of_8TBps": round(nbytes / (ms * 1e-3) / PEAK, 3)}
            torch.cuda.empty_cache()
        for dt in ("f16", "bf16"):
            r[f"{dt}_over_f32"] = round(r[dt]["ms"] / r["f32"]["ms"], 3)
        rows.append({"case": name, **r})
        print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    print(json.dumps({"tool": "half_rates", "device": torch.cuda.get_device_name(0), "reps": REPS, "cases": rows},
                     indent=1))


if __name__ == "__main__":
    main()
