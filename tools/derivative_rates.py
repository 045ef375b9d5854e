"""Rates of derivative handles (output committed as profiles/derivative_rates.json).  Needs an MI355X; there
is no CPU fallback.  Shapes: the eight of profiles/hermite_rates.json (f64 / f32 at 4096 x 4096, 1e6 x 1, 1e5 x 8, 100 x 5).

    python tools/derivative_rates.py --out profiles/derivative_rates.json
        wall time of derivative(1) and derivative(2) of a CubicSpline handle and derivative(1) of a Pchip handle against
        `create` of a Pchip handle of the same shape (device-resident inputs, every call synchronises), median of 7 after
        a warm-up; then the evaluation time of the derivative handles against their source handle, same batch,
        alternating rounds, with the AUTO plan line each of them printed.
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR/<dtype>_<n>x<lanes> -- python tools/derivative_rates.py --profile-shape <dtype> <n> <lanes>
        one run per shape, a run of its own (tracing slows the host): REPS Pchip builds and REPS derivative(1) of a spline
        in the same process, so derivative_build_kernel and the Pchip hermite_build_kernel are traced side by side.
    python tools/derivative_rates.py --merge DIR --out profiles/derivative_rates.json
        adds the two kernels' own times per launch, their ratio (expectation from bytes: at most 7/3) and the fraction of
        8 TB/s that 7 n L sizeof(T) in that time is.
"""
import argparse
import csv
import glob
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = [(4096, 4096), (1_000_000, 1), (100_000, 8), (100, 5)]
DTYPES = {"f64": np.float64, "f32": np.float32}
REPS = 3
PEAK_BPS = 8.0e12    # HBM3E spec peak of the MI355X


def package():
    from __graft_entry__ import load_package
    return load_package()


def inputs(dt, n, lanes):
    import torch
    rng = np.random.default_rng(n + lanes)
    x = np.cumsum(rng.uniform(0.5, 1.5, n)).astype(dt)
    y = rng.normal(size=(n, lanes) if lanes > 1 else (n,)).astype(dt)
    return x, torch.as_tensor(x, device="cuda:0"), torch.as_tensor(y, device="cuda:0")


def median_ms(fn, reps=7):
    import torch
    fn()                                   # warm-up: code objects, allocations
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    return {"median": float(np.median(t)), "min": float(min(t)), "max": float(max(t))}


def plan_line(fn):
    """the [ndi plan] lines one call prints (NDI_TRACE_PLAN; the library writes them to the C stderr)"""
    import torch
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        os.dup2(tmp.fileno(), 2)
        os.environ["NDI_TRACE_PLAN"] = "1"
        try:
            fn()
            torch.cuda.synchronize()
        finally:
            os.environ.pop("NDI_TRACE_PLAN", None)
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        text = tmp.read().decode(errors="replace")
    return [ln for ln in text.splitlines() if ln.startswith("[ndi plan]")]


def timing_pass(out_path):
    import torch
    pkg = package()
    assert torch.cuda.is_available() and pkg.device_count() >= 1, "needs a GPU"
    res = {"device": torch.cuda.get_device_name(0), "build_ms": {}, "eval_ms": {}}
    for name, dt in DTYPES.items():
        for n, lanes in SHAPES:
            key = f"{name}_{n}x{lanes}"
            x, xd, yd = inputs(dt, n, lanes)
            spline = pkg.Interp1D.builder(yd).x(xd).strategy(pkg.CubicSpline.new()).build()
            pchip = pkg.Interp1D.builder(yd).x(xd).strategy(pkg.Pchip.new()).build()
            # strategy.derivative: the handle alone (Interp1D.derivative also copies Y into a tensor for `.data`)
            res["build_ms"][key] = {
                "Pchip_create": median_ms(lambda: pkg.Interp1D.builder(yd).x(xd).strategy(pkg.Pchip.new()).build()),
                "spline_derivative_1": median_ms(lambda: spline.strategy.derivative(1)),
                "spline_derivative_2": median_ms(lambda: spline.strategy.derivative(2)),
                "Pchip_derivative_1": median_ms(lambda: pchip.strategy.derivative(1)),
                "spline_Interp1D_derivative_1": median_ms(lambda: spline.derivative(1)),
            }
            nq = max(1000, min(1_000_000, (1 << 29) // (lanes * np.dtype(dt).itemsize)))
            qd = torch.as_tensor(np.random.default_rng(1).uniform(x[0], x[-1], nq).astype(dt), device="cuda:0")
            out = torch.empty((nq, lanes) if lanes > 1 else (nq,), dtype=yd.dtype, device="cuda:0")
            handles = {"spline": spline, "spline_d1": spline.derivative(1), "spline_d2": spline.derivative(2),
                       "Pchip": pchip, "Pchip_d1": pchip.derivative(1)}
            ev = {"queries": nq, "plan": {k: plan_line(lambda h=h: h.interp_array_into(qd, out)) for k, h in handles.items()}}
            for rnd in range(2):           # alternate the handles: other work shares the host
                for k, h in handles.items():
                    ev[f"{k}_round{rnd}"] = median_ms(lambda h=h: h.interp_array_into(qd, out))
            res["eval_ms"][key] = ev
            print(key, json.dumps(res["build_ms"][key]), json.dumps(ev), flush=True)
            del handles, spline, pchip, out, qd, xd, yd
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump(res, open(out_path, "w"), indent=1)


def profile_shape(name, n, lanes):
    pkg = package()
    x, xd, yd = inputs(DTYPES[name], n, lanes)
    spline = pkg.Interp1D.builder(yd).x(xd).strategy(pkg.CubicSpline.new()).build()
    for _ in range(REPS):
        pkg.Interp1D.builder(yd).x(xd).strategy(pkg.Pchip.new()).build()
        spline.strategy.derivative(1)
    print("profiled", name, n, lanes, flush=True)


def merge(prof_dir, out_path):
    res = json.load(open(out_path)) if os.path.exists(out_path) else {}
    res["build_kernels"] = {}
    for name, dt in DTYPES.items():
        for n, lanes in SHAPES:
            key = f"{name}_{n}x{lanes}"
            files = glob.glob(os.path.join(prof_dir, key, "**", "*kernel_stats.csv"), recursive=True)
            if not files:
                continue
            us = {"derivative_build_kernel": 0.0, "hermite_build_kernel": 0.0}
            for row in csv.DictReader(open(files[0])):
                for kn in us:
                    if kn in row["Name"]:
                        us[kn] += float(row["TotalDurationNs"]) / REPS / 1e3
            moved = 7 * n * lanes * np.dtype(dt).itemsize     # 4 rows in, 3 out
            entry = {"derivative_kernel_us": us["derivative_build_kernel"], "pchip_kernel_us": us["hermite_build_kernel"],
                     "bytes_7nL": moved}
            if us["derivative_build_kernel"] > 0 and us["hermite_build_kernel"] > 0:
                entry["ratio_to_pchip"] = us["derivative_build_kernel"] / us["hermite_build_kernel"]
                entry["fraction_of_8TBps"] = moved / (us["derivative_build_kernel"] * 1e-6) / PEAK_BPS
            res["build_kernels"][key] = entry
            print(key, json.dumps(entry), flush=True)
    json.dump(res, open(out_path, "w"), indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "derivative_rates.json"))
    ap.add_argument("--profile-shape", nargs=3, metavar=("DTYPE", "N", "LANES"))
    ap.add_argument("--merge", metavar="DIR")
    a = ap.parse_args()
    if a.profile_shape:
        profile_shape(a.profile_shape[0], int(a.profile_shape[1]), int(a.profile_shape[2]))
    elif a.merge:
        merge(a.merge, a.out)
    else:
        timing_pass(a.out)
