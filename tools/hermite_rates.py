"""Build rates of the Pchip / Akima strategies against the CubicSpline build (output committed as
profiles/hermite_rates.json).  Needs an MI355X; there is no CPU fallback.

    python tools/hermite_rates.py --out profiles/hermite_rates.json
        `create` wall time (device-resident inputs, the call synchronises), median of 7 after a warm-up, one process:
        CubicSpline (the baseline, measured here, not taken from an older profile), Pchip, Akima; f64 and f32 at
        4096 x 4096, 1e6 x 1, 1e5 x 8, 100 x 5.  Also the evaluation time of a Pchip and a CubicSpline handle of the same
        shape and batch (the same kernels: they should agree within run-to-run noise).
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR/<dtype>_<n>x<lanes> -- python tools/hermite_rates.py --profile-shape <dtype> <n> <lanes>
        one run per shape, a run of its own (tracing slows the host): builds each strategy REPS times.
    python tools/hermite_rates.py --merge DIR --out profiles/hermite_rates.json
        adds the build kernels' own times from those runs: per create, hermite_build_kernel (Pchip / Akima) and the sum of
        the spline_* kernels (CubicSpline), with compulsory bytes / time / 8 TB/s for the one-pass kernel.
"""
import argparse
import csv
import glob
import json
import os
import sys
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


def strategies(pkg):
    return {"CubicSpline": pkg.CubicSpline.new, "Pchip": pkg.Pchip.new, "Akima": pkg.Akima.new}


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
    return float(np.median(t)), float(min(t)), float(max(t))


def timing_pass(out_path):
    import torch
    pkg = package()
    assert torch.cuda.is_available() and pkg.device_count() >= 1, "needs a GPU"
    res = {"device": torch.cuda.get_device_name(0), "create_ms": {}, "eval_ms": {}}
    for name, dt in DTYPES.items():
        for n, lanes in SHAPES:
            key = f"{name}_{n}x{lanes}"
            x, xd, yd = inputs(dt, n, lanes)
            res["create_ms"][key] = {}
            for sname, new in strategies(pkg).items():
                def create():
                    return pkg.Interp1D.builder(yd).x(xd).strategy(new()).build()
                med, lo, hi = median_ms(create)
                res["create_ms"][key][sname] = {"median": med, "min": lo, "max": hi}
            nq = max(1000, min(1_000_000, (1 << 29) // (lanes * np.dtype(dt).itemsize)))
            qd = torch.as_tensor(np.random.default_rng(1).uniform(x[0], x[-1], nq).astype(dt), device="cuda:0")
            out = torch.empty((nq, lanes) if lanes > 1 else (nq,), dtype=yd.dtype, device="cuda:0")
            res["eval_ms"][key] = {"queries": nq}
            handles = {s: pkg.Interp1D.builder(yd).x(xd).strategy(strategies(pkg)[s]()).build() for s in ("CubicSpline", "Pchip")}
            for rnd in range(2):           # alternate the two handles: other work shares the host
                for sname, h in handles.items():
                    med, lo, hi = median_ms(lambda: h.interp_array_into(qd, out))
                    res["eval_ms"][key][f"{sname}_round{rnd}"] = {"median": med, "min": lo, "max": hi}
            print(key, json.dumps(res["create_ms"][key]), json.dumps(res["eval_ms"][key]), flush=True)
            del handles, out, qd, xd, yd
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump(res, open(out_path, "w"), indent=1)


def profile_shape(name, n, lanes):
    pkg = package()
    x, xd, yd = inputs(DTYPES[name], n, lanes)
    for sname, new in strategies(pkg).items():
        for _ in range(REPS):
            pkg.Interp1D.builder(yd).x(xd).strategy(new()).build()
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
            per = {"CubicSpline": 0.0, "Pchip": 0.0, "Akima": 0.0}
            names = {"CubicSpline": [], "Pchip": [], "Akima": []}
            for row in csv.DictReader(open(files[0])):
                kn, total = row["Name"], float(row["TotalDurationNs"])
                if "hermite_build_kernel" in kn:
                    rule = kn.split("hermite_build_kernel<")[1].split(",")[1].strip()
                    who = {"1": "Pchip", "2": "Akima"}.get(rule)
                elif "spline_" in kn:
                    who = "CubicSpline"
                else:
                    who = None
                if who:
                    per[who] += total / REPS
                    names[who].append(kn.split("(")[0])
            size = np.dtype(dt).itemsize
            compulsory = 3 * n * lanes * size        # data in, a and b out (+ the k table where the handle keeps one)
            entry = {"compulsory_bytes": compulsory}
            for who, ns in per.items():
                entry[who] = {"kernel_us_per_create": ns / 1e3, "kernels": sorted(set(names[who]))}
                if who != "CubicSpline" and ns > 0:
                    entry[who]["fraction_of_8TBps"] = compulsory / (ns * 1e-9) / PEAK_BPS
            res["build_kernels"][key] = entry
            print(key, json.dumps(entry), flush=True)
    json.dump(res, open(out_path, "w"), indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hermite_rates.json"))
    ap.add_argument("--profile-shape", nargs=3, metavar=("DTYPE", "N", "LANES"))
    ap.add_argument("--merge", metavar="DIR")
    a = ap.parse_args()
    if a.profile_shape:
        profile_shape(a.profile_shape[0], int(a.profile_shape[1]), int(a.profile_shape[2]))
    elif a.merge:
        merge(a.merge, a.out)
    else:
        timing_pass(a.out)
