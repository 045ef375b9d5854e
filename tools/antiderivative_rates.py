"""Rates of antiderivative handles (output committed as profiles/antiderivative_rates.json).  Needs an
MI355X; there is no CPU fallback.  Shapes: the eight of DESIGN.md 4.11 (f64 / f32 at 4096 x 4096, 1e6 x 1, 1e5 x 8, 100 x 5).

    python tools/antiderivative_rates.py --out profiles/antiderivative_rates.json
        wall time of strategy.antiderivative() of a CubicSpline and a Linear handle against strategy.derivative(1) of the
        same spline (device-resident inputs, every call synchronises), median of 7 after a warm-up; then one device batch
        on the antiderivative handle against the SOURCE handle under NDI_PATH_GATHER (the two-kernel form: like for like)
        and under AUTO (context), same queries and buffer, alternating rounds; then integrate() on the same batch.
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR/<dtype>_<n>x<lanes> -- python tools/antiderivative_rates.py --profile-shape <dtype> <n> <lanes>
        one run per shape, a run of its own (tracing slows the host): REPS derivative(1) and REPS antiderivative() of a
        spline, REPS evaluations of the batch on the antiderivative handle and on the source under NDI_PATH_GATHER.
    python tools/antiderivative_rates.py --merge DIR --out profiles/antiderivative_rates.json
        adds, per launch, the sum of the antiderivative build's kernels against derivative_build_kernel (expectation at
        4096 x 4096: at most 2 x) and the evaluation kernels' times (expectation from bytes: 6/5 cubic, 4/3 Linear).
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


def package():
    from __graft_entry__ import load_package
    return load_package()


def inputs(dt, n, lanes):
    import torch
    rng = np.random.default_rng(n + lanes)
    x = np.cumsum(rng.uniform(0.5, 1.5, n)).astype(dt)
    y = rng.normal(size=(n, lanes) if lanes > 1 else (n,)).astype(dt)
    return x, torch.as_tensor(x, device="cuda:0"), torch.as_tensor(y, device="cuda:0")


def batch(x, dt, lanes, ydtype):
    import torch
    nq = max(1000, min(1_000_000, (1 << 29) // (lanes * np.dtype(dt).itemsize)))
    qd = torch.as_tensor(np.random.default_rng(1).uniform(x[0], x[-1], nq).astype(dt), device="cuda:0")
    out = torch.empty((nq, lanes) if lanes > 1 else (nq,), dtype=ydtype, device="cuda:0")
    return nq, qd, out


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


def with_path(pkg, interp, path):
    interp.strategy.path = path
    return interp


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
            linear = pkg.Interp1D.builder(yd).x(xd).strategy(pkg.Linear.new()).build()
            res["build_ms"][key] = {
                "spline_derivative_1": median_ms(lambda: spline.strategy.derivative(1)),
                "spline_antiderivative": median_ms(lambda: spline.strategy.antiderivative()),
                "linear_antiderivative": median_ms(lambda: linear.strategy.antiderivative()),
            }
            nq, qd, out = batch(x, dt, lanes, yd.dtype)
            hd = qd.flip(0).contiguous()
            Fs, Fl = spline.antiderivative(), linear.antiderivative()
            gs = with_path(pkg, pkg.Interp1D(spline.x, spline.data, spline.strategy.clone(0)), pkg.PATH_GATHER)
            gl = with_path(pkg, pkg.Interp1D(linear.x, linear.data, linear.strategy.clone(0)), pkg.PATH_GATHER)
            o2 = out.view(nq, lanes)
            runs = {"spline_F": lambda: Fs.interp_array_into(qd, out), "spline_gather": lambda: gs.interp_array_into(qd, out),
                    "spline_auto": lambda: spline.interp_array_into(qd, out),
                    "linear_F": lambda: Fl.interp_array_into(qd, out), "linear_gather": lambda: gl.interp_array_into(qd, out),
                    "linear_auto": lambda: linear.interp_array_into(qd, out),
                    "spline_integrate": lambda: Fs.strategy.integrate_into(qd, hd, o2),
                    "linear_integrate": lambda: Fl.strategy.integrate_into(qd, hd, o2)}
            ev = {"queries": nq}
            for rnd in range(2):           # alternate the handles: other work shares the host
                for k, fn in runs.items():
                    ev[f"{k}_round{rnd}"] = median_ms(fn)
            for fam in ("spline", "linear"):
                a = min(ev[f"{fam}_F_round{r}"]["median"] for r in range(2))
                b = min(ev[f"{fam}_gather_round{r}"]["median"] for r in range(2))
                ev[f"{fam}_F_over_gather"] = a / b
            res["eval_ms"][key] = ev
            print(key, json.dumps(res["build_ms"][key]), json.dumps(ev), flush=True)
            del runs, Fs, Fl, gs, gl, spline, linear, out, o2, qd, hd, xd, yd
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump(res, open(out_path, "w"), indent=1)


def profile_shape(name, n, lanes):
    import torch
    pkg = package()
    dt = DTYPES[name]
    x, xd, yd = inputs(dt, n, lanes)
    spline = pkg.Interp1D.builder(yd).x(xd).strategy(pkg.CubicSpline.new()).build()
    nq, qd, out = batch(x, dt, lanes, yd.dtype)
    g = with_path(pkg, pkg.Interp1D(spline.x, spline.data, spline.strategy.clone(0)), pkg.PATH_GATHER)
    for _ in range(REPS):     # exactly REPS launches of everything that merge() divides by REPS
        spline.strategy.derivative(1)
        F = pkg.Interp1D(spline.x, spline.data, spline.strategy.antiderivative())   # (`data` only gives the row shape)
        F.interp_array_into(qd, out)
        g.interp_array_into(qd, out)
    torch.cuda.synchronize()
    print("profiled", name, n, lanes, flush=True)


def merge(prof_dir, out_path):
    res = json.load(open(out_path)) if os.path.exists(out_path) else {}
    res["kernels_us_per_launch"] = {}
    for name in DTYPES:
        for n, lanes in SHAPES:
            key = f"{name}_{n}x{lanes}"
            files = glob.glob(os.path.join(prof_dir, key, "**", "*kernel_stats.csv"), recursive=True)
            if not files:
                continue
            us = {}
            for row in csv.DictReader(open(files[0])):
                nm, t = row["Name"], float(row["TotalDurationNs"]) / 1e3
                if "antideriv" in nm:
                    kn = next(k for k in ("antideriv_local", "antideriv_offsets", "antideriv_add", "antideriv_eval") if k in nm)
                elif "derivative_build_kernel" in nm:
                    kn = "derivative_build_kernel"
                elif "locate_kernel" in nm or "range_check_kernel" in nm:
                    kn = "search_kernels_total"         # both handles' searches (the source's fused forms search inside)
                elif "eval_" in nm:
                    kn = "source_eval_kernel"           # whatever form NDI_PATH_GATHER gives the source
                else:
                    continue
                if kn.startswith("antideriv") or kn == "derivative_build_kernel":
                    assert int(row["Calls"]) == REPS, (key, nm, row["Calls"])     # what "per launch" below relies on
                us[kn] = us.get(kn, 0.0) + t
            # REPS launches of each: derivative(1), antiderivative(), one batch on F, one batch on the source
            entry = {k: (v if k == "search_kernels_total" else v / REPS) for k, v in us.items()}
            build = sum(entry.get(k, 0.0) for k in ("antideriv_local", "antideriv_offsets", "antideriv_add"))
            entry["antiderivative_build_sum"] = build
            if entry.get("derivative_build_kernel"):
                entry["build_over_derivative"] = build / entry["derivative_build_kernel"]
            if entry.get("source_eval_kernel") and entry.get("antideriv_eval"):
                entry["eval_over_source_gather"] = entry["antideriv_eval"] / entry["source_eval_kernel"]
            res["kernels_us_per_launch"][key] = entry
            print(key, json.dumps(entry), flush=True)
    json.dump(res, open(out_path, "w"), indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "antiderivative_rates.json"))
    ap.add_argument("--profile-shape", nargs=3, metavar=("DTYPE", "N", "LANES"))
    ap.add_argument("--merge", metavar="DIR")
    a = ap.parse_args()
    if a.profile_shape:
        profile_shape(a.profile_shape[0], int(a.profile_shape[1]), int(a.profile_shape[2]))
    elif a.merge:
        merge(a.merge, a.out)
    else:
        timing_pass(a.out)
