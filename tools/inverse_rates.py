"""Rates of inverse handles (output committed as profiles/inverse_rates.json).  Needs an MI355X; there is
no CPU fallback.  Classes: Linear, the cubic class (Pchip), the antiderivative of a Pchip and of a Linear; f64 / f32 at
4096 x 4096, 1e6 x 1, 1e5 x 8 and 100 x 5.

    python tools/inverse_rates.py --out profiles/inverse_rates.json
        one device batch of uniformly random in-range values on the inverse handle against the FORWARD evaluation of the
        source handle under NDI_PATH_GATHER on a batch of the same size (the same output bytes, the same table footprint),
        alternating rounds, median of 7 after a warm-up, every call synchronised; the ratio; the fraction of the 8 TB/s
        spec on the compulsory output bytes; and the mean iteration count of the batch's first rows and lanes as
        tests/inverse_ref.py reports it on the handles' own tables.  Batches: 1e7 queries, fewer where the rows are long
        (the output is kept to 512 MiB: 16384 / 32768 queries at 4096 lanes).
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR/<dtype>_<n>x<lanes> -- python tools/inverse_rates.py --profile-shape <dtype> <n> <lanes>
        one run per shape, a run of its own (tracing slows the host): REPS evaluations of the batch per class on the
        inverse handle and on the source.
    python tools/inverse_rates.py --merge DIR --out profiles/inverse_rates.json
        adds the kernel times per launch.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
SHAPES = [(4096, 4096), (1_000_000, 1), (100_000, 8), (100, 5)]
DTYPES = {"f64": np.float64, "f32": np.float32}
CLASSES = ("linear", "pchip", "anti_pchip", "anti_linear")
REPS = 3
SPEC_TBPS = 8.0


def package():
    from __graft_entry__ import load_package
    return load_package()


def source(pkg, cls, dt, n, lanes):
    """(the handle to invert, the handle whose tables its polynomial uses): monotone lanes, alternating directions with a
    common range of about [-1, 1]; antiderivatives: non-negative data, a third of it zero"""
    import torch
    rng = np.random.default_rng(n + lanes)
    x = np.cumsum(rng.uniform(0.5, 1.5, n)).astype(dt)
    if cls.startswith("anti_"):
        y = np.abs(rng.normal(size=(n, lanes)))
        y[rng.random((n, lanes)) < 0.3] = 0.0
        y[0] = 1.0
    else:
        inc = rng.uniform(0.0, 1.0, (n - 1, lanes))
        inc[rng.random((n - 1, lanes)) < 0.15] = 0.0
        inc[0] = 1.0
        c = np.concatenate([np.zeros((1, lanes)), np.cumsum(inc, axis=0)])
        pad = rng.uniform(0.0, 0.25, (2, lanes))
        y = ((-1.0 - pad[0]) + c / c[-1] * (2.0 + pad[0] + pad[1])) * np.where(np.arange(lanes) % 2 == 1, -1.0, 1.0)
    yd = torch.as_tensor(y.astype(dt), device="cuda:0")
    xd = torch.as_tensor(x, device="cuda:0")
    strat = pkg.Linear.new() if cls in ("linear", "anti_linear") else pkg.Pchip.new()
    base = pkg.Interp1D.builder(yd).x(xd).strategy(strat).build()
    return x, (base.antiderivative() if cls.startswith("anti_") else base), base


def batch(inv, src, x, dt, lanes):
    """(nq, values in [Lo, Hi], abscissae in [x0, xn], output), all on the device"""
    import torch
    nq = int(max(16384, min(10_000_000, (1 << 29) // (lanes * np.dtype(dt).itemsize))))
    N = inv.strategy.data_table(device=True)
    ends = torch.stack([N[0], N[-1]])
    lo, hi = float(ends.min(0).values.max()), float(ends.max(0).values.min())
    rng = np.random.default_rng(1)
    v = np.clip(rng.uniform(lo, hi, nq).astype(dt), dt(lo), dt(hi))
    xs = rng.uniform(x[0], x[-1], nq).astype(dt)
    out = torch.empty((nq, lanes), dtype=N.dtype, device="cuda:0")
    return nq, torch.as_tensor(v, device="cuda:0"), torch.as_tensor(xs, device="cuda:0"), out


def mean_iterations(cls, inv, base, x, vd, rows=4096, lanes=8):
    """the restatement's mean iteration count on the first `rows` values and `lanes` lanes, from the handles' own tables"""
    import inverse_ref
    kind = {"linear": "linear", "pchip": "cubic", "anti_pchip": "anti_cubic", "anti_linear": "anti_linear"}[cls]
    cut = lambda t: np.ascontiguousarray(t[:, :lanes].cpu().numpy())      # noqa: E731
    N = cut(inv.strategy.data_table(device=True))
    y = cut(base.strategy.data_table(device=True)) if kind.startswith("anti") else None
    a = b = None
    if kind in ("cubic", "anti_cubic"):
        a, b = (np.ascontiguousarray(t[:, :lanes]) for t in base.strategy.coefficients())
    lo, hi = inverse_ref.common_range(N)
    v = vd[:rows].cpu().numpy()
    v = v[(v >= lo) & (v <= hi)]
    _, it = inverse_ref.solve(kind, x, N, v, y, a, b)
    return float(it.mean()), int(it.max())


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


def timing_pass(out_path):
    import torch
    pkg = package()
    assert torch.cuda.is_available() and pkg.device_count() >= 1, "needs a GPU"
    res = {"device": torch.cuda.get_device_name(0), "eval_ms": {}}
    for name, dt in DTYPES.items():
        for n, lanes in SHAPES:
            for cls in CLASSES:
                key = f"{name}_{n}x{lanes}_{cls}"
                x, src, base = source(pkg, cls, dt, n, lanes)
                src.strategy.path = pkg.PATH_GATHER
                t0 = time.perf_counter()
                inv = src.inverse()
                torch.cuda.synchronize()
                create_ms = (time.perf_counter() - t0) * 1e3
                nq, vd, xd, out = batch(inv, src, x, dt, lanes)
                o = out
                runs = {"inverse": lambda: inv.interp_array_into(vd, o), "forward_gather": lambda: src.interp_array_into(xd, o)}
                ev = {"queries": nq, "create_ms": create_ms}
                for rnd in range(2):           # alternate the handles: other work shares the host
                    for k, fn in runs.items():
                        ev[f"{k}_round{rnd}"] = median_ms(fn)
                inv_ms = min(ev[f"inverse_round{r}"]["median"] for r in range(2))
                fwd_ms = min(ev[f"forward_gather_round{r}"]["median"] for r in range(2))
                ev["inverse_over_forward"] = inv_ms / fwd_ms
                ev["output_fraction_of_spec"] = nq * lanes * np.dtype(dt).itemsize / (inv_ms * 1e-3) / (SPEC_TBPS * 1e12)
                ev["mean_iterations"], ev["most_iterations"] = mean_iterations(cls, inv, base, x, vd)
                res["eval_ms"][key] = ev
                print(key, json.dumps(ev), flush=True)
                del runs, inv, src, base, out, o, vd, xd
                torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump(res, open(out_path, "w"), indent=1)


def profile_shape(name, n, lanes):
    import torch
    pkg = package()
    dt = DTYPES[name]
    for cls in CLASSES:
        x, src, base = source(pkg, cls, dt, n, lanes)
        src.strategy.path = pkg.PATH_GATHER
        inv = src.inverse()
        nq, vd, xd, out = batch(inv, src, x, dt, lanes)
        o = out
        for _ in range(REPS):     # exactly REPS launches of everything that merge() divides by REPS
            inv.interp_array_into(vd, o)
            src.interp_array_into(xd, o)
        torch.cuda.synchronize()
        del inv, src, base, out, o, vd, xd
        torch.cuda.empty_cache()
    print("profiled", name, n, lanes, flush=True)


def merge(prof_dir, out_path):
    """per shape: the inverse kernel's time per launch by class (the template argument in its name: 0 Linear, 1 cubic,
    2 / 3 the antiderivatives) and the creation pass's"""
    res = json.load(open(out_path)) if os.path.exists(out_path) else {}
    res["kernels_us_per_launch"] = {}
    names = {", 0>": "linear", ", 1>": "pchip", ", 2>": "anti_pchip", ", 3>": "anti_linear"}
    for name in DTYPES:
        for n, lanes in SHAPES:
            key = f"{name}_{n}x{lanes}"
            files = glob.glob(os.path.join(prof_dir, key, "**", "*kernel_stats.csv"), recursive=True)
            if not files:
                continue
            entry = {}
            for row in csv.DictReader(open(files[0])):
                nm, t, calls = row["Name"], float(row["TotalDurationNs"]) / 1e3, int(row["Calls"])
                if "inverse_eval_kernel" in nm:
                    cls = next(v for k, v in names.items() if k in nm)
                    assert calls == REPS, (key, nm, calls)
                    entry[f"inverse_eval_{cls}"] = t / REPS
                elif "inverse_check_kernel" in nm:
                    entry["inverse_check_mean"] = t / calls
            res["kernels_us_per_launch"][key] = entry
            print(key, json.dumps(entry), flush=True)
    json.dump(res, open(out_path, "w"), indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inverse_rates.json"))
    ap.add_argument("--profile-shape", nargs=3, metavar=("DTYPE", "N", "LANES"))
    ap.add_argument("--merge", metavar="DIR")
    a = ap.parse_args()
    if a.profile_shape:
        profile_shape(a.profile_shape[0], int(a.profile_shape[1]), int(a.profile_shape[2]))
    elif a.merge:
        merge(a.merge, a.out)
    else:
        timing_pass(a.out)
