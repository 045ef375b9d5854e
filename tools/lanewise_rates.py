"""Rates of the lane-wise evaluation (output committed as profiles/lanewise_rates.json).  Needs an MI355X;
there is no CPU fallback.  Classes: Linear and the cubic class (Pchip); f64 / f32 at 4096 x 4096, 1e6 x 1, 1e5 x 8 and
100 x 5 -- the shapes and the protocol of tools/inverse_rates.py.

    python tools/lanewise_rates.py --out profiles/lanewise_rates.json
        one device batch of (rows, lanes) queries into a device buffer, for uniformly random per-lane queries and for queries
        broadcast along lanes: the lane-wise call as AUTO takes it, with the element-record copy (NDI_LANEWISE_RECORDS=1),
        with the plain tables (0) and in the two-kernel form (NDI_LANEWISE_MODE=1), and beside them the FORWARD
        ndi_interp1d_eval of the same handle under NDI_PATH_GATHER on `rows` queries (the same number of output elements).
        Alternating rounds, median of 7 after a warm-up, every call synchronised, best of the two rounds; the spread between
        the rounds; the fraction of the 8 TB/s spec on the compulsory bytes (the query plus the output).  Batches: 1e7 rows,
        fewer where the rows are long (the output is kept to 512 MiB).
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR/<dtype>_<n>x<lanes> -- python tools/lanewise_rates.py --profile-shape <dtype> <n> <lanes>
        one run per shape, a run of its own (tracing slows the host): REPS evaluations per class, query kind and form.
    python tools/lanewise_rates.py --merge DIR --out profiles/lanewise_rates.json
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

os.environ["NDI_TUNE_LIVE"] = "1"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = [(4096, 4096), (1_000_000, 1), (100_000, 8), (100, 5)]
DTYPES = {"f64": np.float64, "f32": np.float32}
CLASSES = ("linear", "pchip")
# form -> (NDI_LANEWISE_RECORDS, NDI_LANEWISE_MODE); None: unset (AUTO)
FORMS = {"auto": (None, None), "records": ("1", "2"), "plain": ("0", "2"), "two_kernel": ("0", "1")}
QUERIES = ("random", "broadcast")
REPS = 3
SPEC_TBPS = 8.0


def package():
    from __graft_entry__ import load_package
    return load_package()


def set_form(form):
    for name, v in zip(("NDI_LANEWISE_RECORDS", "NDI_LANEWISE_MODE"), FORMS[form]):
        if v is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = v


def handle(pkg, cls, dt, n, lanes):
    import torch
    rng = np.random.default_rng(n + lanes)
    x = np.cumsum(rng.uniform(0.5, 1.5, n)).astype(dt)
    yd = torch.as_tensor(rng.normal(size=(n, lanes)).astype(dt), device="cuda:0")
    strat = pkg.Linear.new() if cls == "linear" else pkg.Pchip.new()
    it = pkg.Interp1D.builder(yd).x(torch.as_tensor(x, device="cuda:0")).strategy(strat).build()
    it.strategy.path = pkg.PATH_GATHER
    return x, it


def batch(x, dt, lanes):
    """(rows, {query kind: (rows, lanes) abscissae}, the forward call's `rows` abscissae, output), all on the device"""
    import torch
    rows = int(max(16384, min(10_000_000, (1 << 29) // (lanes * np.dtype(dt).itemsize))))
    tdt = torch.float64 if dt == np.float64 else torch.float32
    g = torch.Generator(device="cuda:0").manual_seed(1)
    lo, hi = float(x[0]), float(x[-1])

    def uniform(shape):
        return (lo + (hi - lo) * torch.rand(shape, generator=g, device="cuda:0", dtype=torch.float64)).to(tdt).clamp_(lo, hi)
    one = uniform((rows,))
    q = {"random": uniform((rows, lanes)), "broadcast": one[:, None].expand(rows, lanes).contiguous()}
    return rows, q, one, torch.empty((rows, lanes), dtype=tdt, device="cuda:0")


def median_ms(fn, reps=7):
    import torch
    fn()                                   # warm-up: code objects, allocations, the record copy
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def timing_pass(out_path):
    import torch
    pkg = package()
    assert torch.cuda.is_available() and pkg.device_count() >= 1, "needs a GPU"
    res = {"device": torch.cuda.get_device_name(0), "eval_ms": {}}
    for name, dt in DTYPES.items():
        for n, lanes in SHAPES:
            for cls in CLASSES:
                x, it = handle(pkg, cls, dt, n, lanes)
                rows, q, one, out = batch(x, dt, lanes)
                for kind in QUERIES:
                    key = f"{name}_{n}x{lanes}_{cls}_{kind}"
                    qd = q[kind]

                    def lanewise(form):
                        def run():
                            set_form(form)
                            it.interp_lanewise_into(qd, out, fresh=True)
                        return run
                    runs = {form: lanewise(form) for form in FORMS}
                    runs["forward_gather"] = lambda: it.interp_array_into(one, out)
                    rounds = {k: [] for k in runs}
                    for _ in range(2):           # alternate the forms: other work shares the host
                        for k, fn in runs.items():
                            rounds[k].append(median_ms(fn))
                    ev = {"rows": rows}
                    for k, v in rounds.items():
                        ev[k] = {"ms": min(v), "rounds": v, "spread": abs(v[0] - v[1])}
                    ev["auto_over_forward"] = ev["auto"]["ms"] / ev["forward_gather"]["ms"]
                    nbytes = 2 * rows * lanes * np.dtype(dt).itemsize
                    ev["compulsory_fraction_of_spec"] = nbytes / (ev["auto"]["ms"] * 1e-3) / (SPEC_TBPS * 1e12)
                    res["eval_ms"][key] = ev
                    print(key, json.dumps(ev), flush=True)
                set_form("auto")
                del it, q, one, out, qd, runs
                torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump(res, open(out_path, "w"), indent=1)


def profile_shape(name, n, lanes):
    import torch
    pkg = package()
    dt = DTYPES[name]
    for cls in CLASSES:
        x, it = handle(pkg, cls, dt, n, lanes)
        rows, q, one, out = batch(x, dt, lanes)
        for kind in QUERIES:
            for form in ("records", "plain", "two_kernel"):
                set_form(form)
                for _ in range(REPS):
                    it.interp_lanewise_into(q[kind], out, fresh=True)
        torch.cuda.synchronize()
        del it, q, one, out
        torch.cuda.empty_cache()
    print("profiled", name, n, lanes, flush=True)


def merge(prof_dir, out_path):
    """per shape: mean time per launch of every lane-wise kernel instantiation and of locate_kernel, over both classes and
    query kinds (the instantiation's template arguments tell the class, the staging and the table layout)"""
    res = json.load(open(out_path)) if os.path.exists(out_path) else {}
    res["kernels_us_per_launch"] = {}
    for name in DTYPES:
        for n, lanes in SHAPES:
            key = f"{name}_{n}x{lanes}"
            files = glob.glob(os.path.join(prof_dir, key, "**", "*kernel_stats.csv"), recursive=True)
            if not files:
                continue
            entry = {}
            for row in csv.DictReader(open(files[0])):
                nm, t, calls = row["Name"], float(row["TotalDurationNs"]) / 1e3, int(row["Calls"])
                if "lanewise" in nm or "locate_kernel" in nm:
                    short = nm.split("(")[0].replace("void ", "").replace("ndi::", "")
                    entry[short] = {"us": t / calls, "calls": calls}
            res["kernels_us_per_launch"][key] = entry
            print(key, json.dumps(entry), flush=True)
    json.dump(res, open(out_path, "w"), indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lanewise_rates.json"))
    ap.add_argument("--profile-shape", nargs=3, metavar=("DTYPE", "N", "LANES"))
    ap.add_argument("--merge", metavar="DIR")
    a = ap.parse_args()
    if a.profile_shape:
        profile_shape(a.profile_shape[0], int(a.profile_shape[1]), int(a.profile_shape[2]))
    elif a.merge:
        merge(a.merge, a.out)
    else:
        timing_pass(a.out)
