"""Rates of the 2-D lane-wise evaluation (output committed as profiles/lanewise2d_rates.json).  Needs an
MI355X; there is no CPU fallback.  Classes: Bilinear and Bicubic (the spline); f64 / f32 on 100 x 100 x 5 (the reference's
bench grid), 2048 x 2048 x 8 (a grid beyond L2), 64 x 64 x 4096 (a wide trailing axis) and 1000 x 1000 x 1 (a scalar grid)
-- the protocol of tools/lanewise_rates.py.

    python tools/lanewise2d_rates.py --out profiles/lanewise2d_rates.json
        one device batch of (rows, lanes) query pairs into a device buffer under NDI_EVAL_FRESH_OUTPUT, for uniformly random
        per-lane queries and for queries broadcast along lanes: the lane-wise call as AUTO takes it and, for Bicubic, with
        the node-record copy (NDI_LANEWISE2D_RECORDS=1) and with the plain node table (0); beside them the FORWARD
        ndi_interp2d_eval of the same handle on `rows` queries (the same number of output elements).  Alternating rounds,
        median of 7 after a warm-up, every call synchronised, best of the two rounds; the spread between the rounds; the
        fraction of the 8 TB/s spec on the compulsory bytes (two queries plus one output per element).  Batches: 1e7 rows,
        fewer where the rows are long (the output is kept to 512 MiB).
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR/<dtype>_<nx>x<ny>x<lanes> -- python tools/lanewise2d_rates.py --profile-shape <dtype> <nx> <ny> <lanes>
        one run per shape, a run of its own (tracing slows the host): REPS evaluations per class, query kind and form.
    python tools/lanewise2d_rates.py --merge DIR --out profiles/lanewise2d_rates.json
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
SHAPES = [(100, 100, 5), (2048, 2048, 8), (64, 64, 4096), (1000, 1000, 1)]
DTYPES = {"f64": np.float64, "f32": np.float32}
CLASSES = ("bilinear", "bicubic")
# form -> NDI_LANEWISE2D_RECORDS; None: unset (AUTO).  Bilinear has the one form.
FORMS = {"auto": None, "records": "1", "plain": "0"}
QUERIES = ("random", "broadcast")
REPS = 3
SPEC_TBPS = 8.0


def package():
    from __graft_entry__ import load_package
    return load_package()


def set_form(form):
    v = FORMS[form]
    if v is None:
        os.environ.pop("NDI_LANEWISE2D_RECORDS", None)
    else:
        os.environ["NDI_LANEWISE2D_RECORDS"] = v


def forms_of(cls):
    return tuple(FORMS) if cls == "bicubic" else ("auto",)


def handle(pkg, cls, dt, nx, ny, lanes):
    import torch
    rng = np.random.default_rng(nx + ny + lanes)
    x = np.cumsum(rng.uniform(0.5, 1.5, nx)).astype(dt)
    y = np.cumsum(rng.uniform(0.5, 1.5, ny)).astype(dt)
    tdt = torch.float64 if dt == np.float64 else torch.float32
    g = torch.Generator(device="cuda:0").manual_seed(2)
    zd = torch.randn((nx, ny, lanes), generator=g, device="cuda:0", dtype=tdt)
    strat = pkg.Bilinear.new() if cls == "bilinear" else pkg.Bicubic.new()
    it = pkg.Interp2D.builder(zd).x(torch.as_tensor(x, device="cuda:0")).y(torch.as_tensor(y, device="cuda:0")).strategy(strat).build()
    return x, y, it


def batch(x, y, dt, lanes):
    """(rows, {query kind: ((rows, lanes) x, (rows, lanes) y)}, the forward call's `rows` points, output), all on the device"""
    import torch
    rows = int(max(16384, min(10_000_000, (1 << 29) // (lanes * np.dtype(dt).itemsize))))
    tdt = torch.float64 if dt == np.float64 else torch.float32
    g = torch.Generator(device="cuda:0").manual_seed(1)

    def uniform(k, shape):
        lo, hi = float(k[0]), float(k[-1])
        return (lo + (hi - lo) * torch.rand(shape, generator=g, device="cuda:0", dtype=torch.float64)).to(tdt).clamp_(lo, hi)
    one = (uniform(x, (rows,)), uniform(y, (rows,)))
    q = {"random": (uniform(x, (rows, lanes)), uniform(y, (rows, lanes))),
         "broadcast": tuple(o[:, None].expand(rows, lanes).contiguous() for o in one)}
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
        for nx, ny, lanes in SHAPES:
            for cls in CLASSES:
                x, y, it = handle(pkg, cls, dt, nx, ny, lanes)
                rows, q, one, out = batch(x, y, dt, lanes)
                for kind in QUERIES:
                    key = f"{name}_{nx}x{ny}x{lanes}_{cls}_{kind}"
                    qx, qy = q[kind]

                    def lanewise(form):
                        def run():
                            set_form(form)
                            it.interp_lanewise_into(qx, qy, out, fresh=True)
                        return run
                    runs = {form: lanewise(form) for form in forms_of(cls)}
                    runs["forward"] = lambda: it.interp_array_into(one[0], one[1], out, fresh=True)
                    rounds = {k: [] for k in runs}
                    for _ in range(2):           # alternate the forms: other work shares the host
                        for k, fn in runs.items():
                            rounds[k].append(median_ms(fn))
                    ev = {"rows": rows}
                    for k, v in rounds.items():
                        ev[k] = {"ms": min(v), "rounds": v, "spread": abs(v[0] - v[1])}
                    ev["auto_over_forward"] = ev["auto"]["ms"] / ev["forward"]["ms"]
                    nbytes = 3 * rows * lanes * np.dtype(dt).itemsize
                    ev["compulsory_fraction_of_spec"] = nbytes / (ev["auto"]["ms"] * 1e-3) / (SPEC_TBPS * 1e12)
                    res["eval_ms"][key] = ev
                    print(key, json.dumps(ev), flush=True)
                set_form("auto")
                del it, q, one, out, qx, qy, runs
                torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump(res, open(out_path, "w"), indent=1)


def profile_shape(name, nx, ny, lanes):
    import torch
    pkg = package()
    dt = DTYPES[name]
    for cls in CLASSES:
        x, y, it = handle(pkg, cls, dt, nx, ny, lanes)
        rows, q, one, out = batch(x, y, dt, lanes)
        for kind in QUERIES:
            for form in forms_of(cls):
                if form == "auto" and cls == "bicubic":
                    continue
                set_form(form)
                for _ in range(REPS):
                    it.interp_lanewise_into(q[kind][0], q[kind][1], out, fresh=True)
        for _ in range(REPS):
            it.interp_array_into(one[0], one[1], out, fresh=True)
        torch.cuda.synchronize()
        del it, q, one, out
        torch.cuda.empty_cache()
    print("profiled", name, nx, ny, lanes, flush=True)


def merge(prof_dir, out_path):
    """per shape: mean time per launch of every lane-wise 2-D kernel instantiation over both query kinds (the instantiation's
    template arguments tell the class, the staging, the table layout and the orders)"""
    res = json.load(open(out_path)) if os.path.exists(out_path) else {}
    res["kernels_us_per_launch"] = {}
    for name in DTYPES:
        for nx, ny, lanes in SHAPES:
            key = f"{name}_{nx}x{ny}x{lanes}"
            files = glob.glob(os.path.join(prof_dir, key, "**", "*kernel_stats.csv"), recursive=True)
            if not files:
                continue
            entry = {}
            for row in csv.DictReader(open(files[0])):
                nm, t, calls = row["Name"], float(row["TotalDurationNs"]) / 1e3, int(row["Calls"])
                if "lanewise2d" in nm:
                    short = nm.split("(")[0].replace("void ", "").replace("ndi::", "")
                    entry[short] = {"us": t / calls, "calls": calls}
            res["kernels_us_per_launch"][key] = entry
            print(key, json.dumps(entry), flush=True)
    json.dump(res, open(out_path, "w"), indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lanewise2d_rates.json"))
    ap.add_argument("--profile-shape", nargs=4, metavar=("DTYPE", "NX", "NY", "LANES"))
    ap.add_argument("--merge", metavar="DIR")
    a = ap.parse_args()
    if a.profile_shape:
        profile_shape(a.profile_shape[0], *(int(v) for v in a.profile_shape[1:]))
    elif a.merge:
        merge(a.merge, a.out)
    else:
        timing_pass(a.out)
