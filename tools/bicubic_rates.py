"""Rates of the Bicubic strategy against Bilinear on the same shapes (output committed as
profiles/bicubic_rates.json).  Needs an MI355X; there is no CPU fallback.

    python tools/bicubic_rates.py --out profiles/bicubic_rates.json
        one process, device-resident inputs, median of 7 after a warm-up: `create` wall time (the call synchronises) and
        one evaluation batch into a device buffer, for Bicubic and for Bilinear (the baseline, measured here).
        Shapes: f32 and f64 at 100 x 100 x 1 and 100 x 100 x 5 (the reference's bench_interp2d grid), f32 2048 x 2048 x 64,
        f32 4096 x 4096 x 16; 1e7 queries each (fewer where the output would pass 16 GiB: noted per shape).
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR/<key> -- python tools/bicubic_rates.py --profile-shape <dtype> <nx> <ny> <C>
        one run per shape, a run of its own (tracing slows the host): REPS evaluations per strategy.
    python tools/bicubic_rates.py --merge DIR --out profiles/bicubic_rates.json
        adds the evaluation kernels' own times from those runs, the Bicubic / Bilinear ratio (expected from bytes: at most
        17 / 5 = 3.4 beyond the caches, nearer 1 on cache-resident grids) and the fraction of 8 TB/s on the
        17 Q C sizeof(T) compulsory bytes.

Partial-derivative handles (output committed as profiles/bicubic_partial_rates.json): the same three steps
with `--partial NUX,NUY` in each.  The timing pass then times the value handle and its partial handle of those orders side
by side (two alternating rounds each: their spread is the margin), the profiled run evaluates both, and the merge pairs the
two instances of eval_bicubic_kernel by their template arguments.  A partial reads the same sixteen operands and writes the
same row, so by bytes the ratio is 1.

Integral handles (output committed as profiles/bicubic_integral_rates.json): the same three steps with
`--integral` in each.  The timing pass times ndi_interp2d_antiderivative beside ndi_interp2d_create_bicubic, then an F batch
beside the value handle's and a rectangle batch beside the F batch (two alternating rounds each: the value handle's spread
is the margin); the profiled run evaluates all three, and the merge tells eval_bicubic_kernel, the F instance and the
rectangle instance of eval_bicubic_integral_kernel apart by their names.  By bytes F is 26 / 17 of the value (25 operands
and a store against 16 and a store); a rectangle is at most four times F's reads for one store.

The fused value-and-gradient call (output committed as profiles/bicubic_jet_rates.json): the same three steps
with `--jet ORDER` in each, on 4.13's four shapes in f32 and f64.  The timing pass runs alternating rounds of (a) ONE jet call
and (b) the K separate handle calls (the value handle and its K - 1 partial handles) into K buffers, all on device queries
and fresh device outputs, checks that (a) and (b) wrote the same bits at the timed size, and records the two rounds of each
(the ratio of (b)'s two rounds is the spread).  The profiled run does both again; the merge sums the K instances of
eval_bicubic_kernel against the one of eval_bicubic_jet_kernel, and writes their ratio beside the byte-model ratio
17 K / (16 + K), the jet's fraction of 8 TB/s on (16 + K) Q C sizeof(T) and whether the jet is below the separate calls by
more than the spread.  Both orders share the output file (one entry per order).
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
SHAPES = [("f32", 100, 100, 1), ("f64", 100, 100, 1), ("f32", 100, 100, 5), ("f64", 100, 100, 5),
          ("f32", 2048, 2048, 64), ("f32", 4096, 4096, 16)]
DTYPES = {"f64": np.float64, "f32": np.float32}
QUERIES = 10_000_000
REPS = 3
PEAK_BPS = 8.0e12    # HBM3E spec peak of the MI355X


def package():
    from __graft_entry__ import load_package
    return load_package()


def n_queries(dt, C):
    return int(min(QUERIES, (16 << 30) // (C * np.dtype(dt).itemsize)))


def inputs(name, nx, ny, C):
    import torch
    dt = DTYPES[name]
    rng = np.random.default_rng(nx + ny + C)
    x = np.cumsum(rng.uniform(0.5, 1.5, nx)).astype(dt)
    y = np.cumsum(rng.uniform(0.5, 1.5, ny)).astype(dt)
    tdt = torch.float32 if name == "f32" else torch.float64
    z = torch.rand((nx, ny, C), dtype=tdt, device="cuda:0")
    nq = n_queries(dt, C)
    qx = torch.as_tensor(rng.uniform(x[0], x[-1], nq).astype(dt), device="cuda:0")
    qy = torch.as_tensor(rng.uniform(y[0], y[-1], nq).astype(dt), device="cuda:0")
    out = torch.empty((nq, C), dtype=tdt, device="cuda:0")
    return torch.as_tensor(x, device="cuda:0"), torch.as_tensor(y, device="cuda:0"), z, qx, qy, out


def strategies(pkg):
    return {"Bilinear": pkg.Bilinear.new, "Bicubic": pkg.Bicubic.new}


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
    for name, nx, ny, C in SHAPES:
        key = f"{name}_{nx}x{ny}x{C}"
        x, y, z, qx, qy, out = inputs(name, nx, ny, C)
        res["create_ms"][key], res["eval_ms"][key] = {}, {"queries": int(qx.numel())}
        handles = {}
        for sname, new in strategies(pkg).items():
            def create():
                return pkg.Interp2DBuilder.new(z).x(x).y(y).strategy(new()).build()
            med, lo, hi = median_ms(create)
            res["create_ms"][key][sname] = {"median": med, "min": lo, "max": hi}
            handles[sname] = create()
        for rnd in range(2):               # alternate the two handles: other work shares the host
            for sname, h in handles.items():
                med, lo, hi = median_ms(lambda: h.interp_array_into(qx, qy, out))
                res["eval_ms"][key][f"{sname}_round{rnd}"] = {"median": med, "min": lo, "max": hi}
        print(key, json.dumps(res["create_ms"][key]), json.dumps(res["eval_ms"][key]), flush=True)
        del handles, x, y, z, qx, qy, out
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump(res, open(out_path, "w"), indent=1)


def orders_of(text):
    nux, nuy = (int(v) for v in text.split(","))
    assert 0 <= nux <= 2 and 0 <= nuy <= 2 and (nux, nuy) != (0, 0), "orders are 0, 1 or 2 per variable, not both 0"
    return nux, nuy


def partial_timing_pass(out_path, orders):
    import torch
    pkg = package()
    assert torch.cuda.is_available() and pkg.device_count() >= 1, "needs a GPU"
    res = {"device": torch.cuda.get_device_name(0), "orders": list(orders), "partial_create_ms": {}, "eval_ms": {}}
    for name, nx, ny, C in SHAPES:
        key = f"{name}_{nx}x{ny}x{C}"
        x, y, z, qx, qy, out = inputs(name, nx, ny, C)
        value = pkg.Interp2DBuilder.new(z).x(x).y(y).strategy(pkg.Bicubic.new()).build()
        med, lo, hi = median_ms(lambda: value.partial(*orders))
        res["partial_create_ms"][key] = {"median": med, "min": lo, "max": hi}
        handles = {"value": value, "partial": value.partial(*orders)}
        res["eval_ms"][key] = {"queries": int(qx.numel())}
        for rnd in range(2):               # alternate the two handles: the value handle's two rounds give the spread
            for sname, h in handles.items():
                med, lo, hi = median_ms(lambda: h.interp_array_into(qx, qy, out))
                res["eval_ms"][key][f"{sname}_round{rnd}"] = {"median": med, "min": lo, "max": hi}
        print(key, json.dumps(res["partial_create_ms"][key]), json.dumps(res["eval_ms"][key]), flush=True)
        del handles, value, x, y, z, qx, qy, out
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump(res, open(out_path, "w"), indent=1)


def partial_profile_shape(name, nx, ny, C, orders):
    pkg = package()
    x, y, z, qx, qy, out = inputs(name, nx, ny, C)
    value = pkg.Interp2DBuilder.new(z).x(x).y(y).strategy(pkg.Bicubic.new()).build()
    for h in (value, value.partial(*orders)):
        for _ in range(REPS):
            h.interp_array_into(qx, qy, out)
    print("profiled", name, nx, ny, C, "partial", orders, flush=True)


def partial_merge(prof_dir, out_path, orders):
    """value / partial pairs of eval_bicubic_kernel<T, VEC, KLDS, TB, NUX, NUY> by the last two template arguments"""
    res = json.load(open(out_path)) if os.path.exists(out_path) else {}
    res["orders"] = list(orders)
    res["eval_kernels"] = {}
    tails = {"value": ", 0, 0>", "partial": f", {orders[0]}, {orders[1]}>"}
    for name, nx, ny, C in SHAPES:
        key = f"{name}_{nx}x{ny}x{C}"
        files = glob.glob(os.path.join(prof_dir, key, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            continue
        per, names = {"value": 0.0, "partial": 0.0}, {"value": [], "partial": []}
        for row in csv.DictReader(open(files[0])):
            kn = row["Name"].split("(")[0].strip()
            if "eval_bicubic_kernel" not in kn:
                continue
            for who, tail in tails.items():
                if kn.endswith(tail):
                    per[who] += float(row["TotalDurationNs"]) / REPS
                    names[who].append(kn)
        nq, size = n_queries(DTYPES[name], C), np.dtype(DTYPES[name]).itemsize
        entry = {"queries": nq, "compulsory_bytes": 17 * nq * C * size}
        for who, ns in per.items():
            entry[who] = {"kernel_ms_per_batch": ns / 1e6, "kernels": sorted(set(names[who]))}
        if per["value"] > 0 and per["partial"] > 0:
            entry["ratio_partial_over_value"] = per["partial"] / per["value"]
            entry["partial_fraction_of_8TBps"] = entry["compulsory_bytes"] / (per["partial"] * 1e-9) / PEAK_BPS
        res["eval_kernels"][key] = entry
        print(key, json.dumps(entry), flush=True)
    json.dump(res, open(out_path, "w"), indent=1)


def integral_inputs(name, nx, ny, C):
    """the value handle, its integral handle, the four bounds of the rectangle batch (the queries against a rolled copy)"""
    import torch
    pkg = package()
    x, y, z, qx, qy, out = inputs(name, nx, ny, C)
    value = pkg.Interp2DBuilder.new(z).x(x).y(y).strategy(pkg.Bicubic.new()).build()
    return pkg, x, y, z, value, (qx, torch.roll(qx, 1), qy, torch.roll(qy, 1)), out


def integral_timing_pass(out_path):
    import torch
    pkg = package()
    assert torch.cuda.is_available() and pkg.device_count() >= 1, "needs a GPU"
    res = {"device": torch.cuda.get_device_name(0), "create_ms": {}, "eval_ms": {}}
    for name, nx, ny, C in SHAPES:
        key = f"{name}_{nx}x{ny}x{C}"
        pkg, x, y, z, value, r, out = integral_inputs(name, nx, ny, C)
        res["create_ms"][key] = {}
        for what, fn in (("create_bicubic", lambda: pkg.Interp2DBuilder.new(z).x(x).y(y).strategy(pkg.Bicubic.new()).build()),
                         ("antiderivative", lambda: value.antiderivative())):
            med, lo, hi = median_ms(fn, reps=5)
            res["create_ms"][key][what] = {"median": med, "min": lo, "max": hi}
        F = value.antiderivative()
        calls = {"value": lambda: value.interp_array_into(r[0], r[2], out), "F": lambda: F.interp_array_into(r[0], r[2], out),
                 "rectangle": lambda: F.strategy.integral(*r, out)}
        res["eval_ms"][key] = {"queries": int(r[0].numel())}
        for rnd in range(2):               # alternate the three: the value handle's two rounds give the spread
            for what, fn in calls.items():
                med, lo, hi = median_ms(fn)
                res["eval_ms"][key][f"{what}_round{rnd}"] = {"median": med, "min": lo, "max": hi}
        print(key, json.dumps(res["create_ms"][key]), json.dumps(res["eval_ms"][key]), flush=True)
        del F, value, calls, x, y, z, r, out
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump(res, open(out_path, "w"), indent=1)


def integral_profile_shape(name, nx, ny, C):
    pkg, x, y, z, value, r, out = integral_inputs(name, nx, ny, C)
    F = value.antiderivative()
    for fn in (lambda: value.interp_array_into(r[0], r[2], out), lambda: F.interp_array_into(r[0], r[2], out),
               lambda: F.strategy.integral(*r, out)):
        for _ in range(REPS):
            fn()
    print("profiled", name, nx, ny, C, "integral", flush=True)


def integral_merge(prof_dir, out_path):
    """eval_bicubic_kernel<..., 0, 0> (value), eval_bicubic_integral_kernel<..., false> (F) and <..., true> (rectangle)"""
    res = json.load(open(out_path)) if os.path.exists(out_path) else {}
    res["eval_kernels"] = {}
    for name, nx, ny, C in SHAPES:
        key = f"{name}_{nx}x{ny}x{C}"
        files = glob.glob(os.path.join(prof_dir, key, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            continue
        per, names = {"value": 0.0, "F": 0.0, "rectangle": 0.0}, {"value": [], "F": [], "rectangle": []}
        for row in csv.DictReader(open(files[0])):
            kn = row["Name"].split("(")[0].strip()
            if "eval_bicubic_integral_kernel" in kn:
                who = "rectangle" if kn.endswith(", true>") else "F"
            elif "eval_bicubic_kernel" in kn and kn.endswith(", 0, 0>"):
                who = "value"
            else:
                continue                 # range pre-passes, builds, fills
            per[who] += float(row["TotalDurationNs"]) / REPS
            names[who].append(kn)
        nq, size = n_queries(DTYPES[name], C), np.dtype(DTYPES[name]).itemsize
        entry = {"queries": nq, "compulsory_bytes_value": 17 * nq * C * size, "compulsory_bytes_F": 26 * nq * C * size}
        for who, ns in per.items():
            entry[who] = {"kernel_ms_per_batch": ns / 1e6, "kernels": sorted(set(names[who]))}
        if per["value"] > 0 and per["F"] > 0 and per["rectangle"] > 0:
            entry["ratio_F_over_value"] = per["F"] / per["value"]
            entry["ratio_rectangle_over_F"] = per["rectangle"] / per["F"]
            entry["F_fraction_of_8TBps"] = entry["compulsory_bytes_F"] / (per["F"] * 1e-9) / PEAK_BPS
        res["eval_kernels"][key] = entry
        print(key, json.dumps(entry), flush=True)
    json.dump(res, open(out_path, "w"), indent=1)


JET_SHAPES = [(name, nx, ny, C) for nx, ny, C in ((100, 100, 1), (100, 100, 5), (2048, 2048, 64), (4096, 4096, 16))
              for name in ("f32", "f64")]
JET_BEYOND_CACHE = ((2048, 2048, 64), (4096, 4096, 16))     # where 4.13 expects the operand loads to bound the kernel


def jet_queries(dt, C):
    """enough queries that one jet call moves about 24 GB by the byte model (3 ms at 8 TB/s), between 1e6 and 4e7"""
    return int(min(40_000_000, max(1_000_000, 24e9 // (19 * C * np.dtype(dt).itemsize))))


def jet_setup(name, nx, ny, C, order):
    """the value handle and its partial handles in the order of JET_PARTS, device queries, a planar jet buffer (K, nq, C) and
    K separate buffers"""
    import torch
    pkg = package()
    dt = DTYPES[name]
    tdt = torch.float32 if name == "f32" else torch.float64
    rng = np.random.default_rng(nx + ny + C)
    x = np.cumsum(rng.uniform(0.5, 1.5, nx)).astype(dt)
    y = np.cumsum(rng.uniform(0.5, 1.5, ny)).astype(dt)
    gen = torch.Generator(device="cuda:0").manual_seed(nx + ny + C)
    z = torch.rand((nx, ny, C), dtype=tdt, device="cuda:0", generator=gen)
    nq = jet_queries(dt, C)
    span = lambda k: (float(k[0]) + (float(k[-1]) - float(k[0])) * torch.rand(nq, dtype=torch.float64, device="cuda:0",  # noqa: E731
                                                                             generator=gen)).to(tdt).clamp(float(k[0]), float(k[-1]))
    qx, qy = span(x), span(y)
    value = pkg.Interp2DBuilder.new(z).x(torch.as_tensor(x, device="cuda:0")).y(torch.as_tensor(y, device="cuda:0")) \
        .strategy(pkg.Bicubic.new()).build()
    handles = [value if nu == (0, 0) else value.partial(*nu) for nu in pkg.JET_PARTS[order]]
    K = len(handles)
    jet = torch.empty((K, nq, C), dtype=tdt, device="cuda:0")
    sep = [torch.empty((nq, C), dtype=tdt, device="cuda:0") for _ in range(K)]
    parts = [jet[k] for k in range(K)]

    def run_jet():
        value.strategy.jet_into(qx, qy, parts, order=order, fresh=True)

    def run_separate():
        for h, buf in zip(handles, sep):
            h.interp_array_into(qx, qy, buf, fresh=True)
    return dict(nq=nq, K=K, jet=jet, sep=sep, run_jet=run_jet, run_separate=run_separate)


def jet_timing_pass(out_path, order):
    import torch
    pkg = package()
    assert torch.cuda.is_available() and pkg.device_count() >= 1, "needs a GPU"
    res = json.load(open(out_path)) if os.path.exists(out_path) else {}
    res["device"] = torch.cuda.get_device_name(0)
    mine = res.setdefault(f"order_{order}", {})
    mine["parts"] = [list(nu) for nu in pkg.JET_PARTS[order]]
    mine["eval_ms"] = {}
    for name, nx, ny, C in JET_SHAPES:
        key = f"{name}_{nx}x{ny}x{C}"
        s = jet_setup(name, nx, ny, C, order)
        entry = {"queries": s["nq"]}
        for rnd in range(2):               # alternate the two: the separate calls' two rounds give the spread
            for what, fn in (("jet", s["run_jet"]), ("separate", s["run_separate"])):
                med, lo, hi = median_ms(fn)
                entry[f"{what}_round{rnd}"] = {"median": med, "min": lo, "max": hi}
        bits = torch.int32 if name == "f32" else torch.int64
        entry["bit_equal_parts"] = [bool(torch.equal(s["jet"][k].view(bits), s["sep"][k].view(bits))) for k in range(s["K"])]
        entry["wall_ratio_separate_over_jet"] = entry["separate_round1"]["median"] / entry["jet_round1"]["median"]
        entry["spread_of_separate_rounds"] = entry["separate_round0"]["median"] / entry["separate_round1"]["median"]
        mine["eval_ms"][key] = entry
        print(key, json.dumps(entry), flush=True)
        del s
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump(res, open(out_path, "w"), indent=1)


def jet_profile_shape(name, nx, ny, C, order):
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    s = jet_setup(name, nx, ny, C, order)
    for fn in (s["run_jet"], s["run_separate"]):
        for _ in range(REPS):
            fn()
    torch.cuda.synchronize()
    print("profiled", name, nx, ny, C, "jet", order, flush=True)


def jet_merge(prof_dir, out_path, order):
    """eval_bicubic_jet_kernel<..., ORDER> (one launch per batch) against the K instances eval_bicubic_kernel<..., NUX, NUY>"""
    res = json.load(open(out_path)) if os.path.exists(out_path) else {}
    mine = res.setdefault(f"order_{order}", {})
    mine["eval_kernels"] = {}
    K = 3 if order == 1 else 6
    for name, nx, ny, C in JET_SHAPES:
        key = f"{name}_{nx}x{ny}x{C}"
        files = glob.glob(os.path.join(prof_dir, key, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            continue
        per, names = {"jet": 0.0, "separate": 0.0}, {"jet": [], "separate": []}
        for row in csv.DictReader(open(files[0])):
            kn = row["Name"].split("(")[0].strip()
            if "eval_bicubic_jet_kernel" in kn:
                who = "jet"
            elif "eval_bicubic_kernel" in kn:
                who = "separate"
            else:
                continue                 # builds, fills
            per[who] += float(row["TotalDurationNs"]) / REPS
            names[who].append(kn)
        nq, size = jet_queries(DTYPES[name], C), np.dtype(DTYPES[name]).itemsize
        entry = {"queries": nq, "compulsory_bytes_jet": (16 + K) * nq * C * size, "byte_model_ratio": 17 * K / (16 + K),
                 "beyond_cache": (nx, ny, C) in JET_BEYOND_CACHE}
        for who, ns in per.items():
            entry[who] = {"kernel_ms_per_batch": ns / 1e6, "kernels": sorted(set(names[who]))}
        wall = mine.get("eval_ms", {}).get(key)
        if per["jet"] > 0 and per["separate"] > 0:
            entry["ratio_separate_over_jet"] = per["separate"] / per["jet"]
            entry["jet_fraction_of_8TBps"] = entry["compulsory_bytes_jet"] / (per["jet"] * 1e-9) / PEAK_BPS
            if wall:
                spread = abs(wall["spread_of_separate_rounds"] - 1.0)
                entry["spread_of_separate_rounds"] = wall["spread_of_separate_rounds"]
                entry["jet_below_separate_by_more_than_the_spread"] = bool(per["jet"] < per["separate"] * (1.0 - spread))
        mine["eval_kernels"][key] = entry
        print(key, json.dumps(entry), flush=True)
    json.dump(res, open(out_path, "w"), indent=1)


def profile_shape(name, nx, ny, C):
    pkg = package()
    x, y, z, qx, qy, out = inputs(name, nx, ny, C)
    for sname, new in strategies(pkg).items():
        h = pkg.Interp2DBuilder.new(z).x(x).y(y).strategy(new()).build()
        for _ in range(REPS):
            h.interp_array_into(qx, qy, out)
    print("profiled", name, nx, ny, C, flush=True)


def merge(prof_dir, out_path):
    res = json.load(open(out_path)) if os.path.exists(out_path) else {}
    res["eval_kernels"] = {}
    for name, nx, ny, C in SHAPES:
        key = f"{name}_{nx}x{ny}x{C}"
        files = glob.glob(os.path.join(prof_dir, key, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            continue
        per, names = {"Bilinear": 0.0, "Bicubic": 0.0}, {"Bilinear": [], "Bicubic": []}
        for row in csv.DictReader(open(files[0])):
            kn, total = row["Name"], float(row["TotalDurationNs"])
            if "eval_bicubic_kernel" in kn:
                who = "Bicubic"
            elif "eval_" in kn and "2d" in kn or "eval_bilinear" in kn:
                who = "Bilinear"
            else:
                who = None               # range pre-passes, builds, fills
            if who:
                per[who] += total / REPS
                names[who].append(kn.split("(")[0])
        nq, size = n_queries(DTYPES[name], C), np.dtype(DTYPES[name]).itemsize
        entry = {"queries": nq, "compulsory_bytes_bicubic": 17 * nq * C * size}
        for who, ns in per.items():
            entry[who] = {"kernel_ms_per_batch": ns / 1e6, "kernels": sorted(set(names[who]))}
        if per["Bilinear"] > 0 and per["Bicubic"] > 0:
            entry["ratio_bicubic_over_bilinear"] = per["Bicubic"] / per["Bilinear"]
            entry["bicubic_fraction_of_8TBps"] = entry["compulsory_bytes_bicubic"] / (per["Bicubic"] * 1e-9) / PEAK_BPS
        res["eval_kernels"][key] = entry
        print(key, json.dumps(entry), flush=True)
    json.dump(res, open(out_path, "w"), indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--partial", metavar="NUX,NUY", type=orders_of,
                    help="time a partial-derivative handle of these orders beside the value handle")
    ap.add_argument("--integral", action="store_true", help="time the integral handle beside the value handle")
    ap.add_argument("--jet", metavar="ORDER", type=int, choices=(1, 2),
                    help="time one fused jet call of this order beside the K separate handle calls")
    ap.add_argument("--profile-shape", nargs=4, metavar=("DTYPE", "NX", "NY", "C"))
    ap.add_argument("--merge", metavar="DIR")
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "bicubic_jet_rates.json" if a.jet else
                             "bicubic_integral_rates.json" if a.integral else
                             "bicubic_partial_rates.json" if a.partial else "bicubic_rates.json")
    if a.jet and a.profile_shape:
        jet_profile_shape(a.profile_shape[0], *(int(v) for v in a.profile_shape[1:]), a.jet)
    elif a.jet and a.merge:
        jet_merge(a.merge, a.out, a.jet)
    elif a.jet:
        jet_timing_pass(a.out, a.jet)
    elif a.integral and a.profile_shape:
        integral_profile_shape(a.profile_shape[0], *(int(v) for v in a.profile_shape[1:]))
    elif a.integral and a.merge:
        integral_merge(a.merge, a.out)
    elif a.integral:
        integral_timing_pass(a.out)
    elif a.partial and a.profile_shape:
        partial_profile_shape(a.profile_shape[0], *(int(v) for v in a.profile_shape[1:]), a.partial)
    elif a.partial and a.merge:
        partial_merge(a.merge, a.out, a.partial)
    elif a.partial:
        partial_timing_pass(a.out, a.partial)
    elif a.profile_shape:
        profile_shape(a.profile_shape[0], *(int(v) for v in a.profile_shape[1:]))
    elif a.merge:
        merge(a.merge, a.out)
    else:
        timing_pass(a.out)
