"""Rates of the Tricubic build and evaluation kernel (output committed as profiles/tricubic_rates.json).
Needs an MI355X; there is no CPU fallback.

    python tools/tricubic_bench.py --out profiles/tricubic_rates.json

Cases (tools/trilinear_bench.py's), 2^22 queries each, device buffers in and out, NDI_EVAL_FRESH_OUTPUT (the kernel's own
range test, no pre-pass):
    64^3 x 256 f32        wide rows
    256^3 x 4 f32, f64    short rows
    100^3 x 1 f64         a scalar table
each with the axes staged in LDS against bisected in global memory (NDI_TRICUBIC_STAGE 1 / 0) and 16-byte vectors against
single elements (NDI_TRICUBIC_VEC -1 / 1; scalar data has the one form), and next to them Trilinear's AUTO plan on the same
grid, queries and output buffer: the Tricubic / Trilinear time ratio, to be read against the operand ratio 64 / 8.

Protocol (tools/trilinear_bench.py's): the variants alternate within one process, ROUNDS rounds; in a round every variant is
warmed up twice and then launched REPS times, each launch timed with a pair of device events around the library call; a
variant's figure is the median over all its launches, its spread the distance between its lowest and highest ROUND median.
Create time: the host clock around Interp3D...build() on device tensors (the call returns with the table complete), the
median of CREATES builds after one warm-up, each handle released before the next.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

os.environ["NDI_TUNE_LIVE"] = "1"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from trilinear_bench import CASES, NQ, REPS, ROUNDS, measure, package  # noqa: E402

CREATES = 3


def create_time(build):
    import torch
    build().strategy.release()
    times = []
    for _ in range(CREATES):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        it = build()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
        it.strategy.release()
    return float(np.median(times)), times


def main(out_path, nq, only):
    import torch
    pkg = package()
    assert torch.cuda.is_available() and pkg.device_count() >= 1, "needs a GPU"
    res = {"device": torch.cuda.get_device_name(0), "queries": nq, "rounds": ROUNDS, "reps": REPS, "creates": CREATES,
           "operand_ratio": 64 / 8, "cases": {}}
    for name, dt, n, lanes in CASES:
        if only and name not in only:
            continue
        tdt = torch.float64 if dt == np.float64 else torch.float32
        g = torch.Generator(device="cuda:0").manual_seed(1)
        axes = [torch.cumsum(0.5 + torch.rand((n,), generator=g, device="cuda:0", dtype=torch.float64), 0).to(tdt) for _ in range(3)]
        data = torch.rand((n, n, n, lanes), generator=g, device="cuda:0", dtype=tdt)

        def build(strategy):
            return lambda: pkg.Interp3D.builder(data).x(axes[0]).y(axes[1]).z(axes[2]).strategy(strategy()).build()
        case = {"create_ms": {}}
        for label, strategy in (("tricubic", pkg.Tricubic.new), ("trilinear", pkg.Trilinear.new)):
            med, all_ = create_time(build(strategy))
            case["create_ms"][label] = {"median_ms": med, "samples_ms": all_}
        cubic, linear = build(pkg.Tricubic.new)(), build(pkg.Trilinear.new)()
        q = []
        for k in axes:
            lo, hi = float(k[0]), float(k[-1])
            q.append((lo + (hi - lo) * torch.rand((nq,), generator=g, device="cuda:0", dtype=torch.float64)).to(tdt).clamp_(lo, hi))
        out = torch.empty((nq, lanes), dtype=tdt, device="cuda:0")

        def form(stage, vec):
            def run():
                os.environ["NDI_TRICUBIC_STAGE"] = stage
                os.environ["NDI_TRICUBIC_VEC"] = vec
                cubic.interp_array_into(*q, out, fresh=True)
            return run
        wide = lanes % (16 // np.dtype(dt).itemsize) == 0
        variants = {f"stage{s}_{'wide' if v == '-1' else 'scalar'}": form(s, v)
                    for s in ("1", "0") for v in (("-1", "1") if wide else ("1",))}
        variants["trilinear_auto"] = lambda: linear.interp_array_into(*q, out, fresh=True)
        ev = measure(variants)
        nbytes = nq * (lanes + 3) * np.dtype(dt).itemsize
        for v in ev.values():
            v["gqueries_per_s"] = nq / v["median_ms"] / 1e6
            v["gbytes_per_s"] = nbytes / v["median_ms"] / 1e6
        auto = "stage1_wide" if wide else "stage1_scalar"
        case["eval"] = ev
        case["auto_plan"] = auto
        case["tricubic_over_trilinear"] = ev[auto]["median_ms"] / ev["trilinear_auto"]["median_ms"]
        res["cases"][name] = case
        print(name, json.dumps(case), flush=True)
        os.environ.pop("NDI_TRICUBIC_STAGE", None)
        os.environ.pop("NDI_TRICUBIC_VEC", None)
        cubic.strategy.release()
        linear.strategy.release()
        del cubic, linear, data, q, out
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump(res, open(out_path, "w"), indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tricubic_rates.json"))
    ap.add_argument("--queries", type=int, default=NQ)
    ap.add_argument("--case", action="append", help="instead of all cases")
    a = ap.parse_args()
    main(a.out, a.queries, a.case)
