"""Build time of a Bicubic handle by where its node derivatives come from: the spline (ndi_interp2d_create_bicubic: three
Thomas solves, two transposed copies, one pack) against the local rules (ndi_interp2d_create_bicubic_local: a two-launch
stencil into the node table).  DESIGN.md 4.17; output committed as profiles/bicubic_local_build_times.json.  Needs an
MI355X; there is no CPU fallback.

    python tools/bicubic_build_times.py --out profiles/bicubic_local_build_times.json [--label NAME]
        (a run is appended to the file's "runs" when the file exists)

One process, device-resident inputs (so no upload is timed), f64 and f32 at 1024 x 1024 x 1 and 100 x 100 x 5.  `create`
synchronises before it returns, so a host clock around the call is the build's wall time.  Per shape: a warm-up of every
strategy, then ROUNDS rounds that alternate the strategies (a create, then the release of the handle outside the timed
window); the figure is the median, the quartiles are its spread.  A package without the local rules (an older commit) is
timed on the spline alone, which is how the spline figure of the commit before this feature was taken: run the same file
on that checkout with `--root`, and on this one with `--strategies spline` for a like-for-like loop (the creates of the
other strategies between two spline creates change what the allocator hands out).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

SHAPES = [(1024, 1024, 1), (100, 100, 5)]
DTYPES = {"f64": np.float64, "f32": np.float32}
WARMUP, ROUNDS = 5, 41


def package(root):
    sys.path.insert(0, root)
    from __graft_entry__ import load_package
    return load_package()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--label", default="this commit")
    ap.add_argument("--strategies", default="spline,pchip,akima",
                    help="the strategies to alternate (spline alone compares two commits like for like)")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="the checkout whose package is timed (default: this file's)")
    args = ap.parse_args()
    import torch
    pkg = package(args.root)
    assert torch.cuda.is_available() and pkg.device_count() > 0, "needs a GPU: there is no CPU fallback"
    makers = {"spline": pkg.Bicubic.new}
    if hasattr(pkg.Bicubic, "pchip"):
        makers.update(pchip=pkg.Bicubic.pchip, akima=pkg.Bicubic.akima)
    makers = {k: v for k, v in makers.items() if k in args.strategies.split(",")}
    assert makers, f"no strategy of {args.strategies!r} in this package"
    result = {"label": args.label, "strategies": list(makers), "device": torch.cuda.get_device_name(0), "warmup": WARMUP, "rounds": ROUNDS,
              "unit": "ms per create (device-resident inputs; the call synchronises)", "shapes": {}}
    for name, dt in DTYPES.items():
        for nx, ny, C in SHAPES:
            rng = np.random.default_rng(nx + ny + C)
            x = torch.as_tensor(np.cumsum(rng.uniform(0.5, 1.5, nx)).astype(dt), device="cuda:0")
            y = torch.as_tensor(np.cumsum(rng.uniform(0.5, 1.5, ny)).astype(dt), device="cuda:0")
            z = torch.as_tensor(rng.normal(size=(nx, ny, C)).astype(dt), device="cuda:0")
            builder = pkg.Interp2DBuilder.new(z).x(x).y(y)

            def create(make):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                it = builder.strategy(make()).build()
                t1 = time.perf_counter()
                it.strategy.release()
                return (t1 - t0) * 1e3
            for _ in range(WARMUP):
                for make in makers.values():
                    create(make)
            times = {k: [] for k in makers}
            for _ in range(ROUNDS):
                for k, make in makers.items():
                    times[k].append(create(make))
            entry = {}
            for k, v in times.items():
                q1, med, q3 = np.percentile(v, [25, 50, 75])
                entry[k] = {"median_ms": round(float(med), 4), "q1_ms": round(float(q1), 4), "q3_ms": round(float(q3), 4)}
            result["shapes"][f"{name} {nx}x{ny}x{C}"] = entry
            print(f"{name} {nx}x{ny}x{C}: " + "  ".join(f"{k} {e['median_ms']:.3f} ms" for k, e in entry.items()), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    runs = json.load(open(args.out))["runs"] if os.path.exists(args.out) else []     # one file collects the runs of a visit
    with open(args.out, "w") as f:
        json.dump({"runs": runs + [result]}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
