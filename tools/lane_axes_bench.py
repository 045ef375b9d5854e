"""Table layout of the lane-axes evaluation (output committed as profiles/lane_axes_layout.json).  Needs an
MI355X; there is no CPU fallback.

After its search a cubic element of a lane-axes handle reads x, y of rows i and i+1 and a, b of row i: six element reads
from four tables that lie `lanes` elements apart (NDI_LANE_AXES_RECORDS=0, "plain"), or two aligned 16- / 32-byte loads from
the record copy R[i][l] = {x, y, a, b} (NDI_LANE_AXES_RECORDS=1, "records").  This measures one against the other:

    python tools/lane_axes_bench.py --out profiles/lane_axes_layout.json

Shapes: many lanes with few knots (16 x 4096), few lanes with many knots (65536 x 4) and one between (1024 x 64); f32 and
f64; queries broadcast along the lanes (ndi_interp1d_eval on nq queries) and per lane (ndi_interp1d_eval_lanewise on
nq x lanes), nq x lanes = 2^24 output elements, device buffers in and out, the kernel's own range test (no pre-pass).
Beside them, as context, the shared-axis eval_lanewise_kernel (AUTO) of a Pchip handle at the same nq x lanes.

Protocol: the variants alternate within one process, ROUNDS rounds; in a round every variant is warmed up (code objects, the
record copy) and then launched REPS times, each launch timed with a pair of device events around the library call; a
variant's figure is the median over all its launches, its spread the distance between its lowest and highest ROUND median.
`records` wins a case only when its median is below `plain`'s by more than the larger of the two spreads.
"""
import argparse
import json
import os
import sys

import numpy as np

os.environ["NDI_TUNE_LIVE"] = "1"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = [(16, 4096), (1024, 64), (65536, 4)]
DTYPES = {"f64": np.float64, "f32": np.float32}
ELEMENTS = 1 << 24
ROUNDS, REPS = 5, 10


def package():
    from __graft_entry__ import load_package
    return load_package()


def tables(n, lanes, dt):
    rng = np.random.default_rng(n + lanes)
    x = np.cumsum(rng.uniform(0.5, 1.5, (n, lanes)), axis=0)
    x -= x[0] * rng.uniform(0.0, 1.0, lanes)          # every lane starts and ends somewhere else
    return x.astype(dt), rng.normal(size=(n, lanes)).astype(dt)


def timed(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def measure(variants):
    """{name: callable} -> {name: {median_ms, spread_ms, round_medians_ms}}, the variants alternating round by round"""
    import torch
    samples = {k: [] for k in variants}
    for _ in range(ROUNDS):
        for k, fn in variants.items():
            fn()
            fn()
            torch.cuda.synchronize()
            samples[k].append([timed(fn) for _ in range(REPS)])
    out = {}
    for k, rounds in samples.items():
        meds = [float(np.median(r)) for r in rounds]
        out[k] = {"median_ms": float(np.median(np.concatenate(rounds))), "spread_ms": max(meds) - min(meds), "round_medians_ms": meds}
    return out


def main(out_path, shapes):
    import torch
    pkg = package()
    assert torch.cuda.is_available() and pkg.device_count() >= 1, "needs a GPU"
    res = {"device": torch.cuda.get_device_name(0), "elements": ELEMENTS, "rounds": ROUNDS, "reps": REPS, "cases": {}}
    for name, dt in DTYPES.items():
        tdt = torch.float64 if dt == np.float64 else torch.float32
        for n, lanes in shapes:
            x, y = tables(n, lanes, dt)
            tx, ty = torch.as_tensor(x, device="cuda:0"), torch.as_tensor(y, device="cuda:0")
            it = pkg.Interp1D.builder(ty).lane_axes(tx).strategy(pkg.Pchip.new()).build()
            shared = pkg.Interp1D.builder(ty).x(torch.as_tensor(np.ascontiguousarray(x[:, 0]), device="cuda:0")).strategy(pkg.Pchip.new()).build()
            nq = ELEMENTS // lanes
            lo, hi = float(x[0].max()), float(x[-1].min())
            g = torch.Generator(device="cuda:0").manual_seed(1)
            one = (lo + (hi - lo) * torch.rand((nq,), generator=g, device="cuda:0", dtype=torch.float64)).to(tdt).clamp_(lo, hi)
            q = {"broadcast": one[:, None].expand(nq, lanes).contiguous(),
                 "per_lane": (lo + (hi - lo) * torch.rand((nq, lanes), generator=g, device="cuda:0", dtype=torch.float64)).to(tdt).clamp_(lo, hi)}
            s0, s1 = float(x[0, 0]), float(x[-1, 0])
            qs = (s0 + (s1 - s0) * torch.rand((nq, lanes), generator=g, device="cuda:0", dtype=torch.float64)).to(tdt).clamp_(s0, s1)
            out = torch.empty((nq, lanes), dtype=tdt, device="cuda:0")

            def form(records, fn):
                def run():
                    os.environ["NDI_LANE_AXES_RECORDS"] = records
                    fn()
                return run
            for kind in ("broadcast", "per_lane"):
                call = (lambda: it.interp_array_into(one, out, fresh=True)) if kind == "broadcast" else \
                    (lambda: it.interp_lanewise_into(q["per_lane"], out, fresh=True))
                ev = measure({"plain": form("0", call), "records": form("1", call),
                              "shared_axis_lanewise": lambda: shared.interp_lanewise_into(q["broadcast"] if kind == "broadcast" else qs,
                                                                                          out, fresh=True)})
                bar = max(ev["plain"]["spread_ms"], ev["records"]["spread_ms"])
                ev["records_win"] = bool(ev["plain"]["median_ms"] - ev["records"]["median_ms"] > bar)
                ev["nq"] = nq
                key = f"{name}_{n}x{lanes}_{kind}"
                res["cases"][key] = ev
                print(key, json.dumps(ev), flush=True)
            os.environ.pop("NDI_LANE_AXES_RECORDS", None)
            del it, shared, q, qs, one, out, tx, ty
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump(res, open(out_path, "w"), indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lane_axes_layout.json"))
    ap.add_argument("--shape", nargs=2, type=int, action="append", metavar=("N", "LANES"), help="instead of the built-in shapes")
    a = ap.parse_args()
    main(a.out, [tuple(s) for s in a.shape] if a.shape else SHAPES)
