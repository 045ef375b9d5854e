"""Rates of the Trilinear evaluation kernel (output committed as profiles/trilinear_rates.json).  Needs an
MI355X; there is no CPU fallback.

    python tools/trilinear_bench.py --out profiles/trilinear_rates.json

Cases, 2^22 queries each, device buffers in and out, NDI_EVAL_FRESH_OUTPUT (the kernel's own range test, no pre-pass):
    64^3 x 256 f32        wide rows: the store stream should bound it
    256^3 x 4 f32, f64    short rows: the corner gather should bound it
    100^3 x 1 f64         a scalar table
each with the axes staged in LDS against bisected in global memory (NDI_TRILINEAR_STAGE 1 / 0) and 16-byte vectors against
single elements (NDI_TRILINEAR_VEC -1 / 1; scalar data has the one form).

Protocol (tools/lane_axes_bench.py's): the variants alternate within one process, ROUNDS rounds; in a round every variant is
warmed up twice and then launched REPS times, each launch timed with a pair of device events around the library call; a
variant's figure is the median over all its launches, its spread the distance between its lowest and highest ROUND median.
GB/s counts the output rows written plus the three query arrays read -- the compulsory traffic, not the corner reads.
"""
import argparse
import json
import os
import sys

import numpy as np

os.environ["NDI_TUNE_LIVE"] = "1"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CASES = [("f32_64x64x64x256", np.float32, 64, 256), ("f32_256x256x256x4", np.float32, 256, 4),
         ("f64_256x256x256x4", np.float64, 256, 4), ("f64_100x100x100x1", np.float64, 100, 1)]
NQ = 1 << 22
ROUNDS, REPS = 5, 10


def package():
    from __graft_entry__ import load_package
    return load_package()


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


def main(out_path, nq, only):
    import torch
    pkg = package()
    assert torch.cuda.is_available() and pkg.device_count() >= 1, "needs a GPU"
    res = {"device": torch.cuda.get_device_name(0), "queries": nq, "rounds": ROUNDS, "reps": REPS, "cases": {}}
    for name, dt, n, lanes in CASES:
        if only and name not in only:
            continue
        tdt = torch.float64 if dt == np.float64 else torch.float32
        g = torch.Generator(device="cuda:0").manual_seed(1)
        axes = [torch.cumsum(0.5 + torch.rand((n,), generator=g, device="cuda:0", dtype=torch.float64), 0).to(tdt) for _ in range(3)]
        data = torch.rand((n, n, n, lanes), generator=g, device="cuda:0", dtype=tdt)
        it = pkg.Interp3D.builder(data).x(axes[0]).y(axes[1]).z(axes[2]).strategy(pkg.Trilinear.new()).build()
        q = []
        for k in axes:
            lo, hi = float(k[0]), float(k[-1])
            q.append((lo + (hi - lo) * torch.rand((nq,), generator=g, device="cuda:0", dtype=torch.float64)).to(tdt).clamp_(lo, hi))
        out = torch.empty((nq, lanes), dtype=tdt, device="cuda:0")

        def form(stage, vec):
            def run():
                os.environ["NDI_TRILINEAR_STAGE"] = stage
                os.environ["NDI_TRILINEAR_VEC"] = vec
                it.interp_array_into(*q, out, fresh=True)
            return run
        wide = lanes % (16 // np.dtype(dt).itemsize) == 0
        variants = {f"stage{s}_{'wide' if v == '-1' else 'scalar'}": form(s, v)
                    for s in ("1", "0") for v in (("-1", "1") if wide else ("1",))}
        ev = measure(variants)
        nbytes = nq * (lanes + 3) * np.dtype(dt).itemsize
        for v in ev.values():
            v["gqueries_per_s"] = nq / v["median_ms"] / 1e6
            v["gbytes_per_s"] = nbytes / v["median_ms"] / 1e6
        res["cases"][name] = ev
        print(name, json.dumps(ev), flush=True)
        os.environ.pop("NDI_TRILINEAR_STAGE", None)
        os.environ.pop("NDI_TRILINEAR_VEC", None)
        del it, data, q, out
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump(res, open(out_path, "w"), indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trilinear_rates.json"))
    ap.add_argument("--queries", type=int, default=NQ)
    ap.add_argument("--case", action="append", help="instead of all cases")
    a = ap.parse_args()
    main(a.out, a.queries, a.case)
