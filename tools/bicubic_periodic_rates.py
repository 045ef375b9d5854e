"""Rates of Bicubic with periodic axes (output committed as profiles/bicubic_periodic_rates.json).  Needs an
MI355X; there is no CPU fallback.  The method is tools/bicubic_rates.py's: one process, device-resident inputs, fresh
device outputs of the library's own, the median of 7 after a warm-up, two alternating rounds per handle (the spread of a
handle's two rounds is the margin a comparison has to clear).

    python tools/bicubic_periodic_rates.py --plain --out FILE [--root TREE]
        (a) the non-periodic handle alone: 100 x 100 x 5 f64 and 2048 x 2048 x 64 f32, 1e7 queries, four rounds.  --root
        names another checkout of this project (its package and its built library are loaded instead of this one's), so the
        parent commit and the branch run the same script: the branch may not be slower than the parent by more than the
        spread of the parent's own rounds.
    python tools/bicubic_periodic_rates.py --out profiles/bicubic_periodic_rates.json [--merge-plain PARENT_FILE BRANCH_FILE]
        (b) a handle that wraps on both axes beside the non-periodic handle on the same shapes, as ratios to it: all
        queries in range; all queries one to three periods out; 1 % of the queries 1e6 periods out (fmod's trip count
        depends on the quotient, and a wave waits for its farthest lane).
        (c) the build of a both-periodic 2048 x 2048 x 64 f32 grid beside the default-ends build of the same grid.
        --merge-plain adds the two files of (a) and their verdict.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [("f64", 100, 100, 5), ("f32", 2048, 2048, 64)]
DTYPES = {"f64": np.float64, "f32": np.float32}
QUERIES = 10_000_000


def package(root):
    sys.path.insert(0, root)
    from __graft_entry__ import load_package
    return load_package()


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


def grid(name, nx, ny, C, periodic):
    import torch
    dt = DTYPES[name]
    rng = np.random.default_rng(nx + ny + C)
    x = np.cumsum(rng.uniform(0.5, 1.5, nx)).astype(dt)
    y = np.cumsum(rng.uniform(0.5, 1.5, ny)).astype(dt)
    z = torch.rand((nx, ny, C), dtype=torch.float32 if name == "f32" else torch.float64, device="cuda:0")
    if periodic:
        z[-1] = z[0]
        z[:, -1] = z[:, 0]
    return x, y, z


def queries(name, x, y, kind):
    """in: in range; near: every query one to three periods out on both axes; far: 1 % of them 1e6 periods out"""
    import torch
    dt = DTYPES[name]
    rng = np.random.default_rng(len(x) + 7)
    qx, qy = rng.uniform(x[0], x[-1], QUERIES), rng.uniform(y[0], y[-1], QUERIES)
    px, py = float(x[-1] - x[0]), float(y[-1] - y[0])
    if kind == "near":
        qx += rng.choice([-3, -2, -1, 1, 2, 3], QUERIES) * px
        qy += rng.choice([-3, -2, -1, 1, 2, 3], QUERIES) * py
    elif kind == "far":
        far = rng.uniform(size=QUERIES) < 0.01
        qx[far] += 1e6 * px
        qy[far] -= 1e6 * py
    return torch.as_tensor(qx.astype(dt), device="cuda:0"), torch.as_tensor(qy.astype(dt), device="cuda:0")


def build(pkg, x, y, z, strategy):
    import torch
    return pkg.Interp2DBuilder.new(z).x(torch.as_tensor(x, device="cuda:0")).y(torch.as_tensor(y, device="cuda:0")) \
        .strategy(strategy).build()


def plain_pass(root, out_path):
    import torch
    pkg = package(root)
    assert torch.cuda.is_available() and pkg.device_count() >= 1, "needs a GPU"
    res = {"device": torch.cuda.get_device_name(0), "root": os.path.basename(os.path.abspath(root)), "eval_ms": {}}
    for name, nx, ny, C in SHAPES:
        key = f"{name}_{nx}x{ny}x{C}"
        x, y, z = grid(name, nx, ny, C, False)
        h = build(pkg, x, y, z, pkg.Bicubic.new())
        qx, qy = queries(name, x, y, "in")
        out = torch.empty((QUERIES, C), dtype=z.dtype, device="cuda:0")
        res["eval_ms"][key] = [median_ms(lambda: h.interp_array_into(qx, qy, out)) for _ in range(4)]
        print(key, json.dumps(res["eval_ms"][key]), flush=True)
        del h, z, qx, qy, out
        torch.cuda.empty_cache()
    json.dump(res, open(out_path, "w"), indent=1)


def spread(rounds):
    m = [r["median"] for r in rounds]
    return (max(m) - min(m)) / min(m)


def periodic_pass(out_path, merge):
    import torch
    pkg = package(HERE)
    assert torch.cuda.is_available() and pkg.device_count() >= 1, "needs a GPU"
    res = {"device": torch.cuda.get_device_name(0), "queries": QUERIES, "eval_ms": {}, "ratio_to_plain": {}, "create_ms": {}}
    for name, nx, ny, C in SHAPES:
        key = f"{name}_{nx}x{ny}x{C}"
        x, y, z = grid(name, nx, ny, C, True)
        plain = build(pkg, x, y, z, pkg.Bicubic.new().extrapolate(True))
        wrap = build(pkg, x, y, z, pkg.Bicubic.new().periodic().extrapolate(True))
        out = torch.empty((QUERIES, C), dtype=z.dtype, device="cuda:0")
        qs = {kind: queries(name, x, y, kind) for kind in ("in", "near", "far")}
        e = res["eval_ms"][key] = {}
        for rnd in range(2):               # alternate the handles: other work shares the host
            e[f"plain_in_round{rnd}"] = median_ms(lambda: plain.interp_array_into(*qs["in"], out))
            for kind in ("in", "near", "far"):
                e[f"wrap_{kind}_round{rnd}"] = median_ms(lambda: wrap.interp_array_into(*qs[kind], out))
        base = min(e["plain_in_round0"]["median"], e["plain_in_round1"]["median"])
        res["ratio_to_plain"][key] = {kind: min(e[f"wrap_{kind}_round0"]["median"], e[f"wrap_{kind}_round1"]["median"]) / base
                                      for kind in ("in", "near", "far")}
        res["ratio_to_plain"][key]["plain_spread"] = spread([e["plain_in_round0"], e["plain_in_round1"]])
        print(key, json.dumps(res["ratio_to_plain"][key]), flush=True)
        if nx == 2048:                     # (c) the build, both-periodic beside default ends, alternating
            c = res["create_ms"][key] = {}
            for rnd in range(2):
                c[f"default_round{rnd}"] = median_ms(lambda: build(pkg, x, y, z, pkg.Bicubic.new()), reps=5)
                c[f"periodic_round{rnd}"] = median_ms(lambda: build(pkg, x, y, z, pkg.Bicubic.new().periodic()), reps=5)
            c["periodic_over_default"] = min(c["periodic_round0"]["median"], c["periodic_round1"]["median"]) / \
                min(c["default_round0"]["median"], c["default_round1"]["median"])
            print(key, "create", json.dumps(c), flush=True)
        del plain, wrap, z, qs, out
        torch.cuda.empty_cache()
    if merge:
        parent, branch = ([json.load(open(p)) for p in files.split(",")] for files in merge)   # (runs of separate processes)
        res["plain_parent_vs_branch"] = {}
        for key in parent[0]["eval_ms"]:
            p, b = ([r for run in runs for r in run["eval_ms"][key]] for runs in (parent, branch))
            pm, bm = min(r["median"] for r in p), min(r["median"] for r in b)
            res["plain_parent_vs_branch"][key] = {
                "parent_rounds_ms": [r["median"] for r in p], "branch_rounds_ms": [r["median"] for r in b],
                "parent_spread": spread(p), "branch_over_parent": bm / pm,
                "branch_not_slower_by_more_than_the_parents_spread": bool(bm / pm - 1.0 <= spread(p))}
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump(res, open(out_path, "w"), indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--plain", action="store_true", help="(a): the non-periodic handle alone")
    ap.add_argument("--root", default=HERE, help="with --plain: the checkout whose package and library are measured")
    ap.add_argument("--merge-plain", nargs=2, metavar=("PARENT_FILE", "BRANCH_FILE"))
    a = ap.parse_args()
    if a.plain:
        plain_pass(a.root, a.out)
    else:
        periodic_pass(a.out, a.merge_plain)


if __name__ == "__main__":
    main()
