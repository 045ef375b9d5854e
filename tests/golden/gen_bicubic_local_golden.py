"""Writes tests/golden/bicubic_local_scipy.npz: the node derivatives of the Pchip / Akima Bicubic handles as scipy gives
them, for tests/test_bicubic_local_abi.py (which needs only the .npz, not scipy).

    python tests/golden/gen_bicubic_local_golden.py        # scipy >= 1.13 (the `method` argument); written with 1.15

Reference: PchipInterpolator / Akima1DInterpolator(..., axis=, method="akima").derivative() at the knots, in f64, applied
along x (zx), along y (zy), and along y of the x result (zxy) -- the composition include/ndinterp.h states for
ndi_interp2d_create_bicubic_local.  Cases: seeded random data on uneven axes, shapes from 2 x 2 x 1 (Pchip only) to
33 x 17 x 4, f64 and f32.  Akima's specification takes the average for s == 0 exactly where scipy switches below 1e-9 of
the largest s, so the Akima data is drawn until min s > 1e-6 max s along x, along y and along y of zx -- asserted, no
case is left out (as gen_hermite_golden.py does).

The file also stores, per dtype and rule, the largest deviation of the numpy restatement (tests/bicubic_local_ref.py) from
scipy over the three tables of all cases, relative to max|z| + 1 as in gen_hermite_golden.py: the test allows 4 x that.
"""
import os
import sys

import numpy as np
from scipy.interpolate import Akima1DInterpolator, PchipInterpolator

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import bicubic_local_ref  # noqa: E402
import hermite_ref  # noqa: E402

SHAPES = [(2, 2, 1), (2, 5, 1), (5, 2, 2), (3, 3, 1), (4, 3, 2), (5, 6, 3), (7, 5, 4), (33, 17, 4)]


def scipy_k(rule, knots, f, axis):
    """the rule's derivative at the knots along `axis` of f (f64)"""
    if rule == "pchip":
        return PchipInterpolator(knots, f, axis=axis).derivative()(knots)      # (the query axis takes the place of `axis`)
    return Akima1DInterpolator(knots, f, axis=axis, method="akima").derivative()(knots)


def scipy_tables(rule, x, y, z):
    zx = scipy_k(rule, x, z, 0)
    return zx, scipy_k(rule, y, z, 1), scipy_k(rule, y, zx, 1)


def akima_margin(x, y, z):
    """min s / max s of the three Akima passes of the restatement"""
    nx, ny, C = z.shape
    zx = bicubic_local_ref.tables("akima", x, y, z)[0]
    worst = np.inf
    for knots, cols in ((x, z.reshape(nx, ny * C)), (y, z.transpose(1, 0, 2).reshape(ny, nx * C)),
                        (y, zx.transpose(1, 0, 2).reshape(ny, nx * C))):
        s = hermite_ref.akima_k(knots, np.ascontiguousarray(cols))[1]
        worst = min(worst, float(s.min() / s.max()))
    return worst


def main():
    rng = np.random.default_rng(20240917)
    out, cases, worst = {}, [], {}
    for dt in (np.float64, np.float32):
        name = np.dtype(dt).name
        worst[name] = {"pchip": 0.0, "akima": 0.0}
        for nx, ny, C in SHAPES:
            x = np.cumsum(rng.uniform(0.5, 1.5, nx)).astype(dt)
            y = np.cumsum(rng.uniform(0.5, 1.5, ny)).astype(dt)
            cid = f"{name}_{nx}x{ny}x{C}"
            cases.append(cid)
            out[cid + "/x"], out[cid + "/y"] = x, y
            for rule in bicubic_local_ref.RULES:
                if min(nx, ny) < bicubic_local_ref.MINIMUM[rule]:
                    continue
                for attempt in range(1000):
                    z = rng.normal(size=(nx, ny, C)).astype(dt)
                    if rule == "pchip" or akima_margin(x, y, z) > 1e-6:
                        break
                assert rule == "pchip" or akima_margin(x, y, z) > 1e-6, cid
                out[f"{cid}/{rule}/z"] = z
                ref = scipy_tables(rule, x.astype(np.float64), y.astype(np.float64), z.astype(np.float64))
                got = bicubic_local_ref.tables(rule, x, y, z)
                scale = np.abs(z.astype(np.float64)).max() + 1
                for tab, r, g in zip(("zx", "zy", "zxy"), ref, got):
                    assert r.shape == z.shape and g.dtype == np.dtype(dt)
                    out[f"{cid}/{rule}/{tab}"] = r
                    worst[name][rule] = max(worst[name][rule], float(np.abs(g.astype(np.float64) - r).max() / scale))
    out["cases"] = np.array(cases)
    for name, w in worst.items():
        for rule, v in w.items():
            assert v > 0.0
            out[f"deviation/{name}/{rule}"] = np.float64(v)
            print(f"{name} {rule}: restatement vs scipy, largest deviation of a table entry / (max|z| + 1) = {v:.3e}")
    path = os.path.join(HERE, "bicubic_local_scipy.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(cases), "cases")


if __name__ == "__main__":
    main()
