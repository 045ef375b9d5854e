"""Writes tests/golden/bicubic_partial_scipy.npz: f64 scipy values of the partial derivatives of the tensor-product cubic
spline on seeded inputs, for tests/test_bicubic_partial_abi.py (which needs only the .npz, not scipy).

    python tests/golden/gen_bicubic_partial_golden.py        # written with scipy 1.15.3

The ten SHAPES, the knot families and the query layout are gen_bicubic_golden.py's (12 random queries in range, 4 exact
nodes, the last knot on each axis and on both).  Every case carries all eight orders (nu_x, nu_y) in {0, 1, 2}^2 \\ (0, 0).
Boundary classes (per case the ones that apply):
  nk   the default ends: RectBivariateSpline(x, y, z, kx=3, ky=3, s=0).ev(qx, qy, dx=nu_x, dy=nu_y), every case with
       nx, ny >= 4.
  mix  every case: spline-of-spline with scipy's CubicSpline, along y for every grid row evaluated with `(qy, nu_y)`, then
       along x through the row values evaluated with `(qx, nu_x)`.  The ends are gen_bicubic_golden.py's `mix`: a first
       derivative 0.3 at the left and a second derivative -0.2 at the right end of x, a first derivative 0.7 at the left and
       a second derivative 0.4 at the right end of y.  For nu_y >= 1 the x end VALUES become 0 -- the rows are then
       y-derivatives of the surface, and the y-derivative of a constant end value is 0 -- and the kinds stay.
  n3   the default ends on every case with 3 points on an axis (the build's parabola branch; scipy's not-a-knot on 3 points
       is the same parabola), spline-of-spline.

If the file would pass 200 KiB the f32 copies of the two 64 x 48 cases are dropped, never an order.

The script also measures, per (dtype, class, order), the largest deviation of the numpy restatement
(tests/bicubic_partial_ref.py) from scipy as max abs error / (max |expected| + 1) -- normalised by the expected derivative's
own magnitude, because a second derivative on a 0.05-wide interval is thousands of times |z| -- prints it and stores it
under `measured/<dtype>/<class>` (the eight orders in `orders`' order): tests/test_bicubic_partial_abi.py carries these
figures as constants and allows 2 x each.
"""
import os
import sys

import numpy as np
from scipy.interpolate import CubicSpline, RectBivariateSpline

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import bicubic_partial_ref  # noqa: E402
from gen_bicubic_golden import CLASSES, SHAPES  # noqa: E402
from gen_derivative_golden import knots  # noqa: E402

ORDERS = bicubic_partial_ref.ORDERS
LIMIT = 200 * 1024


def classes_of(nx, ny):
    return ["mix", "n3" if min(nx, ny) == 3 else "nk"]


def spline_of_spline(x, y, z, qx, qy, bcx, bcy, nu_x, nu_y):
    nx, ny, C = z.shape
    if isinstance(bcx, tuple) and nu_y >= 1:
        bcx = tuple((o, 0.0) for o, _ in bcx)
    out = np.empty((len(qx), C))
    for c in range(C):
        rows = CubicSpline(y, z[:, :, c], axis=1, bc_type=bcy if not isinstance(bcy, tuple) else
                           tuple((o, np.full(nx, v)) for o, v in bcy))(qy, nu_y)               # (nx, Q)
        for k in range(len(qx)):
            out[k, c] = CubicSpline(x, rows[:, k], bc_type=bcx)(qx[k], nu_x)
    return out


def generate(skip):
    rng = np.random.default_rng(20250612)
    out, cases, worst = {}, [], {}
    for dt in (np.float64, np.float32):
        name = np.dtype(dt).name
        for nx, ny, C, fx, fy in SHAPES:
            x, y = knots(fx, nx, rng, dt), knots(fy, ny, rng, dt)
            z = rng.normal(size=(nx, ny, C)).astype(dt)
            ni, nj = rng.integers(0, nx, 4), rng.integers(0, ny, 4)
            qx = np.concatenate([rng.uniform(x[0], x[-1], 12).astype(dt), x[ni], [x[-1], x[-1]], rng.uniform(x[0], x[-1], 1).astype(dt)]).astype(dt)
            qy = np.concatenate([rng.uniform(y[0], y[-1], 12).astype(dt), y[nj], [y[-1]], rng.uniform(y[0], y[-1], 1).astype(dt), [y[-1]]]).astype(dt)
            cid = f"{name}_{nx}x{ny}x{C}_{fx}_{fy}"
            if cid in skip:
                continue
            cases.append(cid)
            x64, y64, z64, qx64, qy64 = (a.astype(np.float64) for a in (x, y, z, qx, qy))
            labels, expect = [], []
            for cls in classes_of(nx, ny):
                bcx, bcy, ends = CLASSES[cls]
                per_order = []
                for nu_x, nu_y in ORDERS:
                    if cls == "nk":
                        ref = np.stack([RectBivariateSpline(x64, y64, z64[:, :, c], kx=3, ky=3, s=0).ev(qx64, qy64, dx=nu_x, dy=nu_y)
                                        for c in range(C)], axis=1)
                    else:
                        ref = spline_of_spline(x64, y64, z64, qx64, qy64, bcx, bcy, nu_x, nu_y)
                    per_order.append(ref)
                    got = bicubic_partial_ref.interp(x, y, z, qx, qy, nu_x, nu_y, ends).astype(np.float64)
                    dev = float(np.abs(got - ref).max() / (np.abs(ref).max() + 1))
                    key = (name, cls, nu_x, nu_y)
                    if dev > worst.get(key, (0.0, ""))[0]:
                        worst[key] = (dev, cid)
                labels.append(cls)
                expect.append(per_order)
            out[cid + "/x"], out[cid + "/y"], out[cid + "/z"] = x, y, z
            out[cid + "/q"] = np.stack([qx, qy])                # (one entry: an .npz entry costs more than these bytes)
            out[cid + "/labels"] = np.array(labels)
            out[cid + "/expect"] = np.array(expect)          # (classes, 8 orders, Q, C)
    out["cases"] = np.array(cases)
    out["orders"] = np.array(ORDERS)
    return out, cases, worst


def main():
    path = os.path.join(HERE, "bicubic_partial_scipy.npz")
    big = {f"float32_64x48x{C}_{fx}_{fy}" for nx, ny, C, fx, fy in SHAPES if (nx, ny) == (64, 48)}
    for skip in (set(), big):
        out, cases, worst = generate(skip)
        assert all(v > 0.0 for v, _ in worst.values())
        for name, cls in sorted({k[:2] for k in worst}):            # one entry per (dtype, class): the eight orders in ORDERS' order
            out[f"measured/{name}/{cls}"] = np.array([worst[(name, cls) + o][0] for o in ORDERS])
        np.savez_compressed(path, **out)
        if os.path.getsize(path) <= LIMIT:
            break
        print(f"{os.path.getsize(path)} bytes with {len(cases)} cases: dropping {sorted(big)}")
    for (name, cls, nu_x, nu_y), (v, where) in sorted(worst.items()):
        print(f"{name} {cls} ({nu_x}, {nu_y}): restatement vs scipy, largest error / (max|expected| + 1) = {v:.3e}   ({where})")
    print("MEASURED = {")
    for (name, cls, nu_x, nu_y), (v, _) in sorted(worst.items()):
        print(f'    ("{name}", "{cls}", {nu_x}, {nu_y}): {v:.3e},')
    print("}")
    print(path, os.path.getsize(path), "bytes,", len(cases), "cases")
    assert os.path.getsize(path) <= LIMIT


if __name__ == "__main__":
    main()
