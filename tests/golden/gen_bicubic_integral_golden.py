"""Writes tests/golden/bicubic_integral_scipy.npz: f64 scipy values of rectangle integrals of the tensor-product cubic spline
on seeded inputs, for tests/test_bicubic_integral_abi.py (which needs only the .npz, not scipy).

    python tests/golden/gen_bicubic_integral_golden.py        # written with scipy 1.15.3

SHAPES: the small shapes of gen_bicubic_golden.py (3 points on an axis among them, 1 to 3 lanes, the four knot families)
and three long axes that cross the edges of the prefix sum's 256-knot blocks: 257 and 513 knots along x, 513 along y.
Every case carries the same twelve rectangles (xa, xb, ya, yb): the whole domain, xa == xb, ya == yb, both degenerate,
x reversed, both reversed, two with corners on grid nodes, four random ones.
Boundary classes (per case the ones that apply):
  nk   the default ends: RectBivariateSpline(x, y, z, kx=3, ky=3, s=0).integral(xa, xb, ya, yb), every case with
       nx, ny >= 4 (reversed bounds are sorted and the sign applied here: the integral changes sign with each swap).
  mix  every case: spline-of-spline with scipy's CubicSpline, `.integrate(xa, xb)` along x for every grid column, then
       `.integrate(ya, yb)` of the spline along y through those column integrals.  The ends are gen_bicubic_golden.py's
       `mix`; the y end VALUES are multiplied by (xb - xa): the column integrals are x-integrals of the surface, and the
       x-integral of a constant end value v is v (xb - xa).  The kinds stay.
  n3   the default ends on every case with 3 points on an axis (the parabola branch), spline-of-spline.

The script also measures, per (dtype, class), the largest deviation of the numpy restatement
(tests/bicubic_integral_ref.py) from scipy as max abs error / (max |expected| + 1), prints it and stores it under
`measured/<dtype>/<class>`: tests/test_bicubic_integral_abi.py carries these figures as constants and allows 2 x each.
"""
import os
import sys

import numpy as np
from scipy.interpolate import CubicSpline, RectBivariateSpline

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import bicubic_integral_ref  # noqa: E402
from gen_bicubic_golden import CLASSES  # noqa: E402
from gen_derivative_golden import knots  # noqa: E402

LIMIT = 200 * 1024
SHAPES = [(3, 3, 1, "even", "random"), (3, 4, 2, "geometric", "even"), (4, 3, 3, "even", "jittered"),
          (4, 4, 1, "even", "even"), (5, 7, 2, "random", "geometric"), (9, 6, 3, "jittered", "random"),
          (16, 16, 1, "even", "even"), (33, 20, 2, "geometric", "jittered"),
          (257, 5, 2, "random", "even"), (5, 513, 1, "jittered", "random"), (513, 4, 1, "geometric", "jittered")]
NRECT = 12


def classes_of(nx, ny):
    return ["mix", "n3" if min(nx, ny) == 3 else "nk"]


def rectangles(x, y, rng, dt):
    """(4, NRECT): xa, xb, ya, yb"""
    ux = lambda k: rng.uniform(x[0], x[-1], k).astype(dt)   # noqa: E731
    uy = lambda k: rng.uniform(y[0], y[-1], k).astype(dt)   # noqa: E731
    a, b, c, d = ux(1)[0], ux(1)[0], uy(1)[0], uy(1)[0]
    i, j = rng.integers(0, len(x), 4), rng.integers(0, len(y), 4)
    xa = np.array([x[0], a, a, b, max(a, b), max(a, b), x[i[0]], x[i[1]], *ux(4)], dtype=dt)
    xb = np.array([x[-1], a, b, b, min(a, b), min(a, b), x[i[2]], x[-1], *ux(4)], dtype=dt)
    ya = np.array([y[0], c, d, d, min(c, d), max(c, d), y[j[0]], y[j[1]], *uy(4)], dtype=dt)
    yb = np.array([y[-1], d, d, d, max(c, d), min(c, d), y[j[2]], y[-1], *uy(4)], dtype=dt)
    return np.stack([xa, xb, ya, yb])


def spline_of_spline(x, y, z, r, bcx, bcy):
    nx, ny, C = z.shape
    out = np.empty((r.shape[1], C))
    for k, (xa, xb, ya, yb) in enumerate(r.T):
        by = bcy if not isinstance(bcy, tuple) else tuple((o, v * (xb - xa)) for o, v in bcy)
        for c in range(C):
            cols = np.array([CubicSpline(x, z[:, j, c], bc_type=bcx).integrate(xa, xb) for j in range(ny)])
            out[k, c] = CubicSpline(y, cols, bc_type=by).integrate(ya, yb)
    return out


def rect_bivariate(x, y, z, r):
    nx, ny, C = z.shape
    out = np.empty((r.shape[1], C))
    for c in range(C):
        s = RectBivariateSpline(x, y, z[:, :, c], kx=3, ky=3, s=0)
        for k, (xa, xb, ya, yb) in enumerate(r.T):
            sign = (1.0 if xa <= xb else -1.0) * (1.0 if ya <= yb else -1.0)
            out[k, c] = sign * s.integral(min(xa, xb), max(xa, xb), min(ya, yb), max(ya, yb))
    return out


def generate():
    rng = np.random.default_rng(20250701)
    out, cases, worst = {}, [], {}
    for dt in (np.float64, np.float32):
        name = np.dtype(dt).name
        for nx, ny, C, fx, fy in SHAPES:
            x, y = knots(fx, nx, rng, dt), knots(fy, ny, rng, dt)
            z = rng.normal(size=(nx, ny, C)).astype(dt)
            r = rectangles(x, y, rng, dt)
            cid = f"{name}_{nx}x{ny}x{C}_{fx}_{fy}"
            cases.append(cid)
            x64, y64, z64, r64 = (a.astype(np.float64) for a in (x, y, z, r))
            labels, expect = [], []
            for cls in classes_of(nx, ny):
                bcx, bcy, ends = CLASSES[cls]
                ref = rect_bivariate(x64, y64, z64, r64) if cls == "nk" else spline_of_spline(x64, y64, z64, r64, bcx, bcy)
                labels.append(cls)
                expect.append(ref)
                got = bicubic_integral_ref.integral(x, y, z, *r, ends).astype(np.float64)
                dev = float(np.abs(got - ref).max() / (np.abs(ref).max() + 1))
                if dev > worst.get((name, cls), (0.0, ""))[0]:
                    worst[(name, cls)] = (dev, cid)
            out[cid + "/x"], out[cid + "/y"], out[cid + "/z"] = x, y, z
            out[cid + "/r"] = r
            out[cid + "/labels"] = np.array(labels)
            out[cid + "/expect"] = np.array(expect)          # (classes, NRECT, C)
    out["cases"] = np.array(cases)
    return out, cases, worst


def main():
    path = os.path.join(HERE, "bicubic_integral_scipy.npz")
    out, cases, worst = generate()
    assert all(v > 0.0 for v, _ in worst.values())
    for (name, cls), (v, _) in worst.items():
        out[f"measured/{name}/{cls}"] = np.array(v)
    np.savez_compressed(path, **out)
    for (name, cls), (v, where) in sorted(worst.items()):
        print(f"{name} {cls}: restatement vs scipy, largest error / (max|expected| + 1) = {v:.3e}   ({where})")
    print("MEASURED = {")
    for (name, cls), (v, _) in sorted(worst.items()):
        print(f'    ("{name}", "{cls}"): {v:.3e},')
    print("}")
    print(path, os.path.getsize(path), "bytes,", len(cases), "cases")
    assert os.path.getsize(path) <= LIMIT


if __name__ == "__main__":
    main()
