"""Writes tests/golden/bicubic_scipy.npz: f64 scipy values of the tensor-product cubic spline on seeded inputs, for
tests/test_bicubic_abi.py (which needs only the .npz, not scipy).

    python tests/golden/gen_bicubic_golden.py        # written with scipy 1.15.3

Boundary classes (per case the ones that apply):
  nk   the default ends: RectBivariateSpline(x, y, z, kx=3, ky=3, s=0).ev(qx, qy), every case with nx, ny >= 4.
  nat, cl, mix, n3
       spline-of-spline with scipy's CubicSpline: along y for every grid row, then along x through the row values.  `mix`
       has a first derivative 0.3 at the left and a second derivative -0.2 at the right end of x, and a first derivative
       0.7 at the left and a second derivative 0.4 at the right end of y.  `n3` is the default ends on every case with 3
       points on an axis (the build's parabola branch; scipy's not-a-knot on 3 points is the same parabola).
RegularGridInterpolator(method="cubic") is NOT this function and is not used.

Knot families even, random, geometric, jittered; 3 x 3 ... 64 x 48; 1-3 lanes; f64 and f32 inputs (scipy computes in f64
from the inputs' exact values).  Queries: 12 random in range, 4 exact nodes, the last knot on each axis and on both.

The script also measures, per (dtype, class), the largest deviation of the numpy restatement (tests/bicubic_ref.py) from
scipy as max abs error / (max |z| + 1), prints it and stores it under `measured/...`: tests/test_bicubic_abi.py carries
these figures as constants and allows 2 x each.
"""
import os
import sys

import numpy as np
from scipy.interpolate import CubicSpline, RectBivariateSpline

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import bicubic_ref  # noqa: E402
import oracle  # noqa: E402
from gen_derivative_golden import knots  # noqa: E402

# (nx, ny, lanes, x family, y family)
SHAPES = [(3, 3, 1, "even", "random"), (3, 4, 2, "geometric", "even"), (4, 3, 3, "even", "jittered"),
          (4, 4, 1, "even", "even"), (5, 7, 2, "random", "geometric"), (9, 6, 3, "jittered", "random"),
          (16, 16, 1, "even", "even"), (33, 20, 2, "geometric", "jittered"), (64, 48, 1, "even", "even"),
          (64, 48, 2, "random", "random")]

# class -> (scipy bc_type on x, on y, the contract's four ends)
NK = (oracle.BC_NOT_A_KNOT, 0.0)
CLASSES = {
    "nat": ("natural", "natural", ((oracle.BC_NATURAL, 0.0),) * 4),
    "cl": ("clamped", "clamped", ((oracle.BC_CLAMPED, 0.0),) * 4),
    "mix": (((1, 0.3), (2, -0.2)), ((1, 0.7), (2, 0.4)),
            ((oracle.BC_FIRST_DERIV, 0.3), (oracle.BC_SECOND_DERIV, -0.2), (oracle.BC_FIRST_DERIV, 0.7),
             (oracle.BC_SECOND_DERIV, 0.4))),
    "n3": ("not-a-knot", "not-a-knot", (NK,) * 4),
    "nk": (None, None, (NK,) * 4),
}


def classes_of(nx, ny):
    return ["nat", "cl", "mix", "n3" if min(nx, ny) == 3 else "nk"]


def spline_of_spline(x, y, z, qx, qy, bcx, bcy):
    nx, ny, C = z.shape
    out = np.empty((len(qx), C))
    for c in range(C):
        rows = CubicSpline(y, z[:, :, c], axis=1, bc_type=bcy if not isinstance(bcy, tuple) else
                           tuple((o, np.full(nx, v)) for o, v in bcy))(qy)               # (nx, Q)
        for k in range(len(qx)):
            out[k, c] = CubicSpline(x, rows[:, k], bc_type=bcx)(qx[k])
    return out


def main():
    rng = np.random.default_rng(20250117)
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
            cases.append(cid)
            x64, y64, z64, qx64, qy64 = (a.astype(np.float64) for a in (x, y, z, qx, qy))
            labels, expect = [], []
            for cls in classes_of(nx, ny):
                bcx, bcy, ends = CLASSES[cls]
                if cls == "nk":
                    ref = np.stack([RectBivariateSpline(x64, y64, z64[:, :, c], kx=3, ky=3, s=0).ev(qx64, qy64)
                                    for c in range(C)], axis=1)
                else:
                    ref = spline_of_spline(x64, y64, z64, qx64, qy64, bcx, bcy)
                labels.append(cls)
                expect.append(ref)
                got = bicubic_ref.interp(x, y, z, qx, qy, ends).astype(np.float64)
                dev = float(np.abs(got - ref).max() / (np.abs(z64).max() + 1))
                if dev > worst.get((name, cls), (0.0, ""))[0]:
                    worst[(name, cls)] = (dev, cid)
            out[cid + "/x"], out[cid + "/y"], out[cid + "/z"] = x, y, z
            out[cid + "/qx"], out[cid + "/qy"] = qx, qy
            out[cid + "/labels"] = np.array(labels)
            out[cid + "/expect"] = np.array(expect)
    out["cases"] = np.array(cases)
    for (name, cls), (v, where) in sorted(worst.items()):
        assert v > 0.0
        out[f"measured/{name}/{cls}"] = np.float64(v)
        print(f"{name} {cls}: restatement vs scipy, largest error / (max|z| + 1) = {v:.3e}   ({where})")
    path = os.path.join(HERE, "bicubic_scipy.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(cases), "cases")
    assert os.path.getsize(path) <= 200 * 1024


if __name__ == "__main__":
    main()
