"""Writes tests/golden/bicubic_periodic_scipy.npz: f64 scipy values of the tensor-product cubic spline with periodic axes on
seeded inputs, for tests/test_bicubic_periodic_abi.py (which needs only the .npz, not scipy).

    python tests/golden/gen_bicubic_periodic_golden.py        # written with scipy 1.15.3

Expected values are spline-of-spline with scipy's CubicSpline: along y for every grid row (bc_type "periodic" when y is
periodic, else the case's ends), then per query along x through the row values (bc_type "periodic" when x is periodic).  A
"periodic" CubicSpline extrapolates periodically, so queries outside the range are wrapped by scipy itself.  The value and
the five partial derivatives up to order 2 come from `.derivative()` on either pass.

Cases: 3 x 4 ... 33 x 24, the knot families even, random, geometric, jittered, 1-3 lanes, x periodic / y periodic / both,
and on the other axis the default ends (`nk`), natural ends (`nat`) or a first derivative at the left and a second
derivative at the right end with non-zero values (`mix`; a part with nu_y > 0 has the x ends' kinds with value 0: the
y-derivative of a constant end value).  The 4-point non-periodic axis of the first case is jittered, not random: a
not-a-knot cubic through four knots that lie 6e-4 apart swings to 1e3 and the figure then measures the conditioning of
the data, not the rule.  The data is made periodic by copying the first row / column
onto the last, x first, then y.  Queries on a periodic axis: uniform over 3.5 periods either side of the range, and exactly
k0 - p, kn + p, kn and k0; on the other axis: in range, with a few exact knots.

The script also measures, per (dtype, periodic axes, total order of the partial), the largest deviation of the numpy
restatement (tests/bicubic_periodic_ref.py) from scipy as max abs error / (max |z| + 1), prints it and stores it under
`measured/...`: tests/test_bicubic_periodic_abi.py carries these figures as constants and allows 2 x each.
"""
import os
import sys

import numpy as np
from scipy.interpolate import CubicSpline

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import bicubic_periodic_ref as ref  # noqa: E402
import oracle  # noqa: E402
from gen_derivative_golden import knots  # noqa: E402

# (nx, ny, lanes, x family, y family, periodic axes, ends of the other axis)
CASES = [(3, 4, 1, "even", "jittered", 1, "nk"), (4, 3, 2, "geometric", "even", 2, "nk"), (3, 3, 1, "even", "even", 3, "nk"),
         (4, 4, 2, "random", "jittered", 3, "nk"), (5, 7, 3, "jittered", "geometric", 1, "nat"),
         (7, 5, 2, "random", "even", 2, "nat"), (9, 6, 1, "geometric", "random", 1, "mix"),
         (6, 9, 3, "even", "jittered", 2, "mix"), (16, 12, 2, "random", "random", 3, "nk"),
         (33, 24, 1, "jittered", "even", 1, "nk"), (33, 24, 2, "geometric", "random", 2, "mix"),
         (24, 33, 1, "even", "geometric", 3, "nk")]
PARTS = ((0, 0), (1, 0), (0, 1), (2, 0), (1, 1), (0, 2))
AXES_NAME = {1: "x", 2: "y", 3: "xy"}

NK = (oracle.BC_NOT_A_KNOT, 0.0)
# ends -> (scipy bc_type on x, on y, the contract's four ends); the pair of a periodic axis is not read
ENDS = {
    "nk": ("not-a-knot", "not-a-knot", (NK,) * 4),
    "nat": ("natural", "natural", ((oracle.BC_NATURAL, 0.0),) * 4),
    "mix": (((1, 0.3), (2, -0.2)), ((1, 0.7), (2, 0.4)),
            ((oracle.BC_FIRST_DERIV, 0.3), (oracle.BC_SECOND_DERIV, -0.2), (oracle.BC_FIRST_DERIV, 0.7),
             (oracle.BC_SECOND_DERIV, 0.4))),
}


def spline_of_spline(x, y, z, qx, qy, bcx, bcy, nu_x, nu_y):
    nx, ny, C = z.shape
    out = np.empty((len(qx), C))
    for c in range(C):
        sy = CubicSpline(y, z[:, :, c], axis=1, bc_type=bcy if not isinstance(bcy, tuple) else
                         tuple((o, np.full(nx, v)) for o, v in bcy))
        rows = (sy.derivative(nu_y) if nu_y else sy)(qy)               # (nx, Q)
        if nu_y and isinstance(bcx, tuple):      # the y-derivative of a constant end value is 0: the same kinds, value 0
            bcx = tuple((o, 0.0) for o, _ in bcx)
        for k in range(len(qx)):
            sx = CubicSpline(x, rows[:, k], bc_type=bcx)
            out[k, c] = (sx.derivative(nu_x) if nu_x else sx)(qx[k])
    return out


def axis_queries(rng, k, periodic, dt):
    if periodic:
        p = k[-1] - k[0]
        q = np.concatenate([rng.uniform(k[0] - 3.5 * p, k[-1] + 3.5 * p, 16).astype(dt), [k[0] - p, k[-1] + p, k[-1], k[0]]])
    else:
        q = np.concatenate([rng.uniform(k[0], k[-1], 16).astype(dt), k[rng.integers(0, len(k), 3)], [k[-1]]])
    return rng.permutation(q.astype(dt))


def main():
    rng = np.random.default_rng(20250607)
    out, cases, worst = {}, [], {}
    for dt in (np.float64, np.float32):
        name = np.dtype(dt).name
        for nx, ny, C, fx, fy, axes, ends in CASES:
            x, y = knots(fx, nx, rng, dt), knots(fy, ny, rng, dt)
            z = ref.make_periodic(rng.normal(size=(nx, ny, C)).astype(dt), axes)
            qx, qy = axis_queries(rng, x, axes & 1, dt), axis_queries(rng, y, axes & 2, dt)
            cid = f"{name}_{nx}x{ny}x{C}_{fx}_{fy}_p{AXES_NAME[axes]}_{ends}"
            cases.append(cid)
            bcx, bcy, four = ENDS[ends]
            if axes & 1:
                bcx = "periodic"
            if axes & 2:
                bcy = "periodic"
            x64, y64, z64, qx64, qy64 = (a.astype(np.float64) for a in (x, y, z, qx, qy))
            expect = []
            zx, zy, zxy = ref.tables(x, y, z, four, axes)
            for nu_x, nu_y in PARTS:
                want = spline_of_spline(x64, y64, z64, qx64, qy64, bcx, bcy, nu_x, nu_y)
                expect.append(want)
                got = ref.evaluate_partial(x, y, z, zx, zy, zxy, qx, qy, nu_x, nu_y, axes).astype(np.float64)
                dev = float(np.abs(got - want).max() / (np.abs(z64).max() + 1))
                key = (name, AXES_NAME[axes], nu_x + nu_y)
                if dev > worst.get(key, (0.0, ""))[0]:
                    worst[key] = (dev, cid)
            out[cid + "/x"], out[cid + "/y"], out[cid + "/z"] = x, y, z
            out[cid + "/qx"], out[cid + "/qy"] = qx, qy
            out[cid + "/axes"] = np.int32(axes)
            out[cid + "/ends"] = np.array(ends)
            out[cid + "/expect"] = np.array(expect)
    out["cases"] = np.array(cases)
    out["parts"] = np.array(PARTS, np.int32)
    for (name, ax, order), (v, where) in sorted(worst.items()):
        assert v > 0.0
        out[f"measured/{name}/{ax}/{order}"] = np.float64(v)
        print(f"{name} periodic {ax}, order {order}: restatement vs scipy, largest error / (max|z| + 1) = {v:.3e}   ({where})")
    path = os.path.join(HERE, "bicubic_periodic_scipy.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(cases), "cases")
    assert os.path.getsize(path) <= 200 * 1024


if __name__ == "__main__":
    main()
