"""Writes tests/golden/tricubic_scipy.npz: f64 scipy values of the tensor-product cubic spline on a 3-D grid on seeded
inputs, for tests/test_tricubic_abi.py (which needs only the .npz, not scipy).

    python tests/golden/gen_tricubic_golden.py        # written with scipy 1.15.3

Classes of ends (one per case):
  nk   the default ends on grids with at least 4 knots per axis: RegularGridInterpolator(method="cubic",
       solver=scipy.sparse.linalg.spsolve) -- the DIRECT solver; scipy's default iterative solver is only good to about
       1e-5 and is not used.  Every such case is cross-checked here against method="cubic_legacy" (asserted: 1e-12).
  mix  one non-default set, a non-zero end value on each axis (tricubic_ref.MIXED_BC): spline-of-spline with scipy's
       CubicSpline, along z for every grid column, then along y, then along x.
  n3   the default ends with 3 knots on an axis (the build's parabola branch; scipy's not-a-knot on 3 points is the same
       parabola): CubicSpline spline-of-spline.

Knot families even, random, geometric, clustered; 4 x 4 x 4 ... 17 x 9 x 12; 1-3 lanes; f64 and f32 inputs (scipy computes in
f64 from the inputs' exact values).  Queries: 12 random in range, 4 exact nodes, the last knot of every axis.

The script also measures, per (dtype, class), the largest deviation of the numpy restatement (tests/tricubic_ref.py) from
scipy as max abs error / (max |f| + 1), prints it and stores it under `measured/...`: tests/test_tricubic_abi.py carries
these figures as constants and allows 2 x each.
"""
import os
import sys

import numpy as np
from scipy.interpolate import CubicSpline, RegularGridInterpolator
from scipy.sparse.linalg import spsolve

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import oracle  # noqa: E402
import tricubic_ref  # noqa: E402

# (nx, ny, nz, lanes, knot family per axis, class)
CASES = [(4, 4, 4, 1, ("even", "even", "even"), "nk"),
         (5, 7, 6, 2, ("random", "geometric", "clustered"), "nk"),
         (9, 4, 12, 3, ("clustered", "random", "geometric"), "nk"),
         (17, 9, 12, 1, ("random", "random", "random"), "nk"),
         (6, 5, 4, 2, ("geometric", "even", "random"), "mix"),
         (3, 5, 4, 2, ("random", "clustered", "even"), "n3")]

SCIPY_KIND = {oracle.BC_NOT_A_KNOT: "not-a-knot", oracle.BC_NATURAL: "natural", oracle.BC_CLAMPED: "clamped"}


def knots(family, n, rng, dt):
    if family == "even":
        x = np.linspace(0.0, 1.0, n)
    elif family == "random":
        x = np.cumsum(rng.uniform(0.5, 1.5, n))
    elif family == "geometric":
        x = np.logspace(-2, 0, n)
    else:   # clustered: knots crowd towards the middle of the axis
        x = 0.5 + 0.5 * np.sign(np.linspace(-1, 1, n)) * np.abs(np.linspace(-1, 1, n)) ** 2.5 + 1e-3 * np.arange(n)
    x = np.unique(x.astype(dt))
    assert x.size == n, (family, n, x.size)
    return x


def scipy_end(end, shape):
    kind, val = end
    if kind in SCIPY_KIND:
        return SCIPY_KIND[kind]
    return (1 if kind == oracle.BC_FIRST_DERIV else 2, np.full(shape, val))


def spline_of_spline(x, y, z, f, qx, qy, qz, bc):
    """Per query: CubicSpline along z of every (i, j) column, along y of those values, along x of those."""
    nx, ny, nz, C = f.shape
    out = np.empty((len(qx), C))
    for q in range(len(qx)):
        for c in range(C):
            g = CubicSpline(z, f[:, :, :, c], axis=2, bc_type=(scipy_end(bc[4], (nx, ny)), scipy_end(bc[5], (nx, ny))))(qz[q])
            g = CubicSpline(y, g, axis=1, bc_type=(scipy_end(bc[2], (nx,)), scipy_end(bc[3], (nx,))))(qy[q])
            out[q, c] = CubicSpline(x, g, bc_type=(scipy_end(bc[0], ()), scipy_end(bc[1], ())))(qx[q])
    return out


def main():
    rng = np.random.default_rng(20250321)
    out, cases, worst = {}, [], {}
    for dt in (np.float64, np.float32):
        name = np.dtype(dt).name
        for nx, ny, nz, C, fam, cls in CASES:
            ax = [knots(fm, n, rng, dt) for fm, n in zip(fam, (nx, ny, nz))]
            f = rng.normal(size=(nx, ny, nz, C)).astype(dt)
            qs = []
            for k in ax:
                node = k[rng.integers(0, len(k), 4)]
                qs.append(np.concatenate([rng.uniform(k[0], k[-1], 12).astype(dt), node, [k[-1]]]).astype(dt))
            cid = f"{name}_{nx}x{ny}x{nz}x{C}_{'_'.join(fam)}_{cls}"
            cases.append(cid)
            a64 = [a.astype(np.float64) for a in ax]
            f64, q64 = f.astype(np.float64), [q.astype(np.float64) for q in qs]
            bc = tricubic_ref.MIXED_BC if cls == "mix" else tricubic_ref.DEFAULT_BC
            if cls == "nk":
                pts = np.stack(q64, axis=1)
                ref = RegularGridInterpolator(tuple(a64), f64, method="cubic", solver=spsolve)(pts)
                legacy = RegularGridInterpolator(tuple(a64), f64, method="cubic_legacy")(pts)
                cross = float(np.abs(ref - legacy).max() / (np.abs(f64).max() + 1))
                print(f"{cid}: direct solver vs cubic_legacy {cross:.2e}")
                assert cross <= 1e-12, (cid, cross)
            else:
                ref = spline_of_spline(*a64, f64, *q64, bc)
            got = tricubic_ref.interp(*ax, f, *qs, bc).astype(np.float64)
            dev = float(np.abs(got - ref).max() / (np.abs(f64).max() + 1))
            if dev > worst.get((name, cls), (0.0, ""))[0]:
                worst[(name, cls)] = (dev, cid)
            for key, val in zip(("x", "y", "z", "f", "qx", "qy", "qz", "expect"), (*ax, f, *qs, ref)):
                out[f"{cid}/{key}"] = val
            out[cid + "/class"] = np.array(cls)
    out["cases"] = np.array(cases)
    for (name, cls), (v, where) in sorted(worst.items()):
        assert v > 0.0
        out[f"measured/{name}/{cls}"] = np.float64(v)
        print(f"{name} {cls}: restatement vs scipy, largest error / (max|f| + 1) = {v:.3e}   ({where})")
    path = os.path.join(HERE, "tricubic_scipy.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(cases), "cases")
    assert os.path.getsize(path) <= 300 * 1024


if __name__ == "__main__":
    main()
