"""Writes tests/golden/inverse_scipy.npz: what tests/test_inverse_ref.py needs to hold the numpy restatement of the inverse
rule (tests/inverse_ref.py) against scipy without importing scipy -- per case the knots, the values, scipy's own f64 PPoly
coefficients of the source (PchipInterpolator, Akima1DInterpolator, CubicSpline(bc_type="natural"), the Pchip's
.derivative() and .antiderivative(), and for Linear the degree-1 PPoly of the data and its .antiderivative()), the queries
v, and scipy's f64 values of that PPoly at check points, by which the test proves that its own f64 evaluation of the
coefficients IS scipy's.

    python tools/gen_inverse_golden.py        # scipy >= 1.13; written with 1.15

Cases: the arrays of tests/inverse_cases.py (clustered knots, increments over four decades, flat intervals, rising and
falling lanes) at its TRIP_SHAPES, (n, lanes, Q) = (3, 3, 63), (5, 4, 65), (257, 4, 65) -- the very arrays whose returned
abscissae the GPU tests evaluate forward again -- f64 and f32 inputs (scipy computes in f64 from the inputs' exact
values); queries: Lo, Hi, node values, their neighbours one ulp inside, random values.

The script also measures, per (dtype, source), the restatement's worst |f_scipy(x) - v| / (eps_T max(|nl|, |nr|)) over the
file, prints it and stores it under `measured/...`: tests/inverse_cases.py carries these figures as MEASURED and the tests
allow 2 x each.
"""
import os
import sys

import numpy as np
from scipy.interpolate import Akima1DInterpolator, CubicSpline, PchipInterpolator, PPoly

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import inverse_cases as ic  # noqa: E402
import inverse_ref as ir  # noqa: E402



def scipy_ppoly(source, x, y):
    if source in ("linear", "anti_linear"):
        p = PPoly(np.stack([np.diff(y, axis=0) / np.diff(x)[:, None], y[:-1]]), x)
    elif source == "akima":
        p = Akima1DInterpolator(x, y, axis=0, method="akima")
    elif source == "spline":
        p = CubicSpline(x, y, axis=0, bc_type="natural")
    else:
        p = PchipInterpolator(x, y, axis=0)
    if source == "dpchip":
        p = p.derivative()
    if source.startswith("anti_"):
        p = p.antiderivative()
    return p


def main():
    from test_inverse_ref import ppoly_eval, residual_ratio
    out, cases, worst = {}, [], {}
    for dt in (np.float64, np.float32):
        name = np.dtype(dt).name
        for n, L, Q in ic.TRIP_SHAPES:
            for source in ic.SOURCES:
                x, y, q = ic.case(source, dt, n, L, Q)
                p = scipy_ppoly(source, x.astype(np.float64), y.astype(np.float64))
                cid = f"{name}_{source}_n{n}_L{L}"
                cases.append(cid)
                rng = np.random.default_rng([n, L, 99])
                xc = np.concatenate([x[:3].astype(np.float64), rng.uniform(x[0], x[-1], 40)])
                out[cid + "/x"], out[cid + "/y"], out[cid + "/q"] = x, y, q
                out[cid + "/c"], out[cid + "/xc"], out[cid + "/fc"] = np.asarray(p.c), xc, p(xc)
                assert np.allclose(ppoly_eval(p.c, x.astype(np.float64), xc[:, None] * np.ones(L)), p(xc), rtol=1e-12, atol=1e-300)
                cls, N, ys, a, b = ic.tables(source, x, y)
                X, _ = ir.solve(cls, x, N, q, ys, a, b)
                v = float(residual_ratio(p.c, x, N, q, X).max())
                key = (name, source)
                if v > worst.get(key, (-1.0, ""))[0]:
                    worst[key] = (v, cid)
    out["cases"] = np.array(cases)
    for (name, source), (v, where) in sorted(worst.items()):
        out[f"measured/{name}/{source}"] = np.float64(v)
        print(f'    ("{name}", "{source}"): {v:.4g},      # {where}')
    path = os.path.join(ROOT, "tests", "golden", "inverse_scipy.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(path, size, "bytes,", len(cases), "cases")
    assert size <= 640 * 1024


if __name__ == "__main__":
    main()
