"""Writes tests/golden/hermite_scipy.npz: scipy's PchipInterpolator / Akima1DInterpolator (method="akima") on seeded
inputs, for tests/test_hermite_abi.py and tests/test_gpu_hermite.py (which need only the .npz, not scipy).

    python tests/golden/gen_hermite_golden.py        # scipy >= 1.13 (the `method` argument); written with 1.15

Cases: random and rounded data (flat runs, zeros, sign changes), uneven knots, n = 2, 3, 4, 5 and ~50, 1-D and (n, 5)
data, f64 and f32; queries in range and up to half an end interval outside (extrapolate = True).  Akima's specification
takes the average of the neighbouring slopes for s == 0 exactly where scipy switches below 1e-9 of the largest s, so the
Akima inputs are drawn until min s > 1e-6 max s -- asserted, no case is left out (rounded data gets a seeded
perturbation first: exact flat runs are the s == 0 case itself).

The file also stores, per dtype and rule, the largest deviation of the numpy restatement (tests/hermite_ref.py) from
scipy over all cases, relative to max|y| + 1: the tests allow 4 x that.
"""
import os
import sys

import numpy as np
from scipy.interpolate import Akima1DInterpolator, PchipInterpolator

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import hermite_ref  # noqa: E402

SHAPES = [(2, ()), (2, (5,)), (3, ()), (3, (5,)), (4, ()), (4, (5,)), (5, ()), (5, (5,)), (50, ()), (47, (5,)), (53, (5,))]


def queries(rng, x, dt):
    return np.concatenate([rng.uniform(x[0], x[-1], 60),
                           x[0] - rng.uniform(0, 0.5, 10) * (x[1] - x[0]),       # up to half an end interval outside
                           x[-1] + rng.uniform(0, 0.5, 10) * (x[-1] - x[-2])]).astype(dt)


def main():
    rng = np.random.default_rng(20240607)
    out = {}
    worst = {}
    cases = []
    for dt in (np.float64, np.float32):
        name = np.dtype(dt).name
        worst[name] = {"pchip": 0.0, "akima": 0.0}
        for n, trail in SHAPES:
            for rounded in (False, True):
                x = np.cumsum(rng.uniform(0.1, 2.0, n)).astype(dt)          # uneven knots
                y = rng.normal(size=(n,) + trail)
                if rounded:
                    y = np.round(y)                                         # flat runs, zeros, sign changes
                y = y.astype(dt)
                q = queries(rng, x, dt)
                cid = f"{name}_n{n}_{'x'.join(map(str, trail)) or 's'}_{'rounded' if rounded else 'random'}"
                cases.append(cid)
                x64, q64 = x.astype(np.float64), q.astype(np.float64)
                y2 = y.reshape(n, -1)
                scale = np.abs(y2.astype(np.float64)).max() + 1
                out[cid + "/x"], out[cid + "/y"], out[cid + "/q"] = x, y, q
                ref = PchipInterpolator(x64, y2.astype(np.float64), axis=0, extrapolate=True)(q64)
                out[cid + "/pchip"] = ref
                a, b = hermite_ref.build("pchip", x, y)
                dev = np.abs(hermite_ref.evaluate(x, y2, a, b, q).astype(np.float64) - ref).max() / scale
                worst[name]["pchip"] = max(worst[name]["pchip"], float(dev))
                if n < 3:
                    continue
                ya = y2
                for attempt in range(1000):
                    s = hermite_ref.akima_k(x, ya)[1]
                    if s.min() > 1e-6 * s.max():
                        break
                    ya = (y2.astype(np.float64) + rng.uniform(-0.3, 0.3, y2.shape)).astype(dt)
                s = hermite_ref.akima_k(x, ya)[1]
                assert s.min() > 1e-6 * s.max(), cid
                out[cid + "/y_akima"] = ya.reshape(y.shape)
                ref = Akima1DInterpolator(x64, ya.astype(np.float64), axis=0, method="akima", extrapolate=True)(q64)
                out[cid + "/akima"] = ref
                a, b = hermite_ref.build("akima", x, ya)
                scale = np.abs(ya.astype(np.float64)).max() + 1
                dev = np.abs(hermite_ref.evaluate(x, ya, a, b, q).astype(np.float64) - ref).max() / scale
                worst[name]["akima"] = max(worst[name]["akima"], float(dev))
    out["cases"] = np.array(cases)
    for name, w in worst.items():
        for rule, v in w.items():
            assert v > 0.0
            out[f"deviation/{name}/{rule}"] = np.float64(v)
            print(f"{name} {rule}: restatement vs scipy, largest deviation / (max|y| + 1) = {v:.3e}")
    path = os.path.join(HERE, "hermite_scipy.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(cases), "cases")


if __name__ == "__main__":
    main()
