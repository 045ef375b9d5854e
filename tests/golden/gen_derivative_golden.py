"""Writes tests/golden/derivative_scipy.npz: first and second derivatives from f64 scipy -- CubicSpline(...)(q, 1) and
(q, 2), PchipInterpolator(...)(q, 1), Akima1DInterpolator(..., method="akima")(q, 1) -- on seeded inputs, for
tests/test_derivative_abi.py and tests/test_gpu_derivative.py (which need only the .npz, not scipy).

    python tests/golden/gen_derivative_golden.py        # scipy >= 1.13 (the `method` argument); written with 1.15

Cases: knots of four families (even, random, geometric, jittered), n = 2 ... 4096, 1 - 3 lanes, f64 and f32 inputs (scipy
computes in f64 from the inputs' exact values); 10 queries inside the range and 3 + 3 up to half an end interval outside
(extrapolate = True: the end polynomials continue; the periodic spline wraps -- its expected values are taken at the
queries wrapped in the inputs' dtype, `wrap` below, so that the wrap's rounding is not counted as the rule's).
Spline boundary kinds: the ones for which
tests/golden/scipy_cubic.npz shows the oracle's tables agreeing with scipy -- natural, clamped, a first / second
derivative mix and periodic on every knot family, not-a-knot on even knots only (on uneven knots the reference's
not-a-knot row differs from scipy's, cubic_spline.rs:635).  The periodic case replaces the last data row by the first.
n == 2 has Pchip only (the spline and Akima need 3 knots); not-a-knot needs 4.  The Akima inputs are kept away from
scipy's relative threshold as gen_hermite_golden.py does (min s > 1e-6 max s, asserted; no case is left out).

Per case: x, y, q, `labels` (source/nu, e.g. "nat/2") and `expect`[len(labels)][Q][lanes] (f64).

The script also measures, per (dtype, source, nu), the largest deviation of the numpy restatement (the source tables from
the oracle's cubic_build / tests/hermite_ref.build in the inputs' dtype, tests/derivative_ref.derive once or twice,
tests/hermite_ref.evaluate) from scipy, as max abs error / (max |expected| + 1), prints it and stores it under
`measured/...`: tests/test_derivative_abi.py carries these figures as constants and allows 2 x each.
"""
import os
import sys

import numpy as np
from scipy.interpolate import Akima1DInterpolator, CubicSpline, PchipInterpolator

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import derivative_ref  # noqa: E402
import hermite_ref  # noqa: E402
import oracle  # noqa: E402

# (n, lanes, knot family)
SHAPES = [(2, 1, "even"), (2, 3, "random"), (3, 2, "geometric"), (3, 1, "jittered"), (4, 1, "even"), (4, 3, "random"),
          (5, 2, "geometric"), (17, 3, "jittered"), (64, 1, "geometric"), (100, 3, "even"), (257, 2, "random"),
          (500, 1, "jittered"), (1000, 1, "geometric"), (4096, 1, "random")]

# spline boundary kinds: name -> (scipy bc_type, oracle keyword arguments)
SPLINE_KINDS = {
    "nat": ("natural", dict(left=(oracle.BC_NATURAL, 0.0), right=(oracle.BC_NATURAL, 0.0))),
    "cl": ("clamped", dict(left=(oracle.BC_CLAMPED, 0.0), right=(oracle.BC_CLAMPED, 0.0))),
    "mix": (((1, 0.3), (2, -0.2)), dict(left=(oracle.BC_FIRST_DERIV, 0.3), right=(oracle.BC_SECOND_DERIV, -0.2))),
    "per": ("periodic", dict(periodic=True)),
    "nk": ("not-a-knot", dict()),
}


def knots(family, n, rng, dt):
    if family == "even":
        x = np.linspace(0.0, 1.0, n)
    elif family == "random":   # sorted-unique uniform
        x = np.sort(np.unique(rng.uniform(0.0, 1.0, 4 * n).astype(dt))[:n].astype(np.float64))
    elif family == "jittered":
        x = np.sort(np.linspace(0.0, 1.0, n) + rng.uniform(-0.2 / n, 0.2 / n, n))
    else:
        x = np.logspace(-2, 0, n)
    x = np.unique(x.astype(dt))
    assert x.size == n, (family, n, x.size)
    return x


def queries(rng, x, dt):
    q = np.concatenate([rng.uniform(x[0], x[-1], 10),
                        x[0] - rng.uniform(0, 0.5, 3) * (x[1] - x[0]),        # up to half an end interval outside
                        x[-1] + rng.uniform(0, 0.5, 3) * (x[-1] - x[-2])]).astype(dt)
    return q


def sources_of(n, family):
    """the (source, nu) pairs a case has, in file order"""
    out = []
    if n >= 3:
        for kind in SPLINE_KINDS:
            if kind == "nk" and (family != "even" or n < 4):
                continue
            out += [(kind, 1), (kind, 2)]
    out.append(("pchip", 1))
    if n >= 3:
        out.append(("akima", 1))
    return out


def source_tables(source, x, y):
    """(y, a, b) of the source in the inputs' dtype: what the restatement starts from"""
    if source in SPLINE_KINDS:
        if source == "per":
            y = y.copy()
            y[-1] = y[0]
        st, a, b = oracle.cubic_build(x, y, **SPLINE_KINDS[source][1])
        assert st == oracle.OK
        return y, a, b
    a, b = hermite_ref.build(source, x, y)
    return y, a, b


def wrap(source, x, q):
    """the periodic spline's extrapolation: queries taken into [x0, x_{n-1}) by the period, in the inputs' dtype"""
    if source != "per":
        return q
    return (x[0] + np.mod(q - x[0], x[-1] - x[0])).astype(q.dtype)


def restated(source, nu, x, y, q):
    ys, a, b = source_tables(source, x, y)
    Y, A, B = derivative_ref.derive_nu(x, ys, a, b, nu)
    return hermite_ref.evaluate(x, Y, A, B, wrap(source, x, q))


def family_of(source):
    return "spline" if source in SPLINE_KINDS else source


def main():
    rng = np.random.default_rng(20240611)
    out, cases, worst = {}, [], {}
    for dt in (np.float64, np.float32):
        name = np.dtype(dt).name
        for n, L, family in SHAPES:
            x = knots(family, n, rng, dt)
            y = rng.normal(size=(n, L)).astype(dt)
            if n >= 3:   # Akima: clear of scipy's relative threshold (redrawn, never dropped)
                for attempt in range(1000):
                    s = hermite_ref.akima_k(x, y)[1]
                    if s.min() > 1e-6 * s.max():
                        break
                    y = rng.normal(size=(n, L)).astype(dt)
                s = hermite_ref.akima_k(x, y)[1]
                assert s.min() > 1e-6 * s.max(), (name, n, L, family)
            q = queries(rng, x, dt)
            cid = f"{name}_n{n}_L{L}_{family}"
            cases.append(cid)
            x64, y64, q64 = x.astype(np.float64), y.astype(np.float64), q.astype(np.float64)
            labels, expect = [], []
            for source, nu in sources_of(n, family):
                if source in SPLINE_KINDS:
                    yy = y64.copy()
                    if source == "per":
                        yy[-1] = yy[0]
                    bc = SPLINE_KINDS[source][0]
                    if source == "mix":   # scipy wants one value per lane
                        bc = tuple((order, np.full(L, value)) for order, value in bc)
                    # (the periodic spline is asked at the wrapped queries' exact values: the wrap's own rounding moves a
                    # query by an ulp of x, which is evaluation, not the derivative rule measured here)
                    ref = CubicSpline(x64, yy, axis=0, bc_type=bc, extrapolate="periodic" if source == "per" else True)(
                        wrap(source, x, q).astype(np.float64), nu)
                elif source == "pchip":
                    ref = PchipInterpolator(x64, y64, axis=0, extrapolate=True)(q64, nu)
                else:
                    ref = Akima1DInterpolator(x64, y64, axis=0, method="akima", extrapolate=True)(q64, nu)
                labels.append(f"{source}/{nu}")
                expect.append(ref)
                got = restated(source, nu, x, y, q).astype(np.float64)
                dev = float(np.abs(got - ref).max() / (np.abs(ref).max() + 1))
                key = (name, family_of(source), nu)
                if dev > worst.get(key, (0.0, ""))[0]:
                    worst[key] = (dev, f"{cid} {source}")
            out[cid + "/x"], out[cid + "/y"], out[cid + "/q"] = x, y, q
            out[cid + "/labels"] = np.array(labels)
            out[cid + "/expect"] = np.array(expect)
    out["cases"] = np.array(cases)
    for (name, fam, nu), (v, where) in sorted(worst.items()):
        assert v > 0.0
        out[f"measured/{name}/{fam}/{nu}"] = np.float64(v)
        print(f"{name} {fam} nu={nu}: restatement vs scipy, largest error / (max|expected| + 1) = {v:.3e}   ({where})")
    path = os.path.join(HERE, "derivative_scipy.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(path, size, "bytes,", len(cases), "cases")
    assert size <= os.path.getsize(os.path.join(HERE, "hermite_scipy.npz"))


if __name__ == "__main__":
    main()
