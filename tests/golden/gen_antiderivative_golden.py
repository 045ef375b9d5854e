"""Writes tests/golden/antiderivative_scipy.npz: antiderivatives and definite integrals from f64 scipy --
CubicSpline(...).antiderivative()(q) and .integrate(lo, hi), the same of PchipInterpolator and Akima1DInterpolator, and for
Linear the closed-form integral of np.interp's piecewise-linear function -- on seeded inputs, for
tests/test_antiderivative_abi.py (which needs only the .npz, not scipy).

    python tests/golden/gen_antiderivative_golden.py        # scipy >= 1.13; written with 1.15

Cases: the derivative golden's four knot families (even, random, geometric, jittered); interval counts 1, 2, 3, 16, 255,
256, 257, 513, 999, 4095 -- the edges of the prefix sum's 256-knot blocks among them; 1 - 3 lanes; f64 and f32 inputs
(scipy computes in f64 from the inputs' exact values).  Queries: 10 inside the range, 3 + 3 up to half an end interval
outside (extrapolate = True: the end polynomials continue); pairs (lo, hi): the queries against their reverse, so same
interval, across blocks, lo > hi and both outside occur.  Spline boundary kinds as in gen_derivative_golden.py; the
periodic spline is built WITHOUT extrapolation (the Periodic mode has no antiderivative handle): its expected values outside
the knots are NaN and pairs that touch the outside likewise.

Per case: x, y, q, lo, hi, `labels` (sources) and `expect_F`[len(labels)][Q][lanes], `expect_I`[len(labels)][Q][lanes].

The script also measures, per (dtype, source family), the largest deviation of the numpy restatement
(tests/antiderivative_ref.py on the oracle's cubic_build / tests/hermite_ref.build tables in the inputs' dtype) from scipy,
over F and the integrals, as max abs error / (max |expected| + 1), prints it and stores it under `measured/...`:
tests/test_antiderivative_abi.py carries these figures as constants and allows 2 x each.  Likewise, per dtype, the round
trip derivative_ref -> antiderivative_ref of the natural spline of every case against y - y[0], per dtype and knot family
(`measured/<dtype>/roundtrip/<family>`).
"""
import os
import sys

import numpy as np
from scipy.interpolate import Akima1DInterpolator, CubicSpline, PchipInterpolator

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import antiderivative_ref  # noqa: E402
import derivative_ref  # noqa: E402
import hermite_ref  # noqa: E402
import oracle  # noqa: E402
from gen_derivative_golden import SPLINE_KINDS, knots, queries, source_tables  # noqa: E402

# (n, lanes, knot family)
SHAPES = [(2, 1, "even"), (2, 3, "random"), (3, 2, "geometric"), (4, 3, "even"), (17, 3, "jittered"), (256, 1, "random"),
          (257, 1, "geometric"), (258, 3, "jittered"), (514, 1, "even"), (1000, 1, "random"), (4096, 1, "jittered")]


def sources_of(n, family):
    out = []
    if n >= 3:
        out += [k for k in SPLINE_KINDS if not (k == "nk" and (family != "even" or n < 4))]
    out.append("pchip")
    if n >= 3:
        out.append("akima")
    out.append("linear")
    return out


def family_of(source):
    return "spline" if source in SPLINE_KINDS else source


def linear_F(x, y, q):
    """the antiderivative of the piecewise-linear interpolant (end segments continued), closed form, f64"""
    dx = np.diff(x)[:, None]
    C = np.concatenate([np.zeros((1, y.shape[1])), np.cumsum(dx * (y[1:] + y[:-1]) / 2, axis=0)])
    i = np.clip(np.searchsorted(x, q, side="right") - 1, 0, len(x) - 2)
    s = (q - x[i])[:, None]
    m = (y[i + 1] - y[i]) / dx[i]
    return C[i] + s * y[i] + s * s * m / 2


def restated(source, x, y, q, lo, hi):
    if source == "linear":
        ys, a, b = y, None, None
    else:
        ys, a, b = source_tables(source, x, y)
    P = antiderivative_ref.prefix(x, ys, a, b)
    li = antiderivative_ref.lower_index
    return (antiderivative_ref.evaluate(x, ys, a, b, P, li(x, q), q),
            antiderivative_ref.integrate(x, ys, a, b, P, li(x, lo), lo, li(x, hi), hi))


def roundtrip_error(x, y):
    """derivative_ref then antiderivative_ref on the natural spline of (x, y): max |P - (y - y[0])| / (max |y - y[0]| + 1)"""
    ys, a, b = source_tables("nat", x, y)
    Y, A, Bt = derivative_ref.derive(x, ys, a, b)
    P = antiderivative_ref.prefix(x, Y, A, Bt)
    expect = ys.astype(np.float64) - ys[0].astype(np.float64)
    return float(np.abs(P.astype(np.float64) - expect).max() / (np.abs(expect).max() + 1))


def main():
    rng = np.random.default_rng(20240711)
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
            lo, hi = q.copy(), q[::-1].copy()
            lo[0], hi[0] = q[1], np.nextafter(q[1], x[-1]).astype(dt)     # the same interval (almost surely)
            lo[1], hi[1] = q[2], q[2]                                      # lo == hi
            cid = f"{name}_n{n}_L{L}_{family}"
            cases.append(cid)
            x64, y64, q64, lo64, hi64 = (v.astype(np.float64) for v in (x, y, q, lo, hi))
            inside = lambda v: (v >= x64[0]) & (v <= x64[-1])   # noqa: E731
            labels, eF, eI = [], [], []
            for source in sources_of(n, family):
                if source in SPLINE_KINDS:
                    yy = y64.copy()
                    if source == "per":
                        yy[-1] = yy[0]
                    bc = SPLINE_KINDS[source][0]
                    if source == "mix":   # scipy wants one value per lane
                        bc = tuple((order, np.full(L, value)) for order, value in bc)
                    F = CubicSpline(x64, yy, axis=0, bc_type=bc, extrapolate=True).antiderivative()
                    refF, refI = F(q64), F(hi64) - F(lo64)
                    chk = CubicSpline(x64, yy, axis=0, bc_type=bc, extrapolate=True)
                    for j in range(len(q64)):    # .integrate(a, b) is what the file promises: F(b) - F(a) must be it
                        one = chk.integrate(lo64[j], hi64[j], extrapolate=True)
                        assert np.allclose(one, refI[j], rtol=1e-9, atol=1e-12), (cid, source, j)
                    if source == "per":   # built without extrapolation: outside the knots there is no value
                        refF = np.where(inside(q64)[:, None], refF, np.nan)
                        refI = np.where((inside(lo64) & inside(hi64))[:, None], refI, np.nan)
                elif source == "pchip":
                    F = PchipInterpolator(x64, y64, axis=0, extrapolate=True).antiderivative()
                    refF, refI = F(q64), F(hi64) - F(lo64)
                elif source == "akima":
                    F = Akima1DInterpolator(x64, y64, axis=0, method="akima", extrapolate=True).antiderivative()
                    refF, refI = F(q64), F(hi64) - F(lo64)
                else:
                    refF = linear_F(x64, y64, q64)
                    refI = linear_F(x64, y64, hi64) - linear_F(x64, y64, lo64)
                    assert np.allclose(linear_F(x64, y64, x64)[1:], np.cumsum(np.diff(x64)[:, None] * (y64[1:] + y64[:-1]) / 2, 0))
                labels.append(source)
                eF.append(refF)
                eI.append(refI)
                gotF, gotI = restated(source, x, y, q, lo, hi)
                mF, mI = np.isfinite(refF), np.isfinite(refI)
                dev = max(float(np.abs(gotF.astype(np.float64) - refF)[mF].max() / (np.abs(refF[mF]).max() + 1)),
                          float(np.abs(gotI.astype(np.float64) - refI)[mI].max() / (np.abs(refI[mI]).max() + 1)))
                key = (name, family_of(source))
                if dev > worst.get(key, (0.0, ""))[0]:
                    worst[key] = (dev, f"{cid} {source}")
            out[cid + "/x"], out[cid + "/y"], out[cid + "/q"] = x, y, q
            out[cid + "/lo"], out[cid + "/hi"] = lo, hi
            out[cid + "/labels"] = np.array(labels)
            out[cid + "/expect_F"] = np.array(eF)
            out[cid + "/expect_I"] = np.array(eI)
    out["cases"] = np.array(cases)
    # the round trip derivative -> antiderivative of a natural spline against y - y[0], the same scale as above: on knots
    # with near-coincident neighbours a natural spline's derivative is orders of magnitude larger than its values and the
    # sum cancels, so this figure is its own (it is far above the rule's error against scipy), measured like the others
    for name in ("float64", "float32"):
        for family in ("even", "random", "geometric", "jittered"):
            v = max(roundtrip_error(out[c + "/x"], out[c + "/y"]) for c in cases
                    if c.startswith(name) and c.endswith(family) and len(out[c + "/x"]) >= 3)
            out[f"measured/{name}/roundtrip/{family}"] = np.float64(v)
            print(f"{name} roundtrip, {family} knots: antiderivative of the derivative of a natural spline vs y - y[0], "
                  f"largest error / (max|expected| + 1) = {v:.3e}")
    for (name, fam), (v, where) in sorted(worst.items()):
        assert v > 0.0
        out[f"measured/{name}/{fam}"] = np.float64(v)
        print(f"{name} {fam}: restatement vs scipy, largest error / (max|expected| + 1) = {v:.3e}   ({where})")
    path = os.path.join(HERE, "antiderivative_scipy.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(path, size, "bytes,", len(cases), "cases")
    assert size <= 256 * 1024


if __name__ == "__main__":
    main()
