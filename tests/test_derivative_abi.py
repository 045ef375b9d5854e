"""CPU: derivative handles at the boundary -- the two new entry points in the header, the ctypes binding, the built library
and the Rust declarations; the refusals that need no handle; and the accuracy of the numerical rule's numpy restatement
(tests/derivative_ref.py, what the GPU tests compare the device against bit for bit) against scipy's derivatives through
tests/golden/derivative_scipy.npz (tests/golden/gen_derivative_golden.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import derivative_ref
import hermite_ref
import oracle
from conftest import GOLDEN, ROOT

# name -> oracle.cubic_build keyword arguments (the generator's SPLINE_KINDS)
SPLINE_KINDS = {
    "nat": dict(left=(oracle.BC_NATURAL, 0.0), right=(oracle.BC_NATURAL, 0.0)),
    "cl": dict(left=(oracle.BC_CLAMPED, 0.0), right=(oracle.BC_CLAMPED, 0.0)),
    "mix": dict(left=(oracle.BC_FIRST_DERIV, 0.3), right=(oracle.BC_SECOND_DERIV, -0.2)),
    "per": dict(periodic=True),
    "nk": dict(),
}

# Largest error of the restatement against f64 scipy over the golden file, max abs error / (max |expected| + 1), as
# tests/golden/gen_derivative_golden.py measured and printed it; the bar is 2 x each.  The inputs are fixed and the
# operations are + - * /, so the factor only covers a numpy build that orders an operation differently.
MEASURED = {
    ("float64", "spline", 1): 2.065e-15,
    ("float64", "spline", 2): 1.381e-14,
    ("float64", "pchip", 1): 9.624e-16,
    ("float64", "akima", 1): 6.443e-16,
    ("float32", "spline", 1): 6.896e-07,
    ("float32", "spline", 2): 2.330e-06,
    ("float32", "pchip", 1): 3.022e-07,
    ("float32", "akima", 1): 3.971e-07,
}


def golden():
    return np.load(os.path.join(GOLDEN, "derivative_scipy.npz"))


def source_tables(source, x, y):
    """(y, a, b) of the source in the inputs' dtype: the oracle's spline build, the Hermite restatement"""
    if source in SPLINE_KINDS:
        if source == "per":
            y = y.copy()
            y[-1] = y[0]
        st, a, b = oracle.cubic_build(x, y, **SPLINE_KINDS[source])
        assert st == oracle.OK
        return y, a, b
    a, b = hermite_ref.build(source, x, y)
    return y, a, b


def wrap(source, x, q):
    """the periodic spline's extrapolation (the golden's expected values are taken at these wrapped queries)"""
    if source != "per":
        return q
    return (x[0] + np.mod(q - x[0], x[-1] - x[0])).astype(q.dtype)


# ---- the boundary ------------------------------------------------------------------------------------------------
def test_header_capi_library_and_rust_carry_both_symbols(pkg):
    cap = pkg._capi
    header = open(os.path.join(ROOT, "include", "ndinterp.h")).read()
    assert re.search(r"ndi_status ndi_interp1d_derivative\(const ndi_interp1d\* h, int32_t nu, ndi_interp1d\*\* out\);", header)
    assert re.search(r"ndi_status ndi_interp1d_data\(const ndi_interp1d\* h, void\* data_out, int32_t memspace\);", header)
    # the rule, the knot convention and the k-table statement are part of the contract
    for text in ("Y[i]   = (dy + a[i]) / dx", "Y[n-1] = (dy - b[n-2]) / dx", "A[i]   = B[i] = (3 * (b[i] - a[i])) / dx",
                 "interval to its RIGHT", "residual of the Thomas solve", "never read", "keeps no k table"):
        assert text in header, text
    lib = C.CDLL(cap.LIB_PATH)
    for name in ("ndi_interp1d_derivative", "ndi_interp1d_data"):
        assert name in cap.SYMBOLS and hasattr(lib, name), name
    rust = open(os.path.join(ROOT, "rust", "ndarray-interp-hip", "src", "hip_ffi.rs")).read()
    assert "pub fn ndi_interp1d_derivative(h: *const ndi_interp1d, nu: i32, out: *mut *mut ndi_interp1d) -> i32;" in rust
    assert "pub fn ndi_interp1d_data(h: *const ndi_interp1d, data_out: *mut c_void, memspace: i32) -> i32;" in rust
    assert cap.lib().ndi_version() == (0 << 16) | 5     # two new symbols, no new enumerator: no version change
    assert issubclass(pkg.DerivativeStrategy, pkg.CubicSplineStrategy)
    assert callable(pkg.Interp1D.derivative) and callable(pkg.DerivativeStrategy.coefficients)


def test_refusals_that_need_no_handle(pkg):
    cap, lib = pkg._capi, pkg._capi.lib()
    h = C.c_void_p(1234)
    assert lib.ndi_interp1d_derivative(None, 1, C.byref(h)) == cap.BAD_ARG
    assert cap.last_error() == "null handle" and h.value is None       # *out is cleared
    assert lib.ndi_interp1d_derivative(None, 2, C.byref(h)) == cap.BAD_ARG and cap.last_error() == "null handle"
    for nu in (0, -1):
        assert lib.ndi_interp1d_derivative(None, nu, C.byref(h)) == cap.BAD_ARG
        assert cap.last_error() == f"nu = {nu}: the derivative order must be 1 or 2"
    for nu in (3, 7):
        assert lib.ndi_interp1d_derivative(None, nu, C.byref(h)) == cap.BAD_ARG
        assert cap.last_error().startswith(f"nu = {nu}: the third and higher derivatives of a piecewise cubic jump at the knots")
        assert "orders 1 and 2 only" in cap.last_error()
    assert lib.ndi_interp1d_derivative(None, 1, None) == cap.BAD_ARG and cap.last_error() == "null out pointer"
    buf = np.zeros(4)
    assert lib.ndi_interp1d_data(None, buf.ctypes.data, cap.MEM_HOST) == cap.BAD_ARG and cap.last_error() == "null handle"


def test_mirror_refuses_strategies_without_a_handle(pkg):
    class Mine(pkg.Interp1DStrategy):
        def interp_into(self, interpolator, target, x):
            target[...] = 0

    x = np.array([0.0, 1.0, 2.0])
    with pytest.raises(TypeError, match="derivative needs a built-in device strategy"):
        pkg.Interp1D.new_unchecked(x, x.copy(), Mine()).derivative()
    xi = np.array([0, 1, 2], dtype=np.int16)        # the generic host path (no device handle)
    with pytest.raises(TypeError, match="derivative needs a built-in device strategy"):
        pkg.Interp1D.builder(xi.copy()).x(xi).build().derivative(1)


# ---- the restatement against scipy --------------------------------------------------------------------------------
def test_golden_covers_the_cases_the_specification_names():
    g = golden()
    cases = list(g["cases"])
    assert len(cases) == 28 and sum(c.startswith("float32") for c in cases) == 14
    ns, lanes, families, labels = set(), set(), set(), set()
    for cid in cases:
        x, y, q = g[cid + "/x"], g[cid + "/y"], g[cid + "/q"]
        assert x.dtype == y.dtype == q.dtype and y.shape[0] == len(x) and np.all(np.diff(x) > 0)
        assert g[cid + "/expect"].shape == (len(g[cid + "/labels"]), len(q), y.shape[1])
        assert g[cid + "/expect"].dtype == np.float64
        assert np.sum(q < x[0]) == 3 and np.sum(q > x[-1]) == 3 and np.sum((q > x[0]) & (q < x[-1])) == 10
        ns.add(len(x)); lanes.add(y.shape[1]); families.add(cid.split("_")[-1])
        labels |= set(g[cid + "/labels"])
        if len(x) >= 3:     # no Akima case left out, each clear of scipy's relative threshold
            assert "akima/1" in g[cid + "/labels"]
            s = hermite_ref.akima_k(x, y)[1]
            assert s.min() > 1e-6 * s.max(), cid
        if len(x) >= 4 and cid.endswith("even"):
            assert "nk/1" in g[cid + "/labels"] and "nk/2" in g[cid + "/labels"]
    assert {2, 3, 4, 5, 4096} <= ns and lanes == {1, 2, 3} and families == {"even", "random", "geometric", "jittered"}
    assert labels == {f"{k}/{nu}" for k in SPLINE_KINDS for nu in (1, 2)} | {"pchip/1", "akima/1"}
    assert os.path.getsize(os.path.join(GOLDEN, "derivative_scipy.npz")) <= os.path.getsize(os.path.join(GOLDEN, "hermite_scipy.npz"))


@pytest.mark.parametrize("dt,source,nu", sorted(MEASURED))
def test_rule_matches_scipy(dt, source, nu):
    """max abs error / (max |expected| + 1) per (dtype, source, nu) over every golden case of that triple, against 2 x the
    value the generator measured (MEASURED above; DESIGN.md 4.11 repeats the table)."""
    g = golden()
    bound = 2.0 * MEASURED[(dt, source, nu)]
    assert abs(float(g[f"measured/{dt}/{source}/{nu}"]) - MEASURED[(dt, source, nu)]) <= 1e-3 * MEASURED[(dt, source, nu)]
    worst, seen = 0.0, 0
    for cid in g["cases"]:
        if not cid.startswith(dt):
            continue
        x, y, q = g[cid + "/x"], g[cid + "/y"], g[cid + "/q"]
        for k, label in enumerate(g[cid + "/labels"]):
            src, order = label.split("/")
            if int(order) != nu or (src if src not in SPLINE_KINDS else "spline") != source:
                continue
            ys, a, b = source_tables(src, x, y)
            Y, A, B = derivative_ref.derive_nu(x, ys, a, b, nu)
            assert Y.dtype == A.dtype == B.dtype == np.dtype(dt) and Y.shape == y.shape and A.shape == a.shape
            assert np.array_equal(A, B)
            got = hermite_ref.evaluate(x, Y, A, B, wrap(src, x, q))
            assert got.dtype == np.dtype(dt)
            expect = g[cid + "/expect"][k]
            err = float(np.abs(got.astype(np.float64) - expect).max() / (np.abs(expect).max() + 1))
            worst = max(worst, err)
            seen += 1
            assert err <= bound, (cid, label, err, bound)
    # 12 cases per dtype have n >= 3: 4 boundary kinds each, not-a-knot on the 2 even ones with n >= 4
    assert seen == {("spline", 1): 50, ("spline", 2): 50, ("pchip", 1): 14, ("akima", 1): 12}[(source, nu)]
    print(f"{dt} {source} nu={nu}: largest error against scipy {worst:.3e}, bound {bound:.3e}")


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_the_rule_applied_twice_leaves_zero_coefficient_tables(dt):
    """3 * (B - A) with A == B is exactly 0 (the sign of zero is free): a second derivative is the piecewise-linear
    interpolant of its knot values."""
    g = golden()
    seen = 0
    for cid in g["cases"]:
        x, y = g[cid + "/x"], g[cid + "/y"]
        if x.dtype != np.dtype(dt) or len(x) < 3:
            continue
        for src in ("nat", "per", "pchip", "akima"):
            ys, a, b = source_tables(src, x, y)
            Y1, A1, B1 = derivative_ref.derive(x, ys, a, b)
            Y2, A2, B2 = derivative_ref.derive(x, Y1, A1, B1)
            assert np.all(A2 == 0) and np.all(B2 == 0), (cid, src)
            # ... whose knot values are the rule's: ((Y[i+1] - Y[i]) + A[i]) / dx
            dx = (x[1:] - x[:-1])[:, None]
            assert np.array_equal(Y2[:-1], ((Y1[1:] - Y1[:-1]) + A1) / dx)
            seen += 1
    assert seen == 48


def test_derivative_of_a_cubic_is_its_derivative():
    """A CubicHermite interpolant of a cubic with its own derivatives IS the cubic: the rule must return the cubic's
    first and second derivative to rounding (a mistranscribed rule misses by orders of magnitude)."""
    x = np.cumsum(np.random.default_rng(3).uniform(0.5, 1.5, 12))
    y = (0.5 * x ** 3 - x ** 2 + 2 * x - 1)[:, None]
    k = (1.5 * x ** 2 - 2 * x + 2)[:, None]
    a, b = hermite_ref.build("hermite", x, y, k)
    q = np.linspace(x[0] - 0.3, x[-1] + 0.3, 301)
    Y, A, B = derivative_ref.derive(x, y, a, b)
    assert np.abs(Y - k).max() < 1e-12 * np.abs(k).max()
    assert np.abs(hermite_ref.evaluate(x, Y, A, B, q).ravel() - (1.5 * q ** 2 - 2 * q + 2)).max() < 1e-11 * np.abs(k).max()
    Y2, A2, B2 = derivative_ref.derive(x, Y, A, B)
    assert np.abs(hermite_ref.evaluate(x, Y2, A2, B2, q).ravel() - (3 * q - 2)).max() < 1e-10 * np.abs(3 * x - 2).max()
