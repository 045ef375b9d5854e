"""CPU: the Pchip / Akima / CubicHermite strategies at the boundary -- enumerators and the new entry point in the header,
the ctypes binding and the Rust declarations; the builder checks that need no device; and the numerical specification's
numpy restatement (tests/hermite_ref.py, what the GPU tests compare the device against bit for bit) against scipy's
PchipInterpolator / Akima1DInterpolator through tests/golden/hermite_scipy.npz (tests/golden/gen_hermite_golden.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import hermite_ref
from conftest import GOLDEN, ROOT


def golden():
    return np.load(os.path.join(GOLDEN, "hermite_scipy.npz"))


# ---- the boundary ------------------------------------------------------------------------------------------------
def test_header_capi_and_rust_carry_the_new_names(pkg):
    cap = pkg._capi
    assert (cap.LINEAR, cap.CUBIC_SPLINE, cap.PCHIP, cap.AKIMA, cap.CUBIC_HERMITE) == (0, 1, 2, 3, 4)
    header = open(os.path.join(ROOT, "include", "ndinterp.h")).read()
    enum = re.search(r"typedef enum ndi_strategy1d \{(.*?)\} ndi_strategy1d;", header, flags=re.S).group(1)
    assert [e.strip() for e in enum.split(",")] == ["NDI_LINEAR = 0", "NDI_CUBIC_SPLINE = 1", "NDI_PCHIP = 2", "NDI_AKIMA = 3",
                                                    "NDI_CUBIC_HERMITE = 4"]
    assert re.search(r"ndi_status ndi_interp1d_create_hermite\(const ndi_interp1d_desc\* desc, const void\* dydx,\s*"
                     r"ndi_interp1d\*\* out\);", header)
    assert "s == 0" in header and "scipy" in header          # the stated deviation from scipy's Akima
    assert "ndi_interp1d_create_hermite" in cap.SYMBOLS
    assert hasattr(C.CDLL(cap.LIB_PATH), "ndi_interp1d_create_hermite")
    rust = open(os.path.join(ROOT, "rust", "ndarray-interp-hip", "src", "hip_ffi.rs")).read()
    for line in ("pub const NDI_PCHIP: i32 = 2;", "pub const NDI_AKIMA: i32 = 3;", "pub const NDI_CUBIC_HERMITE: i32 = 4;",
                 "pub fn ndi_interp1d_create_hermite("):
        assert line in rust, line
    assert pkg._capi.lib().ndi_version() == (0 << 16) | 5     # new enumerators and one new symbol: no version change
    for cls, need in ((pkg.Pchip, 2), (pkg.Akima, 3), (pkg.CubicHermite, 2)):
        assert cls.MINIMUM_DATA_LENGHT == need
    assert issubclass(pkg.PchipStrategy, pkg.CubicSplineStrategy) and issubclass(pkg.AkimaStrategy, pkg.CubicSplineStrategy) \
        and issubclass(pkg.CubicHermiteStrategy, pkg.CubicSplineStrategy)


def test_validate1d_minimum_lengths_and_monotonic(pkg):
    cap, lib = pkg._capi, pkg._capi.lib()
    x = np.array([1.0, 2.0, 3.0, 4.0])
    for strategy, need in ((cap.PCHIP, 2), (cap.AKIMA, 3), (cap.CUBIC_HERMITE, 2)):
        st = lib.ndi_validate1d(cap.F64, x.ctypes.data, need - 1, need - 1, strategy)
        assert st == cap.NOT_ENOUGH_DATA
        assert cap.last_error() == f"The chosen Interpolation strategy needs at least {need} data points"
        assert lib.ndi_validate1d(cap.F64, x.ctypes.data, need, need, strategy) == cap.OK
        assert lib.ndi_validate1d(cap.F64, x.ctypes.data, 4, 3, strategy) == cap.SHAPE
    rep = np.array([1.0, 2.0, 2.0, 3.0], dtype=np.float32)
    for strategy in (cap.PCHIP, cap.AKIMA, cap.CUBIC_HERMITE):
        assert lib.ndi_validate1d(cap.F32, rep.ctypes.data, 4, 4, strategy) == cap.MONOTONIC
        assert cap.last_error() == "Values in the x axis need to be strictly monotonic rising"


def _desc(pkg, strategy, dtype, x, y):
    cap = pkg._capi
    d = cap.Interp1DDesc()
    d.dtype, d.strategy, d.n, d.lanes, d.x_len = dtype, strategy, len(x), 1, len(x)
    d.x, d.data, d.memspace, d.validate = x.ctypes.data, y.ctypes.data, cap.MEM_HOST, 1
    return d


def test_create_refusals_need_no_device(pkg):
    cap, lib = pkg._capi, pkg._capi.lib()
    x = np.array([1.0, 2.0, 3.0, 4.0]); y = np.array([1.0, 2.0, 0.0, 1.0]); k = np.zeros(4)
    h = C.c_void_p()
    names = {cap.PCHIP: "Pchip", cap.AKIMA: "Akima", cap.CUBIC_HERMITE: "CubicHermite"}

    def create(d):
        if d.strategy == cap.CUBIC_HERMITE:
            return lib.ndi_interp1d_create_hermite(C.byref(d), k.ctypes.data, C.byref(h))
        return lib.ndi_interp1d_create(C.byref(d), C.byref(h))
    for strategy, name in names.items():
        for dtype in (cap.I32, cap.I64, cap.F16, cap.BF16):          # as CubicSpline: f32 / f64 only
            assert create(_desc(pkg, strategy, dtype, x, y)) == cap.BAD_ARG
            assert name in cap.last_error() and "f32 / f64" in cap.last_error()
        d = _desc(pkg, strategy, cap.F64, x, y); d.periodic = 1
        assert create(d) == cap.BAD_ARG and name in cap.last_error() and "periodic" in cap.last_error()
        d = _desc(pkg, strategy, cap.F64, x, y); d.build_flags = cap.BUILD_REFERENCE_ORDER
        assert create(d) == cap.BAD_ARG and name in cap.last_error() and "build_flags" in cap.last_error()
        d = _desc(pkg, strategy, cap.F64, x, y); d.right = cap.Boundary(cap.BC_NATURAL, 0.0)
        assert create(d) == cap.BAD_ARG and name in cap.last_error() and "boundary" in cap.last_error()
        d = _desc(pkg, strategy, cap.F64, x, y); d.left = cap.Boundary(0, 1.5)
        assert create(d) == cap.BAD_ARG and "boundary" in cap.last_error()
        kinds = np.zeros(1, np.int32)
        d = _desc(pkg, strategy, cap.F64, x, y); d.lane_left_kind = kinds.ctypes.data
        assert create(d) == cap.BAD_ARG and name in cap.last_error() and "per-lane" in cap.last_error()
        # the builder checks of validate = 1, before any device work
        xs = np.array([1.0, 2.0, 2.0, 4.0])
        assert create(_desc(pkg, strategy, cap.F64, xs, y)) == cap.MONOTONIC
    d = _desc(pkg, cap.AKIMA, cap.F64, x[:2], y[:2])
    assert lib.ndi_interp1d_create(C.byref(d), C.byref(h)) == cap.NOT_ENOUGH_DATA
    assert cap.last_error() == "The chosen Interpolation strategy needs at least 3 data points"
    d = _desc(pkg, cap.PCHIP, cap.F64, x[:1], y[:1])
    assert lib.ndi_interp1d_create(C.byref(d), C.byref(h)) == cap.NOT_ENOUGH_DATA
    assert cap.last_error() == "The chosen Interpolation strategy needs at least 2 data points"
    # CubicHermite without derivatives: refused, and the message names the entry point that takes them
    d = _desc(pkg, cap.CUBIC_HERMITE, cap.F64, x, y)
    assert lib.ndi_interp1d_create(C.byref(d), C.byref(h)) == cap.BAD_ARG
    assert "ndi_interp1d_create_hermite" in cap.last_error()
    assert lib.ndi_interp1d_create_hermite(C.byref(d), None, C.byref(h)) == cap.BAD_ARG and "dydx" in cap.last_error()
    d = _desc(pkg, cap.PCHIP, cap.F64, x, y)
    assert lib.ndi_interp1d_create_hermite(C.byref(d), k.ctypes.data, C.byref(h)) == cap.BAD_ARG
    assert "NDI_CUBIC_HERMITE" in cap.last_error()
    d.strategy = 5
    assert lib.ndi_interp1d_create(C.byref(d), C.byref(h)) == cap.BAD_ARG and "unknown strategy" in cap.last_error()


def test_mirror_builder_errors(pkg):
    x = np.array([1.0, 2.0, 3.0]); y = np.array([[1.0, 2.0], [0.0, 1.0], [3.0, 2.0]])
    with pytest.raises(pkg.BuilderError.NotEnoughData, match="at least 3 data points"):
        pkg.Interp1D.builder(y[:2]).x(x[:2]).strategy(pkg.Akima.new()).build()
    with pytest.raises(pkg.BuilderError.NotEnoughData, match="at least 2 data points"):
        pkg.Interp1D.builder(y[:1]).x(x[:1]).strategy(pkg.Pchip.new()).build()
    with pytest.raises(pkg.BuilderError.Monotonic):
        pkg.Interp1D.builder(y).x(np.array([1.0, 1.0, 2.0])).strategy(pkg.Pchip.new()).build()
    with pytest.raises(pkg.BuilderError.ShapeError, match=r"dydx has wrong shape. Expected: \[3, 2\], got: \[3\]"):
        pkg.Interp1D.builder(y).x(x).strategy(pkg.CubicHermite.new(np.zeros(3))).build()
    for strat, name in ((pkg.Pchip.new(), "Pchip"), (pkg.Akima.new(), "Akima"), (pkg.CubicHermite.new(np.zeros((3, 2))), "CubicHermite")):
        for dt in (np.int32, np.int64, np.float16):
            with pytest.raises(TypeError, match=name + " covers float32/float64 only"):
                pkg.Interp1D.builder(y.astype(dt)).x(x.astype(dt)).strategy(strat).build()
        assert strat.extrapolate(True) is strat and strat.device(0) is strat


# ---- the restatement against scipy --------------------------------------------------------------------------------
def test_golden_covers_the_cases_the_specification_names():
    g = golden()
    cases = list(g["cases"])
    assert len(cases) == 44
    ns = set()
    for cid in cases:
        x, y = g[cid + "/x"], g[cid + "/y"]
        ns.add(len(x))
        assert x.dtype == y.dtype and y.ndim in (1, 2) and np.all(np.diff(x) > 0)
        q = g[cid + "/q"]
        assert np.any(q < x[0]) and np.any(q > x[-1]) and np.any((q > x[0]) & (q < x[-1]))
        assert q.min() >= x[0] - 0.5 * (x[1] - x[0]) and q.max() <= x[-1] + 0.5 * (x[-1] - x[-2])
        if len(x) >= 3:     # no Akima case left out, each clear of scipy's relative threshold
            s = hermite_ref.akima_k(x, g[cid + "/y_akima"].reshape(len(x), -1))[1]
            assert s.min() > 1e-6 * s.max(), cid
        else:
            assert cid + "/akima" not in g
    assert {2, 3, 4, 5, 50} <= ns
    assert any("rounded" in c for c in cases) and any(g[c + "/y"].ndim == 2 and g[c + "/y"].shape[1] == 5 for c in cases)
    rounded = [g[c + "/y"] for c in cases if "rounded" in c and len(g[c + "/x"]) >= 47]
    assert any(np.any(np.diff(y, axis=0) == 0) for y in rounded) and any(np.any(y == 0) for y in rounded)


@pytest.mark.parametrize("rule", ["pchip", "akima"])
@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_restatement_matches_scipy(rule, dt):
    """Tolerance: 4 x the largest deviation the generator measured over the file (relative to max|y| + 1).  The margin is
    there for a numpy build that orders an operation differently, nothing else: the arithmetic is plain IEEE."""
    g = golden()
    name = np.dtype(dt).name
    bound = 4.0 * float(g[f"deviation/{name}/{rule}"])
    assert bound < (1e-14 if dt == np.float64 else 1e-5)
    worst, seen = 0.0, 0
    for cid in g["cases"]:
        if not cid.startswith(name) or cid + "/" + rule not in g:
            continue
        x, q = g[cid + "/x"], g[cid + "/q"]
        y = g[cid + ("/y_akima" if rule == "akima" else "/y")].reshape(len(x), -1)
        a, b = hermite_ref.build(rule, x, y)
        assert a.dtype == b.dtype == np.dtype(dt) and a.shape == (len(x) - 1, y.shape[1])
        got = hermite_ref.evaluate(x, y, a, b, q)
        assert got.dtype == np.dtype(dt)
        dev = np.abs(got.astype(np.float64) - g[cid + "/" + rule]).max() / (np.abs(y.astype(np.float64)).max() + 1)
        worst = max(worst, float(dev))
        seen += 1
        assert dev <= bound, (cid, dev, bound)
    assert seen == (22 if rule == "pchip" else 18)
    print(f"{name} {rule}: largest deviation from scipy {worst:.3e}, bound {bound:.3e}")


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_pchip_keeps_a_monotone_step_table_monotone(dt):
    """What Pchip is for: a monotone table with steps and plateaus is interpolated without overshoot."""
    x = np.arange(10).astype(dt)
    y = np.array([0, 0, 0, 1, 1, 1, 5, 5, 6, 6], dtype=dt)[:, None]
    a, b = hermite_ref.build("pchip", x, y)
    v = hermite_ref.evaluate(x, y, a, b, np.linspace(0, 9, 2001).astype(dt)).ravel()
    assert np.all(np.diff(v) >= 0) and v.min() >= y.min() and v.max() <= y.max()
    k = hermite_ref.pchip_k(x, y).ravel()
    assert np.all(k == 0) and not np.any(np.signbit(k))     # every knot touches a plateau: +0 everywhere


def test_hermite_tables_reproduce_cubics_exactly():
    """CubicHermite with the derivatives of a cubic reproduces it (to rounding), and the Akima end extension is exact
    for a parabola: its derivative at every knot."""
    x = np.cumsum(np.random.default_rng(3).uniform(0.5, 1.5, 12))
    y = (0.5 * x ** 3 - x ** 2 + 2 * x - 1)[:, None]
    k = (1.5 * x ** 2 - 2 * x + 2)[:, None]
    a, b = hermite_ref.build("hermite", x, y, k)
    q = np.linspace(x[0], x[-1], 301)
    assert np.abs(hermite_ref.evaluate(x, y, a, b, q).ravel() - (0.5 * q ** 3 - q ** 2 + 2 * q - 1)).max() < 1e-11
    xe = np.arange(7.0)
    ka = hermite_ref.akima_k(xe, (xe ** 2)[:, None])[0].ravel()
    assert np.array_equal(ka, 2 * xe)
