"""CPU: antiderivative handles at the boundary -- the two new entry points in the header, the ctypes binding, the built
library and the Rust declarations; the refusals that need no handle; and the accuracy of the numerical rule's numpy
restatement (tests/antiderivative_ref.py, what the GPU tests compare the device against bit for bit) against scipy's
antiderivatives and integrals through tests/golden/antiderivative_scipy.npz (tests/golden/gen_antiderivative_golden.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import antiderivative_ref
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

# Largest error of the restatement against f64 scipy over the golden file (F and the integrals), max abs error /
# (max |expected| + 1), as tests/golden/gen_antiderivative_golden.py measured and printed it; the bar is 2 x each.  The
# inputs are fixed and the operations are + - * /, so the factor only covers a numpy build that orders an operation
# differently.
MEASURED = {
    ("float64", "spline"): 7.173e-16,
    ("float64", "pchip"): 1.257e-16,
    ("float64", "akima"): 2.490e-16,
    ("float64", "linear"): 1.463e-16,
    ("float32", "spline"): 9.306e-07,
    ("float32", "pchip"): 5.464e-08,
    ("float32", "akima"): 2.798e-07,
    ("float32", "linear"): 6.219e-08,
}

RULE_LINES = (
    "cubic class:   dy = yr - yl",
    "c1 = (dy + a) * 0.5",
    "c2 = (b - (a + a)) / 3",
    "c3 = (b - a) * 0.25",
    "G(t) = t * (yl + t * (c1 + t * (c2 - t * c3)))",
    "I[i] = dx * (yl + (c1 + (c2 - c3)))",
    "Linear:        c1 = (yr - yl) * 0.5",
    "G(t) = t * (yl + t * c1)",
    "I[i] = dx * (yl + c1)",
    "t = (xq - x[i]) / dx",
    "F(xq) = P[i] + dx * G(t)",
    "S[i] = +0 where i % B == 0, otherwise S[i] = S[i-1] + I[i-1]",
    "T[k] = S[kB + B - 1] + I[kB + B - 1]",
    "O[0] = +0, O[k+1] = O[k] + T[k]",
    "P[i] = O[i / B] + S[i]",
    "B = 256",
    "may differ from P[n-1] by rounding",
)


def golden():
    return np.load(os.path.join(GOLDEN, "antiderivative_scipy.npz"))


def source_tables(source, x, y):
    """(y, a, b) of the source in the inputs' dtype (Linear: a = b = None)"""
    if source == "linear":
        return y, None, None
    if source in SPLINE_KINDS:
        if source == "per":
            y = y.copy()
            y[-1] = y[0]
        st, a, b = oracle.cubic_build(x, y, **SPLINE_KINDS[source])
        assert st == oracle.OK
        return y, a, b
    a, b = hermite_ref.build(source, x, y)
    return y, a, b


# ---- the boundary ------------------------------------------------------------------------------------------------
def test_header_capi_library_and_rust_carry_both_symbols(pkg):
    cap = pkg._capi
    header = open(os.path.join(ROOT, "include", "ndinterp.h")).read()
    assert re.search(r"ndi_status ndi_interp1d_antiderivative\(const ndi_interp1d\* h, ndi_interp1d\*\* out\);", header)
    assert re.search(r"ndi_status ndi_interp1d_integrate\(const ndi_interp1d\* h, const void\* lo, const void\* hi, uint64_t nq,\s+"
                     r"void\* out, uint64_t out_row_stride,\s+const ndi_eval_opts\* opts, ndi_oob_info\* info\);", header)
    for text in RULE_LINES:
        assert text in header, text
    assert "Not provided: antiderivatives" not in header
    lib = C.CDLL(cap.LIB_PATH)
    for name in ("ndi_interp1d_antiderivative", "ndi_interp1d_integrate"):
        assert name in cap.SYMBOLS and hasattr(lib, name), name
    rust = open(os.path.join(ROOT, "rust", "ndarray-interp-hip", "src", "hip_ffi.rs")).read()
    assert "pub fn ndi_interp1d_antiderivative(h: *const ndi_interp1d, out: *mut *mut ndi_interp1d) -> i32;" in rust
    assert re.search(r"pub fn ndi_interp1d_integrate\(\s+h: \*const ndi_interp1d,\s+lo: \*const c_void,\s+hi: \*const c_void,\s+"
                     r"nq: u64,\s+out: \*mut c_void,\s+out_row_stride: u64,\s+opts: \*const ndi_eval_opts,\s+"
                     r"info: \*mut ndi_oob_info,\s+\) -> i32;", rust)
    assert cap.lib().ndi_version() == (0 << 16) | 5     # two new symbols, no new enumerator: no version change
    assert issubclass(pkg.AntiderivativeStrategy, pkg.Interp1DStrategy)
    for name in ("interp_array_into", "finish", "clone", "data_table", "trim", "release", "integrate_into"):
        assert callable(getattr(pkg.AntiderivativeStrategy, name)), name
    assert callable(pkg.Interp1D.antiderivative) and callable(pkg.Interp1D.integrate)
    assert antiderivative_ref.B == 256


def test_refusals_that_need_no_handle(pkg):
    cap, lib = pkg._capi, pkg._capi.lib()
    h = C.c_void_p(1234)
    assert lib.ndi_interp1d_antiderivative(None, C.byref(h)) == cap.BAD_ARG
    assert cap.last_error() == "null handle" and h.value is None       # *out is cleared
    assert lib.ndi_interp1d_antiderivative(None, None) == cap.BAD_ARG and cap.last_error() == "null out pointer"
    buf = np.zeros(4)
    assert lib.ndi_interp1d_integrate(None, buf.ctypes.data, buf.ctypes.data, 4, buf.ctypes.data, 1, None, None) == cap.BAD_ARG
    assert cap.last_error() == "null handle"


def test_mirror_refuses_strategies_without_a_handle(pkg):
    class Mine(pkg.Interp1DStrategy):
        def interp_into(self, interpolator, target, x):
            target[...] = 0

    x = np.array([0.0, 1.0, 2.0])
    with pytest.raises(TypeError, match="antiderivative needs a built-in device strategy"):
        pkg.Interp1D.new_unchecked(x, x.copy(), Mine()).antiderivative()
    with pytest.raises(TypeError, match="antiderivative needs a built-in device strategy"):
        pkg.Interp1D.new_unchecked(x, x.copy(), Mine()).integrate(x[:2], x[1:])
    xi = np.array([0, 1, 2], dtype=np.int16)        # the generic host path (no device handle)
    with pytest.raises(TypeError, match="antiderivative needs a built-in device strategy"):
        pkg.Interp1D.builder(xi.copy()).x(xi).build().antiderivative()
    with pytest.raises(pkg.Panic, match="incompatible shapes"):
        pkg.Interp1D.new_unchecked(x, x.copy(), Mine()).integrate(x[:2], x)


# ---- the restatement against scipy --------------------------------------------------------------------------------
def test_golden_covers_the_cases_the_specification_names():
    g = golden()
    cases = list(g["cases"])
    assert len(cases) == 22 and sum(c.startswith("float32") for c in cases) == 11
    ns, lanes, families, labels = set(), set(), set(), set()
    for cid in cases:
        x, y, q, lo, hi = (g[cid + "/" + k] for k in ("x", "y", "q", "lo", "hi"))
        assert x.dtype == y.dtype == q.dtype == lo.dtype == hi.dtype and y.shape[0] == len(x) and np.all(np.diff(x) > 0)
        nl = len(g[cid + "/labels"])
        assert g[cid + "/expect_F"].shape == g[cid + "/expect_I"].shape == (nl, len(q), y.shape[1])
        assert g[cid + "/expect_F"].dtype == np.float64
        assert np.sum(q < x[0]) == 3 and np.sum(q > x[-1]) == 3
        assert np.any(lo > hi) and np.any(lo == hi) and np.any(lo < hi)
        ns.add(len(x) - 1); lanes.add(y.shape[1]); families.add(cid.split("_")[-1])
        labels |= set(g[cid + "/labels"])
    assert {1, 2, 255, 256, 257, 513, 4095} <= ns and lanes == {1, 2, 3}
    assert families == {"even", "random", "geometric", "jittered"}
    assert labels == set(SPLINE_KINDS) | {"pchip", "akima", "linear"}
    assert os.path.getsize(os.path.join(GOLDEN, "antiderivative_scipy.npz")) <= 256 * 1024


@pytest.mark.parametrize("dt,source", sorted(MEASURED))
def test_rule_matches_scipy(dt, source):
    """max abs error / (max |expected| + 1) per (dtype, source) over every golden case of that pair, F and integrals,
    against 2 x the value the generator measured (MEASURED above; DESIGN.md 4.12 repeats the table)."""
    g = golden()
    bound = 2.0 * MEASURED[(dt, source)]
    assert abs(float(g[f"measured/{dt}/{source}"]) - MEASURED[(dt, source)]) <= 1e-3 * MEASURED[(dt, source)]
    worst, seen = 0.0, 0
    li = antiderivative_ref.lower_index
    for cid in g["cases"]:
        if not cid.startswith(dt):
            continue
        x, y, q, lo, hi = (g[cid + "/" + k] for k in ("x", "y", "q", "lo", "hi"))
        for k, src in enumerate(g[cid + "/labels"]):
            if (src if src not in SPLINE_KINDS else "spline") != source:
                continue
            ys, a, b = source_tables(src, x, y)
            P = antiderivative_ref.prefix(x, ys, a, b)
            assert P.dtype == np.dtype(dt) and P.shape == y.shape and np.all(P[0] == 0) and not np.any(np.signbit(P[0]))
            gotF = antiderivative_ref.evaluate(x, ys, a, b, P, li(x, q), q)
            gotI = antiderivative_ref.integrate(x, ys, a, b, P, li(x, lo), lo, li(x, hi), hi)
            assert gotF.dtype == gotI.dtype == np.dtype(dt)
            assert np.all(gotI[lo == hi] == 0) and not np.any(np.signbit(gotI[lo == hi]))     # F - F = +0
            for got, expect in ((gotF, g[cid + "/expect_F"][k]), (gotI, g[cid + "/expect_I"][k])):
                m = np.isfinite(expect)      # (the periodic spline has no values outside its knots)
                assert m.any()
                err = float(np.abs(got.astype(np.float64) - expect)[m].max() / (np.abs(expect[m]).max() + 1))
                worst = max(worst, err)
                assert err <= bound, (cid, src, err, bound)
            seen += 1
    # 11 cases per dtype: 9 have n >= 3 (4 boundary kinds each; not-a-knot on the 2 even ones with n >= 4)
    assert seen == {"spline": 38, "pchip": 11, "akima": 9, "linear": 11}[source]
    print(f"{dt} {source}: largest error against scipy {worst:.3e}, bound {bound:.3e}")


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_block_structure_is_pinned(dt):
    """A restatement with one serial sum over all intervals, or with B = 128, differs in bits from the contract's on the
    513-interval case: the 256-knot blocks are part of the rule."""
    g = golden()
    cid = f"{np.dtype(dt).name}_n514_L1_even"
    x, y = g[cid + "/x"], g[cid + "/y"]
    for src in ("nat", "pchip", "linear"):
        ys, a, b = source_tables(src, x, y)
        P = antiderivative_ref.prefix(x, ys, a, b)
        Ps = antiderivative_ref.prefix(x, ys, a, b, serial=True)
        P128 = antiderivative_ref.prefix(x, ys, a, b, block=128)
        assert not np.array_equal(P, Ps), src
        assert not np.array_equal(P, P128), src
        assert np.array_equal(P[:257], Ps[:257])     # ... while the first block (O = +0) is the serial sum itself
        tol = 2.0 * 513 * np.finfo(dt).eps * np.abs(antiderivative_ref.intervals(x, ys, a, b)).sum()
        assert np.abs(P.astype(np.float64) - Ps).max() <= tol and np.abs(P.astype(np.float64) - P128).max() <= tol


# The round trip derivative_ref -> antiderivative_ref of the natural spline of every golden case against y - y[0]: largest
# error / (max |y - y[0]| + 1) per dtype and knot family, as the generator measured and printed it; the bar is 2 x each,
# like MEASURED.  The figures are this check's own: on knots with near-coincident neighbours (the random family) a natural
# spline's derivative is orders of magnitude larger than its values, and the sum that returns y - y[0] cancels.
ROUNDTRIP = {
    ("float64", "even"): 1.668e-15,
    ("float64", "random"): 9.930e-14,
    ("float64", "geometric"): 2.148e-15,
    ("float64", "jittered"): 3.254e-15,
    ("float32", "even"): 1.099e-06,
    ("float32", "random"): 1.779e-04,
    ("float32", "geometric"): 1.146e-06,
    ("float32", "jittered"): 1.769e-06,
}


@pytest.mark.parametrize("dt,family", sorted(ROUNDTRIP))
def test_antiderivative_of_the_derivative_returns_the_function(dt, family):
    """derivative_ref applied to a natural spline, then antiderivative_ref, returns y - y[0]: max abs error /
    (max |y - y[0]| + 1) within 2 x the figure the generator measured for this dtype and knot family (ROUNDTRIP)."""
    g = golden()
    bar = 2.0 * ROUNDTRIP[(dt, family)]
    assert abs(float(g[f"measured/{dt}/roundtrip/{family}"]) - ROUNDTRIP[(dt, family)]) <= 1e-3 * ROUNDTRIP[(dt, family)]
    seen = 0
    for cid in g["cases"]:
        x, y = g[cid + "/x"], g[cid + "/y"]
        if not cid.startswith(dt) or not cid.endswith(family) or len(x) < 3:
            continue
        ys, a, b = source_tables("nat", x, y)
        Y, A, B = derivative_ref.derive(x, ys, a, b)
        P = antiderivative_ref.prefix(x, Y, A, B)
        expect = ys.astype(np.float64) - ys[0].astype(np.float64)
        err = float(np.abs(P.astype(np.float64) - expect).max() / (np.abs(expect).max() + 1))
        assert err <= bar, (cid, err, bar)
        seen += 1
    assert seen == {"even": 2, "random": 2, "geometric": 2, "jittered": 3}[family]
