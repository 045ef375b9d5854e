"""An x axis per lane (`Interp1DBuilder.lane_axes`, ndi_interp1d_create_lane_axes), the part that needs no device: the
mirror's builder errors in the reference's order, `Monotonic` from host arrays with the lowest offending lane named, the
raw C call's refusals (each decided before a device is touched), and the column validation of csrc/host_logic.hpp driven
by a stand-alone C++ program under AddressSanitizer and UBSan."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT


def _xy(n=5, lanes=3, dt=np.float64):
    x = np.cumsum(np.arange(1, n * lanes + 1, dtype=dt).reshape(n, lanes), axis=0)   # every column strictly rising
    return x, np.sin(x).astype(dt)


# ---- the mirror -----------------------------------------------------------------------------------------------------------
def test_shape_errors(pkg):
    x, y = _xy()
    with pytest.raises(pkg.BuilderError.ShapeError):
        pkg.Interp1D.builder(y).lane_axes(x[:, :2]).build()
    with pytest.raises(pkg.BuilderError.ShapeError):
        pkg.Interp1D.builder(y).lane_axes(x[:4]).build()
    with pytest.raises(pkg.BuilderError.ShapeError):
        pkg.Interp1D.builder(y).lane_axes(x[:, 0].copy()).build()
    with pytest.raises(pkg.BuilderError.ShapeError):   # rank first: data of dimension 0
        pkg.Interp1D.builder(np.float64(1.0)).lane_axes(np.float64(1.0)).build()


def test_x_and_lane_axes_together_is_a_value_error(pkg):
    x, y = _xy()
    for b in (pkg.Interp1D.builder(y).x(x[:, 0].copy()).lane_axes(x), pkg.Interp1D.builder(y).lane_axes(x).x(x[:, 0].copy())):
        with pytest.raises(pkg.BuilderError.ValueError, match="lane_axes"):
            b.build()


def test_dtype_and_residence_must_match(pkg):
    x, y = _xy()
    with pytest.raises(TypeError, match="element type"):
        pkg.Interp1D.builder(y).lane_axes(x.astype(np.float32)).build()


@pytest.mark.parametrize("strategy,need", [("Linear", 2), ("Pchip", 2), ("CubicSpline", 3), ("Akima", 3)])
def test_not_enough_data_comes_before_monotonic_and_shape(pkg, strategy, need):
    n = need - 1
    x = np.zeros((n, 2))          # (ties everywhere and, below, the wrong shape: the length is reported first)
    y = np.zeros((n, 3))
    with pytest.raises(pkg.BuilderError.NotEnoughData, match=f"at least {need} data points"):
        pkg.Interp1D.builder(y).lane_axes(x).strategy(getattr(pkg, strategy).new()).build()


def test_hermite_not_enough_data(pkg):
    with pytest.raises(pkg.BuilderError.NotEnoughData):
        pkg.Interp1D.builder(np.zeros((1, 2))).lane_axes(np.zeros((1, 2))).strategy(pkg.CubicHermite.new(np.zeros((1, 2)))).build()


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("how", ["tie", "nan", "falling"])
def test_monotonic_names_the_lowest_offending_lane(pkg, dt, how):
    x, y = _xy(6, 5, dt)
    for lane in (3, 1):      # lane 3 first, then lane 1 as well: the lowest one is named
        if how == "tie":
            x[4, lane] = x[3, lane]
        elif how == "nan":
            x[2, lane] = np.nan
        else:
            x[:, lane] = x[::-1, lane].copy()
        with pytest.raises(pkg.BuilderError.Monotonic) as e:
            pkg.Interp1D.builder(y).lane_axes(x).build()
        assert str(e.value).endswith(f"Values in the x axis need to be strictly monotonic rising (lane {lane})"), str(e.value)


def test_monotonic_comes_before_the_shape(pkg):
    x, y = _xy(6, 5)
    x[1, 2] = x[0, 2]
    with pytest.raises(pkg.BuilderError.Monotonic, match=r"\(lane 2\)"):
        pkg.Interp1D.builder(y[:, :4]).lane_axes(x).build()


def test_monotonic_of_a_rank3_table_counts_flat_lanes(pkg):
    x = np.cumsum(np.ones((4, 2, 3)), axis=0)
    x[2, 1, 1] = x[1, 1, 1]
    with pytest.raises(pkg.BuilderError.Monotonic, match=r"\(lane 4\)"):
        pkg.Interp1D.builder(np.zeros((4, 2, 3))).lane_axes(x).build()


def test_refused_strategies_and_element_types_carry_the_library_message(pkg):
    x, y = _xy()
    with pytest.raises(ValueError, match="periodic"):
        pkg.Interp1D.builder(y).lane_axes(x).strategy(pkg.CubicSpline.new().boundary(pkg.BoundaryCondition.Periodic)).build()
    rows = np.empty((1, 3), dtype=object)
    rows[0, :] = [pkg.RowBoundary.Natural, pkg.RowBoundary.Clamped, pkg.RowBoundary.NotAKnot]
    with pytest.raises(ValueError, match="Individual"):
        pkg.Interp1D.builder(y).lane_axes(x).strategy(
            pkg.CubicSpline.new().boundary(pkg.BoundaryCondition.Individual(rows))).build()
    xi = np.cumsum(np.ones((4, 2), dtype=np.int32), axis=0, dtype=np.int32)
    with pytest.raises(ValueError, match="f32 / f64"):
        pkg.Interp1D.builder(xi.copy()).lane_axes(xi).build()
    xh = np.cumsum(np.ones((4, 2), dtype=np.float16), axis=0, dtype=np.float16)
    with pytest.raises(ValueError, match="f32 / f64"):
        pkg.Interp1D.builder(xh.copy()).lane_axes(xh).build()


def test_a_user_strategy_is_a_type_error(pkg):
    class Mine(pkg.Interp1DStrategyBuilder):
        def build(self, x, data):
            raise AssertionError("not reached")
    x, y = _xy()
    with pytest.raises(TypeError, match="built-in strategy"):
        pkg.Interp1D.builder(y).lane_axes(x).strategy(Mine()).build()


# ---- the raw C call -------------------------------------------------------------------------------------------------------
def _desc(pkg, xs, y, strategy=None, **kw):
    c = pkg._capi
    d = c.Interp1DDesc()
    d.dtype = {np.dtype(np.float32): c.F32, np.dtype(np.float64): c.F64}[y.dtype]
    d.strategy = c.LINEAR if strategy is None else strategy
    d.n, d.lanes, d.x_len = y.shape[0], y.shape[1], y.shape[0]
    d.x = None
    d.data = y.ctypes.data
    d.memspace = c.MEM_HOST
    d.device = 0
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_symbol_is_bound_and_version_unchanged(pkg):
    assert "ndi_interp1d_create_lane_axes" in pkg._capi.SYMBOLS
    assert pkg._capi.lib().ndi_version() == (0 << 16) | 5


def test_c_refusals_come_before_any_device_work(pkg):
    c = pkg._capi
    lib = c.lib()
    x, y = _xy()
    h = C.c_void_p(1234)

    def call(d, xp=x.ctypes.data, dydx=None):
        h.value = 1234
        st = lib.ndi_interp1d_create_lane_axes(C.byref(d) if d is not None else None, xp, dydx, C.byref(h))
        return st, c.last_error()

    st, _ = call(None)
    assert st == c.BAD_ARG
    st, msg = call(_desc(pkg, x, y, dtype=77))
    assert st == c.BAD_ARG and "dtype" in msg and not h.value            # (*out is cleared first)
    for narrow in (2, 3, 4, 5):                                          # i32, i64, f16, bf16
        st, msg = call(_desc(pkg, x, y, dtype=narrow))
        assert st == c.UNSUPPORTED and "f32 / f64" in msg, (narrow, st, msg)
    st, msg = call(_desc(pkg, x, y, x=x.ctypes.data))
    assert st == c.BAD_ARG and "desc->x must be NULL" in msg
    st, msg = call(_desc(pkg, x, y, x_len=4))
    assert st == c.BAD_ARG and "x_len" in msg
    st, msg = call(_desc(pkg, x, y), xp=None)
    assert st == c.BAD_ARG and "x_lanes" in msg
    st, msg = call(_desc(pkg, x, y, strategy=c.CUBIC_HERMITE))
    assert st == c.BAD_ARG and "dydx" in msg
    st, msg = call(_desc(pkg, x, y, strategy=c.PCHIP), dydx=y.ctypes.data)
    assert st == c.BAD_ARG and "dydx" in msg
    st, msg = call(_desc(pkg, x, y, strategy=c.CUBIC_SPLINE, periodic=1))
    assert st == c.UNSUPPORTED and "periodic" in msg
    kinds = np.zeros(3, np.int32)
    vals = np.zeros(3, np.float64)
    st, msg = call(_desc(pkg, x, y, strategy=c.CUBIC_SPLINE, lane_left_kind=kinds.ctypes.data, lane_left_value=vals.ctypes.data,
                         lane_right_kind=kinds.ctypes.data, lane_right_value=vals.ctypes.data))
    assert st == c.UNSUPPORTED and "Individual" in msg
    st, msg = call(_desc(pkg, x[:2], y[:2], strategy=c.AKIMA))
    assert st == c.NOT_ENOUGH_DATA and "at least 3 data points" in msg
    bad = x.copy()
    bad[3, 2] = np.nan
    bad[2, 1] = bad[1, 1]
    st, msg = call(_desc(pkg, bad, y), xp=bad.ctypes.data)
    assert st == c.MONOTONIC and msg == "Values in the x axis need to be strictly monotonic rising (lane 1)"
    assert not h.value


# ---- the column validation of host_logic.hpp, stand-alone under the sanitizers ----------------------------------------------
SRC = os.path.join(ROOT, "tests", "cpp", "test_lane_axes_host.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "test_lane_axes_host")
HDRS = [os.path.join(ROOT, "ndarray-interp_amd", "csrc", f) for f in ("host_logic.hpp", "common.hpp")]


def test_column_validation_under_asan_and_ubsan():
    newest = max(os.path.getmtime(p) for p in [SRC] + HDRS)
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < newest:
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-o", BIN, SRC],
                       check=True, capture_output=True)
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "OK" in r.stdout
