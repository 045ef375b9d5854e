"""GPU: 2-D lane-wise evaluation (ndi_interp2d_eval_lanewise): an (x, y) per channel, out[j, l] = f_l(xs[j, l], ys[j, l]).  Every
row is compared BIT FOR BIT, zero signs included (hostile_inputs.check_bits), and the yardstick is always code that exists
without this entry point: `interp_array` of the same handle -- column l of the result against
`interp_array(xs[:, l], ys[:, l])[:, l]` (per_lane), or, for rows too wide for `lanes` row-wise calls, ONE row-wise call on a
pool of points whose rows are gathered per element (pool_case).  Bicubic cases run under NDI_LANEWISE2D_RECORDS 0 (the plain
node table) and 1 (the node-record copy), and every case asserts the plan line (NDI_TRACE_PLAN) of the call under test."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import hostile_inputs
import inverse_cases as ic
from conftest import ROOT
from test_gpu_lanewise import lane_queries

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
BLOCK = 256          # threads of a workgroup of every lane-wise kernel (csrc/kernels.hpp)
SENTINEL = 7.0
PLAN = re.compile(r"\[ndi plan\] lanewise2d kind=(\w+) stage=(\d) records=(\d) nu=(\d),(\d) wrap=(\w+) check=(\d) grid=(\d+) "
                  r"layout=(\w+)")
FIELDS = ("kind", "stage", "records", "nu_x", "nu_y", "wrap", "check", "grid", "layout")
BICUBIC_KINDS = ("spline", "natural", "pchip", "akima", "hermite")


def tdt(dt):
    import torch
    return torch.float64 if np.dtype(dt) == np.float64 else torch.float32


def host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else a


# ---- handles ------------------------------------------------------------------------------------------------------------------
def axis(kind, rng, n, dt):
    """even: the O(1) guess of the search; clustered: uneven steps, one in five twenty times shorter"""
    return np.arange(n).astype(dt) if kind == "even" else ic.knots(rng, n, dt)


def surface(pkg, kind, x, y, z, extrapolate=False, periodic=0):
    """the interpolator of a source name: 'bilinear', the Bicubic builds, 'dAB' = the partial (A, B) of the spline"""
    B = pkg.Interp2D.builder
    if kind == "bilinear":
        return B(z).x(x).y(y).strategy(pkg.Bilinear.new().extrapolate(extrapolate)).build()
    if kind.startswith("d"):
        return surface(pkg, "spline", x, y, z, extrapolate, periodic).partial(int(kind[1]), int(kind[2]))
    if kind == "hermite":
        tabs = surface(pkg, "spline", x, y, z).strategy.tables()
        return B(z).x(x).y(y).strategy(pkg.Bicubic.hermite(*tabs).extrapolate(extrapolate)).build()
    s = {"spline": pkg.Bicubic.new, "natural": pkg.Bicubic.new, "pchip": pkg.Bicubic.pchip, "akima": pkg.Bicubic.akima}[kind]()
    if kind == "natural":
        s = s.boundary_x(pkg.BoundaryCondition.Natural)       # (x natural, y not-a-knot: two boundary kinds in one handle)
    if periodic & 1:
        s = s.periodic_x()
    if periodic & 2:
        s = s.periodic_y()
    return B(z).x(x).y(y).strategy(s.extrapolate(extrapolate)).build()


def is_bicubic(it):
    return type(it.strategy).__name__ == "Bicubic"


def per_lane(it, xs, ys):
    """the yardstick: column l of the result is interp_array(xs[:, l], ys[:, l])[:, l] -- L row-wise evaluations of the handle"""
    Q, L = xs.shape
    ref = np.empty((Q, L), xs.dtype)
    for l in range(L):
        ref[:, l] = it.interp_array(np.ascontiguousarray(xs[:, l]), np.ascontiguousarray(ys[:, l])).reshape(Q, L)[:, l]
    return ref


def pool_case(it, x, y, Q, L, seed, K=16):
    """(xs, ys, ref) for rows too wide for per_lane: K points -- the four corners of the range, an interior node, its
    neighbouring floats, uniform draws -- evaluated by ONE row-wise call, rows = interp_array(px, py) of shape (K, L); the
    queries are (px, py)[k[j, l]] with k random and the reference is rows[k[j, l], l].  K < 7: the first K of the fixed
    points (K = 4: the corners)"""
    dt = x.dtype
    T = dt.type
    rng = np.random.default_rng(seed)
    xi, yi = x[len(x) // 2], y[len(y) // 2]
    px = np.concatenate([[x[0], x[0], x[-1], x[-1], xi, np.nextafter(xi, T(np.inf)), np.nextafter(xi, T(-np.inf))],
                         rng.uniform(x[0], x[-1], max(K - 7, 0))]).astype(dt)[:K]
    py = np.concatenate([[y[0], y[-1], y[0], y[-1], yi, np.nextafter(yi, T(-np.inf)), np.nextafter(yi, T(np.inf))],
                         rng.uniform(y[0], y[-1], max(K - 7, 0))]).astype(dt)[:K]
    px, py = np.clip(px, x[0], x[-1]), np.clip(py, y[0], y[-1])
    rows = it.interp_array(px, py).reshape(K, L)
    k = rng.integers(0, K, (Q, L))
    k[0, :min(K, L)] = np.arange(min(K, L))                    # every pool point at least once
    return px[k], py[k], np.take_along_axis(rows, k, axis=0)


def grid_data(rng, nx, ny, L, dt):
    return rng.normal(size=(nx, ny, L)).astype(dt)


def queries(rng, x, y, Q, L):
    """lane_queries of the 1-D tests per axis: per lane and independently permuted, both end knots of each axis, every
    interior knot and the floats one ulp either side of it, uniform values between"""
    return lane_queries(rng, x, Q, L), lane_queries(rng, y, Q, L)


# ---- the call under test, with its plan line -------------------------------------------------------------------------------------
class traced:
    """the lanewise2d plan lines (as dicts) and the 'records built' lines of the calls inside"""

    def __init__(self, capfd):
        self.capfd = capfd

    def __enter__(self):
        self.before = os.environ.get("NDI_TRACE_PLAN")
        os.environ["NDI_TRACE_PLAN"] = "1"
        self.capfd.readouterr()
        return self

    def __exit__(self, *a):
        if self.before is None:
            os.environ.pop("NDI_TRACE_PLAN", None)
        else:
            os.environ["NDI_TRACE_PLAN"] = self.before
        err = self.capfd.readouterr().err
        self.plans = [{k: v if k in ("kind", "wrap", "layout") else int(v) for k, v in zip(FIELDS, m.groups())}
                      for m in PLAN.finditer(err)]
        self.built = sum("[ndi plan] lanewise2d records built" in ln for ln in err.splitlines())


def expect(plans, what, n=None, **fields):
    assert plans, f"{what}: no lanewise2d plan line"
    if n is not None:
        assert len(plans) == n, (what, plans)
    for p in plans:
        for k, v in fields.items():
            assert p[k] == v, f"{what}: plan field {k} = {p[k]!r}, expected {v!r} in {p}"


def run(pkg, monkeypatch, capfd, it, xs, ys, ref, what, device=True, **fields):
    """host arrays and device tensors through interp_lanewise (its own output: the kernel tests the queries, check=1) and a
    device call into a caller's buffer (the pre-pass: check=0), under both record settings for a Bicubic handle; bits and
    the plan line of every call.  Returns the last plan."""
    import torch
    bic = is_bicubic(it)
    fields = dict(fields, kind="bicubic" if bic else "bilinear")
    if bic:
        fields.setdefault("nu_x", it.strategy.orders[0])
        fields.setdefault("nu_y", it.strategy.orders[1])
    last = None
    for records in ((0, 1) if bic else (0,)):
        monkeypatch.setenv("NDI_LANEWISE2D_RECORDS", str(records))
        w = f"{what}, records = {records}"
        with traced(capfd) as t:
            got = it.interp_lanewise(xs, ys)
        expect(t.plans, w + ": host", n=1, records=records, check=1, **fields)
        assert isinstance(got, np.ndarray) and got.shape == xs.shape and got.dtype == xs.dtype
        hostile_inputs.check_bits(got, ref, w + ": host")
        if not device:
            last = t.plans[-1]
            continue
        dx, dy = torch.as_tensor(xs, device="cuda:0"), torch.as_tensor(ys, device="cuda:0")
        with traced(capfd) as t:
            got = it.interp_lanewise(dx, dy)
        expect(t.plans, w + ": device", n=1, records=records, check=1, **fields)
        assert got.is_cuda and tuple(got.shape) == xs.shape
        hostile_inputs.check_bits(got.cpu().numpy(), ref, w + ": device")
        buf = torch.full(xs.shape, SENTINEL, dtype=tdt(xs.dtype), device="cuda:0")
        with traced(capfd) as t:
            it.interp_lanewise_into(dx, dy, buf)
        expect(t.plans, w + ": into", n=1, records=records, check=0, **fields)
        hostile_inputs.check_bits(buf.cpu().numpy(), ref, w + ": into a caller's buffer")
        last = t.plans[-1]
    monkeypatch.delenv("NDI_LANEWISE2D_RECORDS")
    return last


def raw_call(pkg, it, qx, qy, nq, q_stride, out, out_stride, *, q_dev, out_dev, flags=0, path=0, async_launch=0, reserved=0):
    cap = pkg._capi
    opts = cap.EvalOpts()
    opts.q_memspace = cap.MEM_DEVICE if q_dev else cap.MEM_HOST
    opts.out_memspace = cap.MEM_DEVICE if out_dev else cap.MEM_HOST
    opts.flags = flags
    opts.path = path
    opts.async_launch = async_launch
    opts.reserved = reserved
    info = cap.OobInfo()

    def ptr(a, on_dev):
        return None if a is None else (a.data_ptr() if on_dev else a.ctypes.data)
    st = cap.lib().ndi_interp2d_eval_lanewise(it.strategy._h, ptr(qx, q_dev), ptr(qy, q_dev), nq, q_stride, ptr(out, out_dev),
                                              out_stride, C.byref(opts), C.byref(info))
    return st, info


# ---- broadcast identity -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("kind", ["bilinear", "spline", "pchip", "akima", "hermite", "d11"])
def test_broadcast_identity(pkg, monkeypatch, capfd, dt, kind):
    """the same (x, y) in every lane of a row: interp_array's row"""
    rng = np.random.default_rng(1)
    nx, ny, L, Q = 9, 7, 7, 301
    x, y = ic.knots(rng, nx, dt), ic.knots(rng, ny, dt)
    it = surface(pkg, kind, x, y, grid_data(rng, nx, ny, L, dt))
    qx, qy = lane_queries(rng, x, Q, 1)[:, 0], lane_queries(rng, y, Q, 1)[:, 0]
    ref = it.interp_array(qx, qy)
    wide = lambda q: np.broadcast_to(q[:, None], (Q, L)).copy()       # noqa: E731
    nu = dict(nu_x=1, nu_y=1) if kind == "d11" else dict(nu_x=0, nu_y=0)
    run(pkg, monkeypatch, capfd, it, wide(qx), wide(qy), ref, f"{kind} broadcast {np.dtype(dt).name}", stage=1, wrap="none", **nu)


# ---- a query per lane ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("axes", ["even", "clustered"])
@pytest.mark.parametrize("kind", ["bilinear", "pchip"])
def test_own_query_per_lane(pkg, monkeypatch, capfd, dt, axes, kind):
    """lanes 1, 5, 63, 64 and 65 (a wavefront spans several rows, exactly one, and a row straddles wavefronts); 67 rows, so
    that the element count is no multiple of 64 wherever the lane count allows it"""
    nx, ny, Q = 9, 7, 67
    for L in (1, 5, 63, 64, 65):
        rng = np.random.default_rng([L, np.dtype(dt).itemsize, axes == "even"])
        x, y = axis(axes, rng, nx, dt), axis(axes, rng, ny, dt)
        it = surface(pkg, kind, x, y, grid_data(rng, nx, ny, L, dt))
        xs, ys = queries(rng, x, y, Q, L)
        assert (Q * L) % 64 != 0 or L % 64 == 0
        run(pkg, monkeypatch, capfd, it, xs, ys, per_lane(it, xs, ys), f"{kind} {axes} {nx} x {ny} x {L} {np.dtype(dt).name}",
            stage=1, wrap="none")


def probe_grid(pkg, monkeypatch, capfd):
    """the grid g the element kernel launches with one workgroup per CU on a batch that fills it"""
    import torch
    monkeypatch.setenv("NDI_LANEWISE_WGS", "1")
    x = np.arange(3.0)
    it = surface(pkg, "bilinear", x, x.copy(), np.zeros((3, 3, 256)))
    q = torch.full((4097, 256), 0.5, dtype=torch.float64, device="cuda:0")
    with traced(capfd) as t:
        it.interp_lanewise(q, q)
    expect(t.plans, "probe", n=1)
    g = t.plans[0]["grid"]
    assert g >= 1 and 2 * BLOCK * g <= 4097 * 256, g
    return g


@pytest.mark.parametrize("kind", ["bilinear", "pchip"])
def test_the_loop_runs_twice_with_a_carry(pkg, monkeypatch, capfd, kind):
    """one workgroup per CU (NDI_LANEWISE_WGS=1) and a row of 256 g + 1 lanes for the g of a probe's plan line: the grid step
    is one lane short of a row, so every trip of LanewisePos::advance after the first lane carries; 5 rows are at least two
    trips of every thread.  The yardstick is pool_case."""
    g = probe_grid(pkg, monkeypatch, capfd)
    L, Q = BLOCK * g + 1, 5
    rng = np.random.default_rng(3)
    x, y = ic.knots(rng, 3, np.float64), ic.knots(rng, 3, np.float64)
    it = surface(pkg, kind, x, y, grid_data(rng, 3, 3, L, np.float64))
    xs, ys, ref = pool_case(it, x, y, Q, L, 4)
    p = run(pkg, monkeypatch, capfd, it, xs, ys, ref, f"{kind} 3 x 3 x {L}, one workgroup per CU", stage=1, grid=g)
    assert 2 * BLOCK * p["grid"] <= Q * L and BLOCK * p["grid"] == L - 1, p


# ---- all eight non-zero partial orders -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_every_partial_order(pkg, monkeypatch, capfd, dt):
    """each partial handle against per_lane on the same handle; the queries hold every knot of either axis, i.e. points on
    grid lines, where one-sided second derivatives would differ"""
    rng = np.random.default_rng(5)
    nx, ny, L, Q = 9, 7, 5, 67
    x, y = ic.knots(rng, nx, dt), ic.knots(rng, ny, dt)
    z = grid_data(rng, nx, ny, L, dt)
    src = surface(pkg, "spline", x, y, z)
    xs, ys = queries(rng, x, y, Q, L)
    assert np.isin(x[1:-1], xs).all() and np.isin(y[1:-1], ys).all()
    for nu_x in range(3):
        for nu_y in range(3):
            if nu_x == 0 and nu_y == 0:
                continue
            it = src.partial(nu_x, nu_y)
            run(pkg, monkeypatch, capfd, it, xs, ys, per_lane(it, xs, ys), f"partial ({nu_x}, {nu_y}) {np.dtype(dt).name}",
                nu_x=nu_x, nu_y=nu_y, stage=1, wrap="none")


# ---- both Bilinear layouts ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,layout", [((9, 7, 5), "plain"), ((101, 41, 5), "packed")])
def test_bilinear_layouts(pkg, monkeypatch, capfd, shape, layout):
    """a grid the handle keeps plain and one it pair-packs by its own rule (at most 64 B per grid point, more than 160 KiB in
    all); the packed case holds queries in the last cell of a grid row (yi = ny - 2), which is reached as the second half of
    the last pair"""
    nx, ny, L = shape
    rng = np.random.default_rng(6)
    x, y = ic.knots(rng, nx, np.float64), ic.knots(rng, ny, np.float64)
    it = surface(pkg, "bilinear", x, y, grid_data(rng, nx, ny, L, np.float64))
    Q = 331
    xs, ys = queries(rng, x, y, Q, L)
    ys[:16] = rng.uniform(y[-2], y[-1], (16, L))       # the last cell of a row: its interior ...
    ys[16] = y[-1]                                      # ... and its far edge
    ys[17] = y[-2]
    assert ((ys >= y[-2]) & (ys <= y[-1])).sum() >= 18 * L
    run(pkg, monkeypatch, capfd, it, xs, ys, per_lane(it, xs, ys), f"bilinear {shape} {layout}", layout=layout, stage=1)


# ---- unstaged axes -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["bilinear", "pchip"])
def test_an_axis_beyond_the_lds_budget(pkg, monkeypatch, capfd, kind):
    """20 001 f64 knots (160 KB and the upper level) are more than LDS_STAGE_LIMIT: both pyramids are read from global memory"""
    rng = np.random.default_rng(7)
    nx, ny, L, Q = 20001, 3, 2, 257
    x, y = ic.knots(rng, nx, np.float64), ic.knots(rng, ny, np.float64)
    it = surface(pkg, kind, x, y, grid_data(rng, nx, ny, L, np.float64))
    xs, ys = queries(rng, x, y, Q, L)
    run(pkg, monkeypatch, capfd, it, xs, ys, per_lane(it, xs, ys), f"{kind} 20001 x 3 x 2", stage=0, wrap="none")


# ---- extrapolation -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("kind", ["bilinear", "spline"])
def test_end_cell_extrapolation(pkg, monkeypatch, capfd, dt, kind):
    rng = np.random.default_rng(8)
    nx, ny, L, Q = 9, 7, 5, 67
    x, y = ic.knots(rng, nx, dt), ic.knots(rng, ny, dt)
    it = surface(pkg, kind, x, y, grid_data(rng, nx, ny, L, dt), extrapolate=True)
    xs, ys = queries(rng, x, y, Q, L)
    wx, wy = x[-1] - x[0], y[-1] - y[0]
    xs[:20] = rng.uniform(x[0] - wx, x[-1] + wx, (20, L)).astype(dt)          # outside on x, on y, on both
    ys[10:30] = rng.uniform(y[0] - wy, y[-1] + wy, (20, L)).astype(dt)
    assert (xs < x[0]).any() and (xs > x[-1]).any() and (ys < y[0]).any() and (ys > y[-1]).any()
    run(pkg, monkeypatch, capfd, it, xs, ys, per_lane(it, xs, ys), f"{kind} extrapolate {np.dtype(dt).name}", stage=1, wrap="none")


def periodic_grid(rng, nx, ny, L, dt, axes):
    z = grid_data(rng, nx, ny, L, dt)
    if axes & 1:
        z[-1] = z[0]
    if axes & 2:
        z[:, -1] = z[:, 0]
    return z


def wrap_queries(rng, k, Q, L, wraps):
    """a wrapping axis: several periods out in both directions, exactly k0, kn and kn + period, +-0.0; the other axis: inside"""
    dt = k.dtype
    if not wraps:
        return lane_queries(rng, k, Q, L)
    p = k[-1] - k[0]
    q = rng.uniform(k[0] - 4 * p, k[-1] + 4 * p, (Q, L)).astype(dt)
    for l in range(L):
        special = np.array([k[0], k[-1], k[-1] + p, 0.0, -0.0, k[0] - p, k[-1] + 3 * p], dt)
        q[rng.permutation(Q)[:len(special)], l] = special
    return q


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("axes", [1, 2, 3])
def test_periodic_axes_wrap(pkg, monkeypatch, capfd, dt, axes):
    """a periodic-x, a periodic-y and a doubly periodic Bicubic with extrapolate: the WRAP variant, the wrap field of the plan
    line; the same build without extrapolate wraps nothing (wrap=none)"""
    rng = np.random.default_rng([9, axes])
    nx, ny, L, Q = 9, 7, 5, 67
    x = (ic.knots(rng, nx, dt) - dt(1.5)).astype(dt)              # 0.0 lies inside neither axis' first cell by accident:
    y = (ic.knots(rng, ny, dt) - dt(0.75)).astype(dt)             # the knots straddle it
    z = periodic_grid(rng, nx, ny, L, dt, axes)
    it = surface(pkg, "spline", x, y, z, extrapolate=True, periodic=axes)
    xs, ys = wrap_queries(rng, x, Q, L, axes & 1), wrap_queries(rng, y, Q, L, axes & 2)
    name = {1: "x", 2: "y", 3: "xy"}[axes]
    run(pkg, monkeypatch, capfd, it, xs, ys, per_lane(it, xs, ys), f"periodic {name} {np.dtype(dt).name}", stage=1, wrap=name)
    d = it.partial(1, 0)
    run(pkg, monkeypatch, capfd, d, xs, ys, per_lane(d, xs, ys), f"periodic {name}, partial (1, 0)", stage=1, wrap=name, device=False)
    inside = surface(pkg, "spline", x, y, z, extrapolate=False, periodic=axes)
    xi, yi = queries(rng, x, y, Q, L)
    run(pkg, monkeypatch, capfd, inside, xi, yi, per_lane(inside, xi, yi), f"periodic {name}, no extrapolate", stage=1, wrap="none",
        device=False)


# ---- failures ------------------------------------------------------------------------------------------------------------------------------
def failing_cases(cap, x, y, dt):
    """(name, handle kind, extrapolate, periodic, [(j, l, axis, value)...] planted, the expected (j, l, axis, status))"""
    T = np.dtype(dt).type
    hi_x, lo_y = np.nextafter(x[-1], T(np.inf)), np.nextafter(y[0], T(-np.inf))
    OOB, NANQ = cap.OUT_OF_BOUNDS, cap.NAN_QUERY
    return (
        ("x only", "bilinear", False, 0, [(20, 3, 0, hi_x)], (20, 3, 0, OOB)),
        ("y only", "pchip", False, 0, [(20, 3, 1, lo_y)], (20, 3, 1, OOB)),
        ("both in one element: x is reported", "pchip", False, 0, [(20, 3, 1, lo_y), (20, 3, 0, hi_x)], (20, 3, 0, OOB)),
        ("a lower element fails on y, a higher one on x", "bilinear", False, 0, [(20, 1, 1, lo_y), (20, 4, 0, hi_x), (25, 0, 0, hi_x)],
         (20, 1, 1, OOB)),
        ("NaN without extrapolation", "pchip", False, 0, [(20, 2, 1, T(np.nan)), (31, 0, 0, hi_x)], (20, 2, 1, OOB)),
        ("NaN with extrapolation", "bilinear", True, 0, [(20, 2, 0, T(np.nan)), (20, 3, 1, T(np.nan))], (20, 2, 0, NANQ)),
        ("+inf on a wrapping axis", "spline", True, 3, [(20, 2, 1, T(np.inf)), (22, 0, 0, T(-np.inf))], (20, 2, 1, NANQ)),
        ("-inf on a wrapping axis", "spline", True, 1, [(20, 2, 0, T(-np.inf))], (20, 2, 0, NANQ)),
    )


@pytest.mark.parametrize("dt", DTYPES)
def test_first_error_rule(pkg, monkeypatch, dt):
    """index, value and axis of the report; rows before the failing row equal the reference; the failing row and all later
    rows keep the sentinel -- through host arrays and device tensors, with the pre-pass and without it (there only the rows
    before the failing row are asserted)"""
    import torch
    cap = pkg._capi
    rng = np.random.default_rng(10)
    nx, ny, L, Q = 9, 7, 5, 40
    x = (ic.knots(rng, nx, dt) - dt(1.5)).astype(dt)
    y = (ic.knots(rng, ny, dt) - dt(0.75)).astype(dt)
    for name, kind, extrapolate, periodic, planted, (j1, l1, axis1, status) in failing_cases(cap, x, y, dt):
        it = surface(pkg, kind, x, y, periodic_grid(rng, nx, ny, L, dt, periodic), extrapolate, periodic)
        xs, ys = queries(rng, x, y, Q, L)
        ref = per_lane(it, xs, ys)
        bx, by = xs.copy(), ys.copy()
        for j, l, ax, v in planted:
            (by if ax else bx)[j, l] = v
        value = (by if axis1 else bx)[j1, l1]
        for records in ((0, 1) if kind != "bilinear" else (0,)):
            monkeypatch.setenv("NDI_LANEWISE2D_RECORDS", str(records))
            for q_dev in (False, True):
                for out_dev in (False, True):
                    for flags in (0, cap.EVAL_FRESH_OUTPUT, cap.EVAL_ROWS_AFTER_ERROR_UNSPECIFIED):
                        qx, qy = (torch.as_tensor(a, device="cuda:0") if q_dev else a for a in (bx, by))
                        out = torch.full((Q, L), SENTINEL, dtype=tdt(dt), device="cuda:0") if out_dev else np.full((Q, L), SENTINEL, dt)
                        st, info = raw_call(pkg, it, qx, qy, Q, L, out, L, q_dev=q_dev, out_dev=out_dev, flags=flags)
                        w = f"{name} {np.dtype(dt).name}, records = {records}, q_dev = {q_dev}, out_dev = {out_dev}, flags = {flags}"
                        assert (st, info.index, info.axis, info.status) == (status, j1 * L + l1, axis1, status), \
                            (w, st, info.index, info.axis, cap.last_error())
                        msg = cap.last_error()
                        if np.isnan(value):
                            assert np.isnan(info.value), w
                        else:
                            assert info.value == float(value), (w, info.value)
                        if status == cap.NAN_QUERY:
                            assert "NaN" in msg, (w, msg)
                        else:
                            assert msg.startswith("xy"[axis1] + " = ") and msg.endswith("is not in range"), (w, msg)
                        o = host(out)
                        hostile_inputs.check_bits(o[:j1], ref[:j1], w + ": rows before the failing row")
                        if not (flags and out_dev):
                            assert np.all(o[j1:] == SENTINEL), w
        monkeypatch.delenv("NDI_LANEWISE2D_RECORDS")
        if status == cap.OUT_OF_BOUNDS:        # ... and the mirror's exception
            with pytest.raises(pkg.InterpolateError.OutOfBounds, match="^%s = .* is not in range$" % "xy"[axis1]) as e:
                it.interp_lanewise(bx, by)
            assert (e.value.index, e.value.axis) == (j1 * L + l1, axis1)
            buf = np.full((Q, L), SENTINEL, dt)
            with pytest.raises(pkg.InterpolateError.OutOfBounds):
                it.interp_lanewise_into(bx, by, buf, rows_after_error_unspecified=True)
            hostile_inputs.check_bits(buf[:j1], ref[:j1], name + ": the mirror, rows before the failing row")
        else:
            with pytest.raises(pkg.Panic, match="failed to convert NaN to usize") as e:
                it.interp_lanewise(bx, by)
            assert e.value.index == j1 * L + l1


def test_a_failure_past_the_prepass_first_trip(pkg, capfd):
    """lanewise2d_check_kernel caps its grid at 4096 blocks of 256 threads: with rows of 1 048 577 lanes every element of rows 1
    and 2 is seen in a later trip.  Row 1 fails on y, row 2 (and a higher lane of row 1) on x: y is reported, row 0 is
    written, rows 1 and 2 keep the sentinel."""
    import torch
    cap = pkg._capi
    dt = np.float32
    L, Q = 1_048_577, 3
    rng = np.random.default_rng(11)
    x, y = np.arange(3, dtype=dt), np.arange(3, dtype=dt)
    it = surface(pkg, "bilinear", x, y, grid_data(rng, 3, 3, L, dt))
    xs, ys, ref = pool_case(it, x, y, Q, L, 12)
    ys[1, 7] = 2.5
    xs[1, 900_000] = -1.0
    xs[2, 3] = 3.0
    qx, qy = torch.as_tensor(xs, device="cuda:0"), torch.as_tensor(ys, device="cuda:0")
    out = torch.full((Q, L), SENTINEL, dtype=torch.float32, device="cuda:0")
    with traced(capfd) as t:
        st, info = raw_call(pkg, it, qx, qy, Q, L, out, L, q_dev=True, out_dev=True)
    expect(t.plans, "wide rows", n=1, kind="bilinear", check=0)
    assert (st, info.index, info.axis, info.value) == (cap.OUT_OF_BOUNDS, L + 7, 1, 2.5), (st, info.index, info.axis, info.value)
    assert L + 7 >= 4096 * BLOCK
    o = out.cpu().numpy()
    hostile_inputs.check_bits(o[:1], ref[:1], "row 0")
    assert np.all(o[1:] == SENTINEL)
    # the same report when the kernel tests the queries itself
    st, info = raw_call(pkg, it, qx, qy, Q, L, out, L, q_dev=True, out_dev=True, flags=cap.EVAL_FRESH_OUTPUT)
    assert (st, info.index, info.axis, info.value) == (cap.OUT_OF_BOUNDS, L + 7, 1, 2.5)
    hostile_inputs.check_bits(out[:1].cpu().numpy(), ref[:1], "row 0, fresh")


# ---- strides and staging -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["bilinear", "pchip"])
def test_row_pitches_above_lanes_and_the_empty_batch(pkg, kind):
    """device query and output tensors that are column slices of wider tensors, and a padded host query array, through the C
    ABI; the padding holds NaN (queries) and the sentinel (output) and is neither read nor written; nq == 0 touches nothing"""
    import torch
    cap = pkg._capi
    rng = np.random.default_rng(13)
    nx, ny, L, Q = 9, 7, 5, 67
    dt = np.float64
    x, y = ic.knots(rng, nx, dt), ic.knots(rng, ny, dt)
    it = surface(pkg, kind, x, y, grid_data(rng, nx, ny, L, dt))
    xs, ys = queries(rng, x, y, Q, L)
    ref = per_lane(it, xs, ys)
    px, py = np.full((Q, L + 3), np.nan, dt), np.full((Q, L + 3), np.nan, dt)
    px[:, :L], py[:, :L] = xs, ys
    for q_dev in (False, True):
        for out_dev in (False, True):
            for flags in (0, cap.EVAL_FRESH_OUTPUT):
                qx, qy = (torch.as_tensor(a, device="cuda:0") if q_dev else a for a in (px, py))
                out = torch.full((Q, L + 2), SENTINEL, dtype=tdt(dt), device="cuda:0") if out_dev else np.full((Q, L + 2), SENTINEL, dt)
                st, info = raw_call(pkg, it, qx, qy, Q, L + 3, out, L + 2, q_dev=q_dev, out_dev=out_dev, flags=flags)
                w = f"{kind} strided rows, q_dev = {q_dev}, out_dev = {out_dev}, flags = {flags}"
                assert st == cap.OK and info.status == cap.OK, (w, cap.last_error())
                o = host(out)
                hostile_inputs.check_bits(np.ascontiguousarray(o[:, :L]), ref, w)
                assert np.all(o[:, L:] == SENTINEL), w
    out = np.full((Q, L), SENTINEL, dt)
    st, info = raw_call(pkg, it, None, None, 0, L, None, L, q_dev=False, out_dev=False)
    assert st == cap.OK and info.status == cap.OK
    st, _ = raw_call(pkg, it, xs, ys, 0, L, out, L, q_dev=False, out_dev=False)
    assert st == cap.OK and np.all(out == SENTINEL)
    # any leading rank through the mirror; scalar data takes queries of any shape
    got = it.interp_lanewise(xs[:60].reshape(3, 20, L), ys[:60].reshape(3, 20, L))
    assert got.shape == (3, 20, L)
    hostile_inputs.check_bits(got.reshape(60, L), ref[:60], "rank-3 queries")
    sc = surface(pkg, kind, x, y, grid_data(rng, nx, ny, 1, dt)[:, :, 0])
    qx, qy = rng.uniform(x[0], x[-1], (3, 4)), rng.uniform(y[0], y[-1], (3, 4))
    hostile_inputs.check_bits(sc.interp_lanewise(qx, qy), sc.interp_array(qx, qy), "scalar data")


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------
def test_refusals_on_a_device(pkg):
    import torch
    cap = pkg._capi
    x, y = np.arange(5.0), np.arange(4.0)
    L = 3
    z = np.random.default_rng(14).normal(size=(5, 4, L))
    q = np.full((4, L), 1.5)
    bil, bic = surface(pkg, "bilinear", x, y, z), surface(pkg, "spline", x, y, z)
    for name, it in (("Bilinear", bil), ("Bicubic", bic), ("a Bicubic partial-derivative handle", bic.partial(1, 0))):
        out = np.full((4, L), SENTINEL)
        kw = dict(q_dev=False, out_dev=False)
        st, _ = raw_call(pkg, it, q, q, 4, L, out, L, path=cap.PATH_BUCKETED, **kw)
        assert st == cap.BAD_ARG and cap.last_error().startswith(f"eval_lanewise of {name}: NDI_PATH_BUCKETED"), cap.last_error()
        st, _ = raw_call(pkg, it, q, q, 4, L, out, L, async_launch=1, **kw)
        assert st == cap.UNSUPPORTED and "async_launch is not provided" in cap.last_error()
        st, _ = raw_call(pkg, it, q, q, 4, L - 1, out, L, **kw)
        assert st == cap.BAD_ARG and cap.last_error() == "q_row_stride (2) < lanes (3)"
        st, _ = raw_call(pkg, it, q, q, 4, L, out, L - 1, **kw)
        assert st == cap.BAD_ARG and cap.last_error() == "out_row_stride (2) < lanes (3)"
        for args in ((None, q, out), (q, None, out), (q, q, None)):
            st, _ = raw_call(pkg, it, args[0], args[1], 4, L, args[2], L, **kw)
            assert st == cap.BAD_ARG and cap.last_error() == "null query / output pointer"
        st, _ = raw_call(pkg, it, q, q, 4, L, out, L, flags=64, **kw)
        assert st == cap.BAD_ARG and "unknown bits" in cap.last_error()
        st, _ = raw_call(pkg, it, q, q, 4, L, out, L, reserved=12345, **kw)
        assert st == cap.BAD_ARG and "reserved must be 0" in cap.last_error()
        assert np.all(out == SENTINEL)
    out = np.full((4, L), SENTINEL)
    integ = bic.antiderivative()
    st, _ = raw_call(pkg, integ, q, q, 4, L, out, L, q_dev=False, out_dev=False)
    assert st == cap.BAD_ARG and "integral handle" in cap.last_error() and "per lane is not provided" in cap.last_error()
    with pytest.raises(ValueError, match="the integral of a surface per lane is not provided"):
        integ.interp_lanewise(q, q)
    assert np.all(out == SENTINEL)
    xi, yi = torch.arange(5, dtype=torch.int32, device="cuda:0"), torch.arange(4, dtype=torch.int32, device="cuda:0")
    zi = torch.arange(60, dtype=torch.int32, device="cuda:0").reshape(5, 4, L)
    qi = torch.ones((4, L), dtype=torch.int32, device="cuda:0")
    with pytest.raises(ValueError, match="eval_lanewise: an integer handle is a Bilinear interpolator"):
        pkg.Interp2D.builder(zi).x(xi).y(yi).build().interp_lanewise(qi, qi)
    with pytest.raises(ValueError, match="eval_lanewise: an f16 / bf16 handle is a Bilinear interpolator"):
        pkg.Interp2D.builder(zi.half()).x(xi.half()).y(yi.half()).build().interp_lanewise(qi.half(), qi.half())
    # the mirror's shapes
    with pytest.raises(pkg.Panic, match=r"ShapeError/IncompatibleShape: incompatible shapes expected: \[.., 3\], got: \[4, 2\]"):
        bic.interp_lanewise(np.zeros((4, 2)), np.zeros((4, 2)))
    with pytest.raises(pkg.Panic, match=r"ShapeError/IncompatibleShape: incompatible shapes expected: \[4, 3\], got: \[5, 3\]"):
        bic.interp_lanewise(np.zeros((4, 3)), np.zeros((5, 3)))
    with pytest.raises(pkg.Panic, match=r"ShapeError/IncompatibleShape: incompatible shapes expected: \[2, 4, 3\], got: \[8, 3\]"):
        bic.interp_lanewise_into(np.full((2, 4, 3), 1.5), np.full((2, 4, 3), 1.5), np.zeros((8, 3)))
    with pytest.raises(TypeError, match="buffer has element type float32"):
        bic.interp_lanewise_into(q, q, np.zeros((4, 3), np.float32))


# ---- the record copy's lifecycle ---------------------------------------------------------------------------------------------------------------
def test_records_lifecycle(pkg, monkeypatch, capfd):
    """trim releases the copy and the next call rebuilds it (same bits); a clone builds its own; a partial handle made before
    and one made after the first lane-wise call share the source's copy: one build in all"""
    rng = np.random.default_rng(15)
    nx, ny, L, Q = 9, 7, 5, 67
    x, y = ic.knots(rng, nx, np.float64), ic.knots(rng, ny, np.float64)
    it = surface(pkg, "pchip", x, y, grid_data(rng, nx, ny, L, np.float64))
    xs, ys = queries(rng, x, y, Q, L)
    ref = per_lane(it, xs, ys)
    before = it.partial(1, 0)
    ref_b = per_lane(before, xs, ys)
    monkeypatch.setenv("NDI_LANEWISE2D_RECORDS", "1")

    def call(h, want, what, built):
        with traced(capfd) as t:
            got = h.interp_lanewise(xs, ys)
        expect(t.plans, what, n=1, records=1)
        hostile_inputs.check_bits(got, want, what)
        assert t.built == built, (what, t.built)
    call(it, ref, "first call", 1)
    call(it, ref, "second call", 0)                       # kept
    after = it.partial(0, 2)
    call(before, ref_b, "a partial made before the first call", 0)
    call(after, per_lane(after, xs, ys), "a partial made after it", 0)
    it.strategy.trim()
    call(before, ref_b, "after trim, through the partial", 1)         # released by trim, rebuilt -- for all three
    call(it, ref, "after trim", 0)
    rep = pkg.Interp2D(it.x, it.y, it.data, it.strategy.clone(0))
    call(rep, ref, "clone", 1)                            # the clone's own
    it.strategy.release()
    call(rep, ref, "clone, after the source is destroyed", 0)
    call(before, ref_b, "the partial, after the source is destroyed", 0)


def test_auto_takes_the_measured_decision(pkg, monkeypatch, capfd):
    """DESIGN.md 4.21 with the knob unset: a Bicubic handle takes the node-record copy, Bilinear has none"""
    monkeypatch.delenv("NDI_LANEWISE2D_RECORDS", raising=False)
    rng = np.random.default_rng(17)
    nx, ny, Q = 9, 7, 67
    x, y = ic.knots(rng, nx, np.float32), ic.knots(rng, ny, np.float32)
    for kind, L, records in (("bilinear", 5, 0), ("akima", 5, 1), ("spline", 65, 1), ("d20", 1, 1)):
        it = surface(pkg, kind, x, y, grid_data(rng, nx, ny, L, np.float32))
        xs, ys = queries(rng, x, y, Q, L)
        with traced(capfd) as t:
            got = it.interp_lanewise(xs, ys)
        expect(t.plans, f"AUTO {kind}", n=1, records=records)
        hostile_inputs.check_bits(got, per_lane(it, xs, ys), f"AUTO {kind}")


@pytest.mark.parametrize("dt,nx,records", [(np.float32, 2048, 1), (np.float32, 2049, 0), (np.float64, 1025, 1)])
def test_auto_at_the_f32_table_limit(pkg, monkeypatch, capfd, dt, nx, records):
    """... except an f32 handle whose node table is above 256 MiB: 2048 x 2048 x 4 nodes of 16 bytes are exactly 256 MiB (the
    copy), one grid row more is above it (the plain table); an f64 table of that size takes the copy.  Data drawn on the
    device; the yardstick is per_lane."""
    import torch
    monkeypatch.delenv("NDI_LANEWISE2D_RECORDS", raising=False)
    ny, L, Q = 2048, 4, 67
    g = torch.Generator(device="cuda:0").manual_seed(18)
    z = torch.randn((nx, ny, L), generator=g, device="cuda:0", dtype=tdt(dt))
    x, y = np.arange(nx).astype(dt), np.arange(ny).astype(dt)
    it = pkg.Interp2D.builder(z).x(torch.as_tensor(x, device="cuda:0")).y(torch.as_tensor(y, device="cuda:0")) \
        .strategy(pkg.Bicubic.pchip()).build()
    rng = np.random.default_rng(19)
    xs, ys = rng.uniform(x[0], x[-1], (Q, L)).astype(dt), rng.uniform(y[0], y[-1], (Q, L)).astype(dt)
    with traced(capfd) as t:
        got = it.interp_lanewise(xs, ys)
    expect(t.plans, f"AUTO {nx} x {ny} x {L} {np.dtype(dt).name}", n=1, records=records, kind="bicubic")
    hostile_inputs.check_bits(got, per_lane(it, xs, ys), f"AUTO {nx} x {ny} x {L} {np.dtype(dt).name}")


CAPTURE_CHILD = r"""
import os, sys
os.environ["NDI_TUNE_LIVE"] = "1"
sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, "tests"))
import numpy as np, torch
import __graft_entry__ as g
pkg = g.load_package()
rng = np.random.default_rng(16)
x, y = np.arange(9.0), np.arange(7.0)
it = pkg.Interp2D.builder(rng.normal(size=(9, 7, 5))).x(x).y(y).strategy(pkg.Bicubic.pchip()).build()
xs = torch.as_tensor(rng.uniform(0, 8, (67, 5)), device="cuda:0"); ys = torch.as_tensor(rng.uniform(0, 6, (67, 5)), device="cuda:0")
os.environ["NDI_LANEWISE2D_RECORDS"] = "0"
side = torch.cuda.Stream()
out = torch.zeros((67, 5), dtype=torch.float64, device="cuda:0")
with torch.cuda.stream(side):
    it.interp_lanewise_into(xs, ys, out, fresh=True)              # warm-up on the capture stream: workspace, LDS attribute
    side.synchronize()
    want = out.clone()
    os.environ["NDI_LANEWISE2D_RECORDS"] = "1"
    os.environ["NDI_TRACE_PLAN"] = "1"
    print("CAPTURE BEGIN", file=sys.stderr, flush=True)
    try:
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            try:
                it.interp_lanewise_into(xs, ys, out, fresh=True)  # (the call reads its status back: it cannot complete in a capture)
            except Exception as e:
                print("call:", type(e).__name__, file=sys.stderr)
    except Exception as e:
        print("capture:", type(e).__name__, file=sys.stderr)
    print("CAPTURE END", file=sys.stderr, flush=True)
torch.cuda.synchronize()
got = it.interp_lanewise(xs, ys)
assert torch.equal(got.view(torch.int64), want.view(torch.int64))
print("AFTER OK", file=sys.stderr, flush=True)
"""


def test_no_record_build_during_stream_capture():
    """a call while the stream is being captured reads the plain table (records=0 although the knob asks for the copy) and
    does not build; the first call after the capture builds it.  A child process: the call cannot complete inside a capture
    (it reads its status back), which ends the capture of that process."""
    r = subprocess.run([sys.executable, "-c", CAPTURE_CHILD.format(root=ROOT)], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and "AFTER OK" in r.stderr, r.stdout[-2000:] + r.stderr[-3000:]
    inside = r.stderr.split("CAPTURE BEGIN", 1)[1].split("CAPTURE END", 1)[0]
    plans = PLAN.findall(inside)
    assert len(plans) == 1 and plans[0][FIELDS.index("records")] == "0", inside
    assert "records built" not in inside, inside
    after = r.stderr.split("CAPTURE END", 1)[1]
    assert after.count("lanewise2d records built") == 1 and "records=1" in after, after


# ---- the bounds-checked library ------------------------------------------------------------------------------------------------------------------
def test_checked_cases(pkg, monkeypatch, capfd):
    """what runs again under the bounds-checked library (below): the 256 g + 1-lane row with a carry in every trip, through
    both kinds and both record settings, and the pair-packed Bilinear grid with queries in the last cell of a row"""
    for kind in ("bilinear", "pchip"):
        test_the_loop_runs_twice_with_a_carry(pkg, monkeypatch, capfd, kind)
    monkeypatch.delenv("NDI_LANEWISE_WGS")
    test_bilinear_layouts(pkg, monkeypatch, capfd, (101, 41, 5), "packed")


def test_the_bounds_checked_library_runs_clean():
    """the NDI_CHK on p.j / p.l and on both cell indices is what would catch a bad carry or a cell past the grid"""
    from test_gpu_checked_build import _ensure_debug_library
    _ensure_debug_library()
    env = dict(os.environ, NDI_LIB="libndinterp_hip_dbg.so")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_lanewise2d.py"), "-m", "gpu", "-x", "-q",
                        "-k", "test_checked_cases"],
                       capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
