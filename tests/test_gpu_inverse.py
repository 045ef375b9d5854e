"""GPU: inverse handles (ndi_interp1d_inverse).  Rows are compared BIT FOR BIT, zero signs included, with the numpy
restatement of the header's rule (tests/inverse_ref.py) applied to the SOURCE HANDLE'S OWN tables, read back through
data_table() / coefficients().  Arrays: tests/inverse_cases.py -- every source, n in {2, 3, 5, 257}, lanes in {1, 3, 4, 64,
65}, Q in {1, 63, 65, 4097}, rising and falling lanes in one handle, flat runs, queries at node values, one ulp beside
them, at Lo and Hi and in between; monotone hostile data on tests/hostile_inputs.py knots.  The round trip (the shapes of
inverse_cases.TRIP_SHAPES, which are the cases of tests/golden/inverse_scipy.npz) evaluates the source at every returned
x: nothing is out of bounds, and |f(x) - v| stays within the bound of tests/test_inverse_ref.py (2 x the restatement's
worst residual against scipy on those arrays, inverse_cases.MEASURED)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import hostile_inputs
import inverse_cases as ic
import inverse_ref as ir
from conftest import ROOT

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]


def host(v):
    return v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)


def build(pkg, source, x, y):
    """(the interpolator to invert, the interpolator whose {y, a, b} its polynomial is formed from)"""
    B = pkg.Interp1D.builder
    if source in ("linear", "anti_linear"):
        base = B(y).x(x).strategy(pkg.Linear.new()).build()
    elif source == "akima":
        base = B(y).x(x).strategy(pkg.Akima.new()).build()
    elif source == "spline":
        base = B(y).x(x).strategy(pkg.CubicSpline.new().boundary(pkg.BoundaryCondition.Natural)).build()
    else:
        base = B(y).x(x).strategy(pkg.Pchip.new()).build()
    if source == "dpchip":
        d = base.derivative(1)
        return d, d
    if source.startswith("anti_"):
        return base.antiderivative(), base
    return base, base


def device_tables(source, src, base):
    """(cls, N, y, a, b) as inverse_ref.solve takes them, from the handles' own tables"""
    cls = ic.CLASS_OF[source]
    y = base.strategy.data_table()
    a, b = (None, None) if cls in ("linear", "anti_linear") else base.strategy.coefficients()
    if cls in ("linear", "cubic"):
        return cls, y, None, a, b
    return cls, src.strategy.data_table(), y, a, b


def residual_bound(source, dt, N, q):
    """2 x the measured worst |f_scipy(x) - v| / (eps_T max(|nl|, |nr|)) of the restatement, per element (Q, lanes)"""
    _, nl, nr = ir.intervals(N, q)
    scale = np.maximum(np.abs(nl), np.abs(nr)).astype(np.float64)
    return 2.0 * ic.MEASURED[(np.dtype(dt).name, source)] * float(np.finfo(dt).eps) * scale


def round_trip(src, X, q, bound, what):
    """f_l(X[j, l]) against q[j]: one forward evaluation of all returned abscissae, lane l of row (j, l) taken"""
    Q, L = X.shape
    F = src.interp_array(np.ascontiguousarray(X.reshape(-1))).reshape(Q, L, L)     # raises nothing: x is inside the knots
    f = F[:, np.arange(L), np.arange(L)].astype(np.float64)
    err = np.abs(f - q[:, None].astype(np.float64))
    worst = float((err / np.where(bound > 0, bound, 1.0)).max())
    print(f"{what}: round trip, largest |f(x) - v| / bound = {worst:.3f}")
    assert np.all(err <= bound), (what, worst)


def check_case(pkg, source, dt, x, y, q, what, trip=True):
    import torch
    src, base = build(pkg, source, x, y)
    cls, N, ys, a, b = device_tables(source, src, base)
    inv = src.inverse()
    assert isinstance(inv.strategy, pkg.InverseStrategy) and inv.x is src.x
    hostile_inputs.check_bits(inv.strategy.data_table(), N, what + ": data() is N")
    ref, iters = ir.solve(cls, x, N, q, ys, a, b)
    assert iters.max() < ir.K[np.dtype(dt)]
    got = inv.interp_array(q)
    assert got.shape == q.shape + tuple(y.shape[1:]) and got.dtype == np.dtype(dt)
    hostile_inputs.check_bits(got.reshape(ref.shape), ref, what + ": host rows")
    gd = inv.interp_array(torch.as_tensor(q, device="cuda:0"))
    hostile_inputs.check_bits(gd.cpu().numpy().reshape(ref.shape), ref, what + ": device rows")
    i, _, _ = ir.intervals(N, q)
    assert np.all((ref >= x[i]) & (ref <= x[i + 1]))
    if trip:
        round_trip(src, ref, q, residual_bound(source, dt, N, q), what)
    return inv, ref


# ---- rows ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("source", ic.SOURCES)
def test_rows_bit_for_bit_and_round_trip(pkg, dt, source):
    for n, L, Q in ic.shapes_of(source):
        x, y, q = ic.case(source, dt, n, L, Q)
        check_case(pkg, source, dt, x, y, q, f"{source} {n} x {L}, Q = {Q}, {np.dtype(dt).name}", trip=(n, L, Q) in ic.TRIP_SHAPES)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("source", ["linear", "pchip", "spline"])
def test_a_constant_lane_between_a_rising_and_a_falling_one(pkg, dt, source):
    """Lo == Hi == the constant: the one value every lane takes.  The constant lane returns x[n-2] (the search's last i)."""
    n = 9
    x = ic.knots(np.random.default_rng(5), n, dt)
    up = np.linspace(-1.0, 2.0, n)
    y = np.stack([up, np.full(n, 0.25), -up, up * up * up], axis=1).astype(dt)
    q = np.full(65, 0.25, dtype=dt)
    inv, ref = check_case(pkg, source, dt, x, y, q, f"{source} constant lane {np.dtype(dt).name}", trip=False)
    assert np.all(ref[:, 1] == x[n - 2])
    for v in (np.nextafter(dt(0.25), dt(1)), np.nextafter(dt(0.25), dt(-1))):
        with pytest.raises(pkg.InterpolateError.OutOfBounds):
            inv.interp_array(np.array([0.25, v], dtype=dt))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("recipe", ic.HOSTILE_DATA)
@pytest.mark.parametrize("kind", ic.HOSTILE_KNOTS)
def test_hostile_monotone_data(pkg, dt, kind, recipe):
    """clustered knots (neighbouring floats, steps of 1e300 beside them), subnormal increments, a large offset with
    increments of one ulp: Linear and Pchip, and the antiderivative of the offset data on the uneven knots"""
    rng = np.random.default_rng(3)
    for n, L, Q in ((33, 5, 257), (4, 4, 63)):
        x, y = ic.hostile(kind, recipe, dt, n, L)
        for source in ic.hostile_sources(kind, recipe):
            yy = y if source != "anti_pchip" else np.abs(y[:, ::2])      # (rising lanes only: every P starts at +0)
            q = ic.queries(rng, ic.tables(source, x, yy)[1], Q)
            check_case(pkg, source, dt, x, yy, q, f"hostile {kind} {recipe} {source} {n} x {yy.shape[1]} {np.dtype(dt).name}",
                       trip=False)


# ---- errors ---------------------------------------------------------------------------------------------------------------
def _eval(pkg, inv, q, out, stride, *, q_dev, out_dev, async_launch=False, flags=0):
    cap = pkg._capi
    opts = cap.EvalOpts()
    opts.q_memspace = cap.MEM_DEVICE if q_dev else cap.MEM_HOST
    opts.out_memspace = cap.MEM_DEVICE if out_dev else cap.MEM_HOST
    opts.async_launch = int(async_launch)
    opts.flags = flags
    info = cap.OobInfo()
    qp = q.data_ptr() if q_dev else q.ctypes.data
    op = out.data_ptr() if out_dev else out.ctypes.data
    st = cap.lib().ndi_interp1d_eval(inv.strategy._h, qp, len(q), op, stride, C.byref(opts), C.byref(info))
    return st, info, opts


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("source", ["pchip", "anti_linear"])
def test_first_error_rule(pkg, dt, source):
    import torch
    cap = pkg._capi
    n, L, Q = 17, 5, 300
    x, y, q = ic.case(source, dt, n, L, Q)
    src, base = build(pkg, source, x, y)
    cls, N, ys, a, b = device_tables(source, src, base)
    inv = src.inverse()
    lo, hi = ir.common_range(N)
    ref, _ = ir.solve(cls, x, N, q, ys, a, b)
    tdt = torch.float64 if dt == np.float64 else torch.float32
    above, below = np.nextafter(hi, dt(np.inf)), np.nextafter(lo, dt(-np.inf))
    for bad, k, status in ((above, 131, cap.OUT_OF_BOUNDS), (below, 0, cap.OUT_OF_BOUNDS), (dt(np.nan), 77, cap.NAN_QUERY),
                           (dt(np.inf), 299, cap.OUT_OF_BOUNDS)):
        qq = q.copy()
        qq[k] = bad
        if k < Q - 40:
            qq[k + 20] = dt(np.nan)             # a later failure of the other kind: the lowest index is reported
        for q_dev in (False, True):
            for out_dev in (False, True):
                for fresh in (0, cap.EVAL_FRESH_OUTPUT, cap.EVAL_ROWS_AFTER_ERROR_UNSPECIFIED):
                    what = f"{source} bad = {bad} at {k}, q_dev = {q_dev}, out_dev = {out_dev}, flags = {fresh}"
                    qa = torch.as_tensor(qq, device="cuda:0") if q_dev else qq
                    out = torch.full((Q, L + 2), 7.0, dtype=tdt, device="cuda:0") if out_dev else np.full((Q, L + 2), 7.0, dtype=dt)
                    st, info, _ = _eval(pkg, inv, qa, out, L + 2, q_dev=q_dev, out_dev=out_dev, flags=fresh)
                    assert st == status and info.status == status and info.index == k and info.axis == 0, what
                    msg = cap.last_error()
                    if status == cap.NAN_QUERY:
                        assert np.isnan(info.value) and "NaN" in msg and f"query {k}" in msg, (what, msg)
                    else:
                        assert info.value == float(bad) and msg.startswith("v = ") and msg.endswith("is not in range"), (what, msg)
                    if fresh:
                        continue                  # the rows are the caller's to drop: only the report is checked
                    o = host(out)
                    hostile_inputs.check_bits(np.ascontiguousarray(o[:k, :L]), ref[:k], what + ": rows before the index")
                    assert np.all(o[k:] == 7.0) and np.all(o[:, L:] == 7.0), what
        # async_launch + finish: the report comes from finish
        qa = torch.as_tensor(qq, device="cuda:0")
        out = torch.full((Q, L), 7.0, dtype=tdt, device="cuda:0")
        st, info, _ = _eval(pkg, inv, qa, out, L, q_dev=True, out_dev=True, async_launch=True)
        assert st == cap.OK
        fin = cap.OobInfo()
        assert cap.lib().ndi_interp1d_finish(inv.strategy._h, None, C.byref(fin)) == status
        assert fin.index == k and fin.status == status and fin.axis == 0
        o = out.cpu().numpy()
        hostile_inputs.check_bits(np.ascontiguousarray(o[:k]), ref[:k], "async rows before the index")
        assert np.all(o[k:] == 7.0)
        # the Python mirror: the same report as an exception
        if status == cap.OUT_OF_BOUNDS:
            with pytest.raises(pkg.InterpolateError.OutOfBounds, match="^v = .* is not in range$") as e:
                inv.interp_array(qq)
            assert e.value.index == k and e.value.value == float(bad)
        else:
            with pytest.raises(pkg.Panic, match="NaN") as e:
                inv.interp_array(qq)
            assert e.value.index == k
    # the good batch: strided device and host outputs, async + finish, out[1:], a clone, trim
    wide = torch.full((Q, L + 3), 7.0, dtype=tdt, device="cuda:0")
    inv.strategy.interp_array_into(inv, torch.as_tensor(q, device="cuda:0"), wide[:, :L])
    hostile_inputs.check_bits(wide[:, :L].cpu().numpy(), ref, "strided device rows")
    assert bool((wide[:, L:] == 7.0).all())
    hw = np.full((Q, L + 2), 7.0, dtype=dt)
    inv.strategy.interp_array_into(inv, q, hw[:, :L])
    hostile_inputs.check_bits(np.ascontiguousarray(hw[:, :L]), ref, "strided host rows")
    assert np.all(hw[:, L:] == 7.0)
    out = torch.empty((Q, L), dtype=tdt, device="cuda:0")
    inv.strategy.interp_array_into(inv, torch.as_tensor(q, device="cuda:0"), out, async_launch=True)
    inv.strategy.finish()
    hostile_inputs.check_bits(out.cpu().numpy(), ref, "async rows")
    rep = pkg.Interp1D(inv.x, inv.data, inv.strategy.clone(0))
    hostile_inputs.check_bits(rep.strategy.data_table(), N, "clone: node table")
    hostile_inputs.check_bits(rep.interp_array(q).reshape(ref.shape), ref, "clone rows")
    inv.strategy.trim()
    hostile_inputs.check_bits(inv.interp_array(q).reshape(ref.shape), ref, "after trim")
    hostile_inputs.check_bits(inv.interp(q[3]).reshape(-1), ref[3], "interp")
    # either handle may go first
    src.strategy.release(); base.strategy.release()
    hostile_inputs.check_bits(inv.interp_array(q).reshape(ref.shape), ref, "after the source is destroyed")


# ---- creation ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_creation_refuses_lanes_that_are_not_monotone(pkg, dt):
    cap = pkg._capi
    rng = np.random.default_rng(11)
    n, L = 40, 7
    x = ic.knots(rng, n, dt)
    good = ic.data("linear", rng, x, L, dt)
    for source in ("linear", "pchip"):
        for lane, row, nan in ((5, 17, False), (2, 39, True), (0, 0, True), (6, 1, False)):
            y = good.copy()
            kink = lambda l, r: y[r - 1, l] - np.sign(y[-1, l] - y[0, l]) * dt(10)      # noqa: E731  against the lane's direction
            y[3, 6] = kink(6, 3)                  # lane 6 is never monotone: the LOWEST failing lane is named
            y[row, lane] = np.nan if nan else kink(lane, row)
            why = "holds a NaN" if nan else "both rises and falls"
            src, _ = build(pkg, source, x, y)
            h = C.c_void_p(99)
            assert cap.lib().ndi_interp1d_inverse(src.strategy._h, C.byref(h)) == cap.MONOTONIC and h.value is None
            msg = cap.last_error()
            name = "Linear" if source == "linear" else "Pchip"
            assert msg.startswith(f"inverse of {name}: lane {lane} of the node table {why}"), msg
            with pytest.raises(pkg.BuilderError.Monotonic, match=f"lane {lane} "):
                src.inverse()
    # an antiderivative of data that changes sign: P rises and falls
    y = good.copy()
    src, _ = build(pkg, "anti_linear", x, y)
    with pytest.raises(pkg.BuilderError.Monotonic, match="inverse of the antiderivative of Linear: lane 0 .* both rises and falls"):
        src.inverse()


@pytest.mark.parametrize("dt", DTYPES)
def test_one_lane_of_100001_knots(pkg, dt):
    """1 x 100001: the check runs over knots in parallel (1563 runs of 64), and the search is 17 levels deep"""
    n = 100001
    rng = np.random.default_rng(13)
    x = np.arange(n).astype(dt)
    inc = rng.uniform(0.0, 1.0, n - 1)
    inc[rng.random(n - 1) < 0.2] = 0.0
    y = np.concatenate([[0.0], np.cumsum(inc)])[:, None].astype(dt)
    q = ic.queries(rng, y, 65)
    check_case(pkg, "linear", dt, x, y, q, f"linear 100001 x 1 {np.dtype(dt).name}", trip=False)
    check_case(pkg, "pchip", dt, x, y, q, f"pchip 100001 x 1 {np.dtype(dt).name}", trip=False)
    for row, value in ((64 * 700 + 63, None), (99999, np.nan), (100000, None)):     # a run's last pair, the last run
        bad = y.copy()
        bad[row, 0] = value if value is not None else bad[row - 1, 0] - dt(1)
        src, _ = build(pkg, "linear", x, bad)
        with pytest.raises(pkg.BuilderError.Monotonic, match="lane 0 "):
            src.inverse()


def test_refusals_on_handles(pkg):
    import torch
    cap, lib = pkg._capi, pkg._capi.lib()
    x = np.arange(8.0)
    y = np.stack([x * x, -x], axis=1)
    out = C.c_void_p(99)
    xi = torch.arange(6, dtype=torch.int32, device="cuda:0")
    with pytest.raises(ValueError, match="inverse: an integer handle is a Linear interpolator"):
        pkg.Interp1D.builder(xi * 3).x(xi).build().inverse()
    xh = torch.arange(6, dtype=torch.float16, device="cuda:0")
    with pytest.raises(ValueError, match="inverse: an f16 / bf16 handle is a Linear interpolator"):
        pkg.Interp1D.builder(xh * 0.5).x(xh).build().inverse()
    yp = y.copy(); yp[-1] = yp[0]
    per = pkg.Interp1D.builder(yp).x(x).strategy(
        pkg.CubicSpline.new().boundary(pkg.BoundaryCondition.Periodic).extrapolate(True)).build()
    assert lib.ndi_interp1d_inverse(per.strategy._h, C.byref(out)) == cap.BAD_ARG and out.value is None
    assert cap.last_error().startswith("inverse of CubicSpline: the Periodic extrapolation mode has no inverse handle")
    with pytest.raises(ValueError, match="inverse of CubicSpline: the Periodic extrapolation mode"):
        per.inverse()
    sp = pkg.Interp1D.builder(y).x(x).strategy(pkg.Pchip.new().extrapolate(True)).build()
    assert lib.ndi_interp1d_inverse(sp.strategy._h, None) == cap.BAD_ARG and cap.last_error() == "null out pointer"
    inv = sp.inverse()
    s = inv.strategy
    # `extrapolate` of the source is ignored: outside the node range there is no inverse
    with pytest.raises(pkg.InterpolateError.OutOfBounds, match="^v = 50.0 is not in range$"):
        inv.interp_array(np.array([50.0]))
    for call, text in ((s.inverse, "inverse: this handle is already the inverse of Pchip"),
                       (s.coefficients, "coefficients: the inverse of Pchip is no piecewise polynomial"),
                       (s.derivative, "derivative: the inverse of Pchip is no piecewise polynomial"),
                       (s.antiderivative, "antiderivative: the inverse of Pchip is no piecewise polynomial"),
                       (inv.inverse, "inverse: this handle is already the inverse of Pchip")):
        with pytest.raises(ValueError, match=text):
            call()
    q = np.array([0.0, -1.0]); buf = np.zeros((2, 2))
    opts = cap.EvalOpts(); opts.q_memspace = cap.MEM_HOST; opts.out_memspace = cap.MEM_HOST
    info = cap.OobInfo()
    assert lib.ndi_interp1d_integrate(s._h, q.ctypes.data, q.ctypes.data, 2, buf.ctypes.data, 2, C.byref(opts), C.byref(info)) == cap.BAD_ARG
    assert cap.last_error().startswith("integrate: the inverse of Pchip is no antiderivative handle")
    ring = cap.RingDesc(); ring.chunk_queries = 2; ring.n_slots = 2; ring.row_stride = 2
    ropts = cap.EvalOpts(); ropts.q_memspace = cap.MEM_HOST; ropts.out_memspace = cap.MEM_DEVICE
    assert lib.ndi_interp1d_eval_ring(s._h, q.ctypes.data, 2, C.byref(ring), C.cast(None, cap.RING_CONSUMER), None,
                                      C.byref(ropts), C.byref(info)) == cap.UNSUPPORTED
    assert "an inverse handle (of Pchip) has no ring evaluation" in cap.last_error()
    opts.path = cap.PATH_BUCKETED
    assert lib.ndi_interp1d_eval(s._h, q.ctypes.data, 2, buf.ctypes.data, 2, C.byref(opts), C.byref(info)) == cap.UNSUPPORTED
    assert cap.last_error().startswith("NDI_PATH_BUCKETED: an inverse handle (of Pchip)")
    rep = s.clone(0)
    with pytest.raises(Exception, match="do not take inverse handles"):
        pkg.sharding.interp_array_sharded([pkg.Interp1D(x, inv.data, s), pkg.Interp1D(x, inv.data, rep)], np.linspace(-6.0, 0.0, 64))
    with pytest.raises(Exception, match="must be replicas of one interpolator"):
        pkg.sharding.interp_array_sharded([sp, pkg.Interp1D(x, inv.data, rep)], np.linspace(-6.0, 0.0, 64))
    # an antiderivative handle keeps its other refusals and gains inverse()
    F = pkg.Interp1D.builder(np.abs(y)).x(x).strategy(pkg.Pchip.new()).build().antiderivative()
    with pytest.raises(ValueError, match="this handle is already the antiderivative of Pchip"):
        F.strategy.antiderivative()
    assert isinstance(F.inverse().strategy, pkg.InverseStrategy)


# ---- the bounds-checked library ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", ["linear", "pchip", "anti_pchip", "anti_linear"])
def test_one_case_per_class(pkg, source):
    """one case per evaluation class, rows longer and shorter than a wavefront: with the 100001-knot test this is what runs
    again under the bounds-checked library (below)"""
    for dt, (n, L, Q) in ((np.float64, (257, 65, 63)), (np.float32, (5, 4, 65))):
        x, y, q = ic.case(source, dt, n, L, Q)
        check_case(pkg, source, dt, x, y, q, f"{source} {n} x {L} {np.dtype(dt).name}", trip=False)


def test_the_bounds_checked_library_runs_clean():
    from test_gpu_checked_build import _ensure_debug_library
    _ensure_debug_library()
    env = dict(os.environ, NDI_LIB="libndinterp_hip_dbg.so")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_inverse.py"), "-m", "gpu", "-x", "-q",
                        "-k", "test_one_case_per_class or test_one_lane_of_100001_knots"],
                       capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "failed" not in r.stdout.splitlines()[-1]
