"""An x axis per lane (`Interp1DBuilder.lane_axes`, ndi_interp1d_create_lane_axes) on the device.

The yardstick is the existing code: lane `l` must equal, bit for bit, the shared-axis handle built from column `l` alone
(`reference_order(True)` for CubicSpline) -- its coefficient tables and every evaluated value, zero signs included, compared
on the integer views.  One CubicSpline and one Linear case are also compared per column against the oracle, as the
shared-axis tests are.  Shapes are the smallest at which this code can go wrong: n at each strategy's minimum, 3, 4, 5 and 33
(a binary search that is no power of two), lanes 1, 3 and 65 (more than a wavefront) and a rank-3 table, 1 and 257 queries."""
import ctypes as C

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

UINT = {np.dtype(np.float32): np.uint32, np.dtype(np.float64): np.uint64}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(UINT[a.dtype])


def assert_bits(got, ref, what):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    if not np.array_equal(bits(got), bits(ref)):
        bad = np.argwhere(bits(got) != bits(ref))
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {bad.shape[0]} of {got.size} elements differ in bits; first at {i}: "
                             f"got {got[i]!r} ref {ref[i]!r}")


def columns(n, lanes, dt, seed=0):
    """Knot columns deliberately unlike each other in one table: a linspace on [0, 1]; one shifted to [0.9, 2] so that the
    common range [Lo, Hi] = [0.9, 1] is a sliver; a log-spaced one; a jittered one."""
    rng = np.random.default_rng(1000 * n + lanes + seed)
    x = np.empty((n, lanes), dtype=dt)
    for l in range(lanes):
        kind = l % 4
        if kind == 0:
            c = np.linspace(0.0, 1.0 + l / 64.0, n)
        elif kind == 1:
            c = np.linspace(0.9 - l / 1024.0, 2.0, n)
        elif kind == 2:
            c = np.geomspace(1e-3, 1.5 + l / 64.0, n)
        else:
            c = np.linspace(-0.5, 1.25, n) + np.concatenate([[0.0], rng.uniform(-0.4, 0.4, n - 2) * (1.75 / (n - 1)), [0.0]]) \
                if n > 2 else np.array([-0.5, 1.25])
        x[:, l] = c.astype(dt)
    assert np.all(x[1:] > x[:-1])
    return x


def table(n, lanes, dt, seed=0):
    x = columns(n, lanes, dt, seed)
    rng = np.random.default_rng(7 * n + lanes + seed)
    y = (np.sin(3.0 * x) + rng.uniform(-0.2, 0.2, x.shape)).astype(dt)
    dydx = (3.0 * np.cos(3.0 * x) + rng.uniform(-0.1, 0.1, x.shape)).astype(dt)
    return x, y, dydx


def mixed_boundary(pkg, shape):
    rows = np.empty((1,) + tuple(shape[1:]), dtype=object)
    rows[...] = pkg.RowBoundary.Mixed(pkg.SingleBoundary.FirstDeriv(0.5), pkg.SingleBoundary.SecondDeriv(-1.0))
    return pkg.BoundaryCondition.Individual(rows)   # (identical rows: one global boundary)


STRATEGIES = {
    # name: (minimum length, builder of the strategy from (pkg, dydx, data shape))
    "Linear": (2, lambda pkg, k, sh: pkg.Linear.new()),
    "Pchip": (2, lambda pkg, k, sh: pkg.Pchip.new()),
    "CubicHermite": (2, lambda pkg, k, sh: pkg.CubicHermite.new(k)),
    "Akima": (3, lambda pkg, k, sh: pkg.Akima.new()),
    "CubicSpline": (3, lambda pkg, k, sh: pkg.CubicSpline.new().reference_order(True)),
    "CubicSpline-natural": (3, lambda pkg, k, sh: pkg.CubicSpline.new().reference_order(True).boundary(pkg.BoundaryCondition.Natural)),
    "CubicSpline-clamped": (3, lambda pkg, k, sh: pkg.CubicSpline.new().reference_order(True).boundary(pkg.BoundaryCondition.Clamped)),
    "CubicSpline-mixed": (3, lambda pkg, k, sh: pkg.CubicSpline.new().reference_order(True).boundary(mixed_boundary(pkg, sh))),
}


def build(pkg, name, x, y, dydx, extrapolate=False):
    """(the lane-axes interpolator, [the single-column shared-axis interpolator of every lane])"""
    make = STRATEGIES[name][1]
    it = pkg.Interp1D.builder(y).lane_axes(x).strategy(make(pkg, dydx, y.shape).extrapolate(extrapolate)).build()
    n = y.shape[0]
    xc, yc, kc = (a.reshape(n, -1) for a in (x, y, dydx))
    refs = []
    for l in range(xc.shape[1]):
        col = np.ascontiguousarray(yc[:, l])
        s = make(pkg, np.ascontiguousarray(kc[:, l]), col.shape).extrapolate(extrapolate)
        refs.append(pkg.Interp1D.builder(col).x(np.ascontiguousarray(xc[:, l])).strategy(s).build())
    return it, refs


def ref_rows(refs, q):
    """out[j][l] from the single-column handles for one query array q[j]"""
    return np.stack([r.interp_array(np.ascontiguousarray(q)) for r in refs], axis=1)


def ref_lanewise(refs, q2):
    return np.stack([r.interp_array(np.ascontiguousarray(q2[:, l])) for l, r in enumerate(refs)], axis=1)


def common_queries(x, nq):
    """Queries for the row-wise call, all inside [Lo, Hi]: the ends, their inner neighbours, every knot of every lane that
    lies inside and the midpoints of those; filled up to nq with uniform draws."""
    xc = x.reshape(x.shape[0], -1)
    lo, hi = xc[0].max(), xc[-1].min()
    assert lo < hi
    inside = np.unique(xc[(xc >= lo) & (xc <= hi)])
    q = np.concatenate([[lo, hi, np.nextafter(lo, hi), np.nextafter(hi, lo)], inside, 0.5 * (inside[1:] + inside[:-1])]).astype(x.dtype)
    q = q[(q >= lo) & (q <= hi)]
    rng = np.random.default_rng(q.size)
    if q.size < nq:
        q = np.concatenate([q, rng.uniform(lo, hi, nq - q.size).astype(x.dtype)])
    return np.clip(q, lo, hi), lo, hi


def own_queries(x):
    """A query per lane, (2n - 1, lanes): every knot of the lane, x[n-1][l] included, and the midpoints, row order shuffled
    per lane so that the lanes of a row sit in different intervals."""
    xc = x.reshape(x.shape[0], -1)
    q = np.concatenate([xc, (0.5 * (xc[1:].astype(np.float64) + xc[:-1])).astype(x.dtype)], axis=0)
    q = np.clip(q, xc[0], xc[-1])
    rng = np.random.default_rng(q.shape[0])
    for l in range(q.shape[1]):
        q[:, l] = q[rng.permutation(q.shape[0]), l]
    return q


def shapes_for(name):
    nmin = STRATEGIES[name][0]
    out = [(nmin, (3,)), (4, (1,)), (5, (65,)), (33, (3,)), (5, (2, 3))]
    if nmin == 2:
        out.append((3, (3,)))
    if name in ("Linear", "CubicSpline"):
        out.append((33, (65,)))
    return out


CASES = [(name, n, lanes) for name in STRATEGIES for (n, lanes) in shapes_for(name)]


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("name,n,lanes", CASES)
def test_parity_with_the_single_column_handles(pkg, dt, name, n, lanes):
    L = int(np.prod(lanes))
    x, y, k = (a.reshape((n,) + lanes) for a in table(n, L, dt))
    it, refs = build(pkg, name, x, y, k)
    what = f"{name} n={n} lanes={lanes} {np.dtype(dt).name}"
    assert it.x is x and it.data is y
    if name != "Linear":   # the build value rule
        a, b = it.strategy.coefficients()
        ra = np.concatenate([r.strategy.coefficients()[0] for r in refs], axis=1)
        rb = np.concatenate([r.strategy.coefficients()[1] for r in refs], axis=1)
        assert_bits(a, ra, what + " a")
        assert_bits(b, rb, what + " b")
    # the row-wise call: 257 queries and a single one
    q, lo, hi = common_queries(x, 257)
    assert it.is_in_range(lo) and it.is_in_range(hi) and not it.is_in_range(np.nextafter(lo, dt(-np.inf)))
    got = it.interp_array(q)
    assert got.shape == (q.size,) + lanes
    assert_bits(got.reshape(q.size, L), ref_rows(refs, q), what + " interp_array")
    assert_bits(it.interp_array(q[:1]).reshape(1, L), ref_rows(refs, q[:1]), what + " one query")
    assert_bits(it.interp(q[1]).reshape(1, L), ref_rows(refs, q[1:2]), what + " interp")
    # the lane-wise call: every knot and every midpoint of every lane
    q2 = own_queries(x)
    got2 = it.interp_lanewise(q2.reshape((q2.shape[0],) + lanes))
    assert_bits(got2.reshape(q2.shape[0], L), ref_lanewise(refs, q2), what + " interp_lanewise")
    assert_bits(it.interp_lanewise(q2[:1].reshape((1,) + lanes)).reshape(1, L), ref_lanewise(refs, q2[:1]), what + " one row")


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_scalar_data(pkg, dt):
    """1-D data: one lane, `interp_scalar`."""
    x, y, k = (a.reshape(-1) for a in table(5, 1, dt))
    it = pkg.Interp1D.builder(y).lane_axes(x).strategy(pkg.CubicSpline.new().reference_order(True)).build()
    ref = pkg.Interp1D.builder(y).x(x).strategy(pkg.CubicSpline.new().reference_order(True)).build()
    for q in (x[0], x[2], x[-1], dt(0.4)):
        assert_bits(np.asarray(it.interp_scalar(q)), np.asarray(ref.interp_scalar(q)), f"interp_scalar({q})")


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_against_the_oracle_per_column(pkg, dt):
    n, L = 33, 3
    x, y, _ = table(n, L, dt)
    q, lo, hi = common_queries(x, 257)
    lin = pkg.Interp1D.builder(y).lane_axes(x).build()
    cub = pkg.Interp1D.builder(y).lane_axes(x).strategy(pkg.CubicSpline.new()).build()
    a, b = cub.strategy.coefficients()
    got_lin, got_cub = lin.interp_array(q), cub.interp_array(q)
    for l in range(L):
        xc, yc = np.ascontiguousarray(x[:, l]), np.ascontiguousarray(y[:, l])
        st, ra, rb = oracle.cubic_build(xc, yc)
        assert st == 0
        assert_bits(a[:, l], ra[:, 0], f"oracle a lane {l}")
        assert_bits(b[:, l], rb[:, 0], f"oracle b lane {l}")
        _, _, ref = oracle.interp1d_cubic(xc, yc, ra, rb, q)
        assert_bits(got_cub[:, l], ref[:, 0], f"oracle cubic lane {l}")
        _, _, ref = oracle.interp1d_linear(xc, yc, q)
        assert_bits(got_lin[:, l], ref[:, 0], f"oracle linear lane {l}")


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("name", ["Linear", "CubicSpline", "Pchip"])
def test_first_error_and_buffer_state(pkg, dt, name):
    n, L = 5, 3
    x, y, k = table(n, L, dt)
    it, refs = build(pkg, name, x, y, k)
    q, lo, hi = common_queries(x, 40)
    good = ref_rows(refs, q)
    for bad, at in ((np.nextafter(lo, dt(-np.inf)), 17), (np.nextafter(hi, dt(np.inf)), 0), (dt(np.nan), 39), (dt(np.inf), 5), (dt(-np.inf), 23)):
        qq = q.copy()
        qq[at] = bad
        qq[min(at + 3, 39)] = bad if at + 3 <= 39 else qq[39]      # a later failure too: the lowest index wins
        buf = np.full((40, L), -77.0, dtype=dt)
        with pytest.raises(pkg.InterpolateError.OutOfBounds) as e:
            it.interp_array_into(qq, buf)
        assert e.value.index == at and "is not in range" in str(e.value) and str(e.value).startswith("x = ")
        assert (np.isnan(e.value.value) and np.isnan(bad)) or e.value.value == float(dt(bad))
        assert_bits(buf[:at], good[:at], f"{name} rows before the failing query {at}")
        assert np.all(buf[at:] == dt(-77.0)), "rows at / after the failing query keep the sentinel"
        # device tensors in and out: the same rule
        import torch
        dbuf = torch.full((40, L), -77.0, dtype=torch.float64 if dt == np.float64 else torch.float32, device="cuda:0")
        with pytest.raises(pkg.InterpolateError.OutOfBounds) as e:
            it.interp_array_into(torch.as_tensor(qq, device="cuda:0"), dbuf)
        assert e.value.index == at
        assert_bits(dbuf.cpu().numpy()[:at], good[:at], "device rows before the failing query")
        assert np.all(dbuf.cpu().numpy()[at:] == dt(-77.0))
        # the fresh-output form (interp_array owns its buffer): the kernel tests the queries itself, the report is the same
        for arr in (qq, torch.as_tensor(qq, device="cuda:0")):
            with pytest.raises(pkg.InterpolateError.OutOfBounds) as e:
                it.interp_array(arr)
            assert e.value.index == at
    # and the handle is fine afterwards
    assert_bits(it.interp_array(q), good, "after the failures")


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("name", ["Linear", "CubicSpline", "Akima", "CubicHermite"])
def test_extrapolation_continues_each_lanes_own_end_interval(pkg, dt, name):
    n, L = 5, 3
    x, y, k = table(n, L, dt)
    it, refs = build(pkg, name, x, y, k, extrapolate=True)
    q = np.concatenate([x.reshape(-1), [x.min() - 1.0, x.max() + 1.0, np.nextafter(x[0].max(), dt(-np.inf)), np.nextafter(x[-1].min(), dt(np.inf))],
                        x[0] - 0.125, x[-1] + 0.125]).astype(dt)          # below and above each lane's own range
    assert_bits(it.interp_array(q), ref_rows(refs, q), f"{name} extrapolated rows")
    q2 = np.stack([x[0] - 0.25, x[-1] + 0.25, x[0], x[-1], x[2]]).astype(dt)
    assert_bits(it.interp_lanewise(q2), ref_lanewise(refs, q2), f"{name} extrapolated lane-wise")
    # +-inf is no failure with extrapolation: NaN-ness and everything finite must agree with the single-column handles
    qi = np.array([x[1, 0], np.inf, -np.inf, x[2, 1]], dtype=dt)
    got, ref = it.interp_array(qi), ref_rows(refs, qi)
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    assert_bits(np.where(np.isnan(got), dt(0), got), np.where(np.isnan(ref), dt(0), ref), "infinite queries")
    # a NaN is the one failure: the lowest index, rows before it written
    qn = q.copy()
    qn[7] = np.nan
    qn[11] = np.nan
    buf = np.full((q.size, L), -77.0, dtype=dt)
    with pytest.raises(pkg.Panic) as e:
        it.interp_array_into(qn, buf)
    assert e.value.index == 7
    assert_bits(buf[:7], ref_rows(refs, q[:7]), "rows before the NaN")
    assert np.all(buf[7:] == dt(-77.0))
    q2n = np.tile(q2, (3, 1))
    q2n[4, 2] = np.nan
    buf2 = np.full(q2n.shape, -77.0, dtype=dt)
    with pytest.raises(pkg.Panic) as e:
        it.interp_lanewise_into(q2n, buf2)
    assert e.value.index == 4 * L + 2
    assert_bits(buf2[:4], ref_lanewise(refs, q2n[:4]), "lane-wise rows before the NaN")
    assert np.all(buf2[4:] == dt(-77.0))


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("name", ["Linear", "CubicSpline"])
def test_lanewise_errors_use_each_lanes_own_range(pkg, dt, name):
    n, L = 5, 3
    x, y, k = table(n, L, dt)
    it, refs = build(pkg, name, x, y, k)
    q2 = np.tile(own_queries(x), (2, 1))            # 18 rows, each element inside its own lane's range
    good = ref_lanewise(refs, q2)
    # lane 0's range is [0, 1], lane 1's [0.9, 2]: 1.5 fails in lane 0 and passes in lane 1
    ok = q2.copy()
    ok[6, 1] = dt(1.5)
    assert_bits(it.interp_lanewise(ok)[6, 1:2], refs[1].interp_array(np.array([1.5], dtype=dt)), "inside lane 1 only")
    for (j, l), bad in (((6, 0), dt(1.5)), ((0, 2), np.nextafter(x[0, 2], dt(-np.inf))), ((17, 1), np.nextafter(x[-1, 1], dt(np.inf))),
                        ((9, 1), dt(np.nan)), ((3, 0), dt(np.inf))):
        qq = q2.copy()
        qq[j, l] = bad
        if j + 2 < qq.shape[0]:
            qq[j + 2, 0] = dt(-np.inf)              # a later failure too
        buf = np.full(qq.shape, -77.0, dtype=dt)
        with pytest.raises(pkg.InterpolateError.OutOfBounds) as e:
            it.interp_lanewise_into(qq, buf)
        assert e.value.index == j * L + l and "is not in range" in str(e.value)
        assert_bits(buf[:j], good[:j], "rows before the failing row")
        assert np.all(buf[j:] == dt(-77.0)), "the failing row and all later rows are untouched"
        import torch
        tq = torch.as_tensor(qq, device="cuda:0")
        dbuf = torch.full(qq.shape, -77.0, dtype=tq.dtype, device="cuda:0")
        with pytest.raises(pkg.InterpolateError.OutOfBounds) as e:
            it.interp_lanewise_into(tq, dbuf)
        assert e.value.index == j * L + l
        assert_bits(dbuf.cpu().numpy()[:j], good[:j], "device rows before the failing row")
        assert np.all(dbuf.cpu().numpy()[j:] == dt(-77.0))
        with pytest.raises(pkg.InterpolateError.OutOfBounds) as e:      # the fresh-output form
            it.interp_lanewise(tq)
        assert e.value.index == j * L + l


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_padded_row_strides_through_the_c_call(pkg, dt):
    n, L = 33, 3
    x, y, k = table(n, L, dt)
    it, refs = build(pkg, "CubicSpline", x, y, k)
    q2 = own_queries(x)
    rows, qs, os_ = q2.shape[0], L + 2, L + 5
    qpad = np.full((rows, qs), np.nan, dtype=dt)
    qpad[:, :L] = q2
    out = np.full((rows, os_), -77.0, dtype=dt)
    c = pkg._capi
    opts, info = c.EvalOpts(), c.OobInfo()
    opts.q_memspace = opts.out_memspace = c.MEM_HOST
    st = c.lib().ndi_interp1d_eval_lanewise(it.strategy._h, qpad.ctypes.data, rows, qs, out.ctypes.data, os_, C.byref(opts), C.byref(info))
    assert st == c.OK, c.last_error()
    assert_bits(out[:, :L], ref_lanewise(refs, q2), "padded strides")
    assert np.all(out[:, L:] == dt(-77.0)), "the padding of the output rows is not written"
    qpad[20, 1] = np.nan
    st = c.lib().ndi_interp1d_eval_lanewise(it.strategy._h, qpad.ctypes.data, rows, qs, out.ctypes.data, os_, C.byref(opts), C.byref(info))
    assert st == c.OUT_OF_BOUNDS and info.index == 20 * L + 1 and info.axis == 0 and np.isnan(info.value)


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_device_tensors_in_and_out_and_replicate(pkg, dt):
    import torch
    n, lanes = 33, (2, 3)
    x, y, k = (a.reshape((n,) + lanes) for a in table(n, 6, dt))
    host, refs = build(pkg, "Pchip", x, y, k)
    tx, ty = torch.as_tensor(x, device="cuda:0"), torch.as_tensor(y, device="cuda:0")
    dev = pkg.Interp1D.builder(ty).lane_axes(tx).strategy(pkg.Pchip.new()).build()
    assert dev.x is tx
    q, lo, hi = common_queries(x, 257)
    ref = ref_rows(refs, q).reshape((q.size,) + lanes)
    q2 = own_queries(x)
    ref2 = ref_lanewise(refs, q2).reshape((q2.shape[0],) + lanes)
    for it in (host, dev, host.replicate([0])[0], dev.replicate([0])[0]):
        assert_bits(it.interp_array(q), ref, "host queries")
        out = it.interp_array(torch.as_tensor(q, device="cuda:0"))
        assert out.is_cuda
        assert_bits(out.cpu().numpy(), ref, "device queries")
        assert_bits(it.interp_lanewise(q2.reshape(ref2.shape)), ref2, "host lane-wise queries")
        out2 = it.interp_lanewise(torch.as_tensor(q2.reshape(ref2.shape), device="cuda:0"))
        assert_bits(out2.cpu().numpy(), ref2, "device lane-wise queries")
        a, b = it.strategy.coefficients()
        assert_bits(a, np.concatenate([r.strategy.coefficients()[0] for r in refs], axis=1), "a")
    # a device-resident CubicHermite: the derivatives travel with the data
    tk = torch.as_tensor(k, device="cuda:0")
    herm, hrefs = build(pkg, "CubicHermite", x, y, k)
    dherm = pkg.Interp1D.builder(ty).lane_axes(tx).strategy(pkg.CubicHermite.new(tk)).build()
    assert_bits(dherm.interp_array(q), ref_rows(hrefs, q).reshape(ref.shape), "device CubicHermite")
    assert_bits(herm.interp_array(q), dherm.interp_array(q), "host and device builds agree")


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_no_common_range(pkg, dt):
    """Lo > Hi is allowed: every row-wise query fails, the lane-wise call still serves each lane."""
    x = np.stack([np.linspace(0.0, 1.0, 5), np.linspace(2.0, 3.0, 5)], axis=1).astype(dt)
    y = (x * x).astype(dt)
    it, refs = build(pkg, "CubicSpline", x, y, y)
    assert not it.is_in_range(0.5) and not it.is_in_range(1.5) and not it.is_in_range(2.5)
    for v in (0.5, 1.5, 2.5, 1.0, 2.0):
        with pytest.raises(pkg.InterpolateError.OutOfBounds) as e:
            it.interp_array(np.array([v], dtype=dt))
        assert e.value.index == 0
    q2 = own_queries(x)
    assert_bits(it.interp_lanewise(q2), ref_lanewise(refs, q2), "lane-wise without a common range")


def test_refusals_name_their_reason_and_leave_the_handle_usable(pkg):
    import torch
    dt = np.float64
    x, y, k = table(5, 3, dt)
    it, refs = build(pkg, "CubicSpline", x, y, k)
    q, lo, hi = common_queries(x, 16)
    good = ref_rows(refs, q)
    c = pkg._capi

    def refused(exc, text, fn):
        with pytest.raises(exc) as e:
            fn()
        assert text in str(e.value), str(e.value)
        assert_bits(it.interp_array(q), good, f"after the refusal ({text})")

    def bucketed():
        it.strategy.path = pkg.PATH_BUCKETED
        try:
            it.interp_array(q)
        finally:
            it.strategy.path = pkg.PATH_AUTO

    refused(pkg.DeviceError, "no common interval", bucketed)
    refused(pkg.DeviceError, "no ring evaluation", lambda: it.interp_array_ring(torch.as_tensor(q, device="cuda:0"), 8))
    out = np.zeros((q.size, 3), dtype=dt)
    refused(pkg.DeviceError, "lane-axes handles", lambda: pkg.sharding.interp_array_sharded(it.replicate([0]), q, out=out))
    refused(ValueError, "no derivative handle", lambda: it.derivative(1))
    refused(ValueError, "no antiderivative handle", lambda: it.antiderivative())
    refused(ValueError, "no inverse handle", lambda: it.inverse())
    refused(ValueError, "lane axes", lambda: it.get_index_left_of(0.95))
    refused(ValueError, "lane axes", lambda: it.index_point(1))
    # the raw statuses: NDI_UNSUPPORTED for each, async_launch on the lane-wise call and the bucketed path on it included
    h = it.strategy._h
    q2 = own_queries(x)
    out2 = np.zeros_like(q2)
    info = c.OobInfo()
    for field, value, text in (("async_launch", 1, "async_launch"), ("path", c.PATH_BUCKETED, "no common interval")):
        opts = c.EvalOpts()
        opts.q_memspace = opts.out_memspace = c.MEM_HOST
        setattr(opts, field, value)
        st = c.lib().ndi_interp1d_eval_lanewise(h, q2.ctypes.data, q2.shape[0], 3, out2.ctypes.data, 3, C.byref(opts), C.byref(info))
        assert st == c.UNSUPPORTED and text in c.last_error(), (st, c.last_error())
    opts = c.EvalOpts()
    opts.q_memspace = opts.out_memspace = c.MEM_HOST
    opts.path = c.PATH_BUCKETED
    assert c.lib().ndi_interp1d_eval(h, q.ctypes.data, q.size, out.ctypes.data, 3, C.byref(opts), C.byref(info)) == c.UNSUPPORTED
    new = C.c_void_p()
    for call in (lambda: c.lib().ndi_interp1d_derivative(h, 1, C.byref(new)), lambda: c.lib().ndi_interp1d_antiderivative(h, C.byref(new)),
                 lambda: c.lib().ndi_interp1d_inverse(h, C.byref(new))):
        assert call() == c.UNSUPPORTED and not new.value
    it.strategy.trim()
    assert_bits(it.interp_array(q), good, "after trim")
    assert_bits(it.interp_lanewise(q2), ref_lanewise(refs, q2), "lane-wise after the refusals")
