"""An x axis per lane on hostile inputs: knot spacings at the denormal edge and of order 1e300 (f32: 1e30), data with
signed zeros, infinities and NaN in single entries -- parity with the single-column handle must still hold bit for bit,
NaN payloads aside (there NaN-ness is compared); device-resident axes whose only flaw is in the last lane, found by the
kernel pass; and one case per kernel under the bounds-checked library with no recorded violation.

Then the independent yardsticks of the shared-axis hostile tests, applied per column: the knot tables of
hostile_inputs.lane_axes_cases (every knot kind of the hostile list across the lanes of one table, adjacent floats
included, under the branch, zero, scale and non-finite recipes) against the numpy restatement for the tables and the CPU
oracle fed with those tables for the rows, with extrapolation, from the record copy and from the plain tables; CubicSpline
of every end kind on the same knot tables; columns that are legal but odd (-inf as a first knot, +inf as a last one), the
signed-zero and infinite ties, and a list of flawed tables on which the host validation and the kernel pass must give the
same verdict."""
import os
import subprocess
import sys

import ctypes as C

import numpy as np
import pytest

import hostile_inputs as hostile
import oracle
from conftest import ROOT
from hostile_inputs import check_bits
from test_gpu_lane_axes import STRATEGIES, assert_bits, build, own_queries, ref_lanewise, ref_rows, table

pytestmark = pytest.mark.gpu


def assert_bits_or_nan(got, ref, what):
    got, ref = np.asarray(got), np.asarray(ref)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), f"{what}: NaN-ness differs"
    z = got.dtype.type(0)
    assert_bits(np.where(np.isnan(got), z, got), np.where(np.isnan(ref), z, ref), what)


def check_all(pkg, name, x, y, k, what):
    """tables, the row-wise call on [Lo, Hi] and the lane-wise call on every knot and midpoint, against the columns"""
    it, refs = build(pkg, name, x, y, k)
    if name != "Linear":
        a, b = it.strategy.coefficients()
        assert_bits_or_nan(a, np.concatenate([r.strategy.coefficients()[0] for r in refs], axis=1), what + " a")
        assert_bits_or_nan(b, np.concatenate([r.strategy.coefficients()[1] for r in refs], axis=1), what + " b")
    lo, hi = x[0].max(), x[-1].min()
    if lo <= hi:
        inside = np.unique(x[(x >= lo) & (x <= hi)])
        q = np.unique(np.concatenate([inside, inside[:-1] + 0.5 * (inside[1:] - inside[:-1]), [lo, hi]]).astype(x.dtype))
        q = q[(q >= lo) & (q <= hi)]
        assert_bits_or_nan(it.interp_array(q), ref_rows(refs, q), what + " rows")
    q2 = own_queries(x)
    assert_bits_or_nan(it.interp_lanewise(q2), ref_lanewise(refs, q2), what + " lane-wise")


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("name", list(STRATEGIES))
def test_extreme_spacings(pkg, dt, name):
    n = 6
    fi = np.finfo(dt)
    sub = fi.smallest_subnormal
    big = dt(1e300) if dt == np.float64 else dt(1e30)
    steps = np.array([0, 1, 3, 4, 9, 10], dtype=dt)
    x = np.stack([steps * sub * dt(4),                      # subnormal knots, spacings of a few ulp of zero
                  steps * sub * dt(4) + fi.tiny,            # spacings below the smallest normal, on normal knots
                  steps * big,                              # dx * dx overflows
                  -big + steps * (big / dt(8)),             # large knots, both signs
                  steps * dt(1e-3) + dt(1.0)], axis=1).astype(dt)
    assert np.all(x[1:] > x[:-1])
    rng = np.random.default_rng(5)
    y = rng.uniform(-1.0, 1.0, x.shape).astype(dt)
    k = rng.uniform(-1.0, 1.0, x.shape).astype(dt)
    check_all(pkg, name, x, y, k, f"{name} {np.dtype(dt).name} extreme spacings")


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("name", list(STRATEGIES))
def test_hostile_data_entries(pkg, dt, name):
    n, L = 7, 6
    x, y, k = table(n, L, dt)
    y[2, 0] = dt(0.0)
    y[3, 0] = dt(-0.0)
    y[:, 1] = dt(-0.0)                 # a column of negative zeros: the zero signs of the results
    y[3, 2] = dt(np.inf)
    y[0, 3] = dt(-np.inf)
    y[6, 4] = dt(np.nan)
    y[1, 5] = np.finfo(dt).max
    y[2, 5] = -np.finfo(dt).max
    k[4, 0] = dt(np.nan)
    k[2, 2] = dt(np.inf)
    check_all(pkg, name, x, y, k, f"{name} {np.dtype(dt).name} hostile data")


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("n,rows", [(33, (31, 32)), (130, (63, 64)), (130, (64, 65)), (2, (0, 1))])
@pytest.mark.parametrize("how", ["tie", "nan"])
def test_device_axes_are_checked_by_the_kernel_pass(pkg, dt, n, rows, how):
    """A flaw in the LAST lane only, between two given rows (130 knots: across the edge of a thread's run of 64)."""
    import torch
    L = 65
    x, y, _ = table(n, L, dt)
    if how == "tie":
        x[rows[1], L - 1] = x[rows[0], L - 1]
    else:
        x[rows[1], L - 1] = np.nan
    tx, ty = torch.as_tensor(x, device="cuda:0"), torch.as_tensor(y, device="cuda:0")
    with pytest.raises(pkg.BuilderError.Monotonic) as e:
        pkg.Interp1D.builder(ty).lane_axes(tx).build()
    assert str(e.value).endswith(f"Values in the x axis need to be strictly monotonic rising (lane {L - 1})"), str(e.value)
    x[0, 7] = x[1, 7] if n > 2 else np.nan        # and a lower lane as well: the lowest one is named
    with pytest.raises(pkg.BuilderError.Monotonic, match=r"\(lane 7\)"):
        pkg.Interp1D.builder(ty).lane_axes(torch.as_tensor(x, device="cuda:0")).build()


def test_one_case_per_kernel(pkg, monkeypatch):
    """Every new kernel instance once: the check pass, the spline build (general and parabola rows), the local cubics with
    the per-lane knot accessor, and the evaluation kernel for Linear and the cubic class, row-wise and lane-wise, from the
    plain tables and from the record copy; more elements than one grid-stride trip of a small grid covers."""
    import torch
    for dt in (np.float64, np.float32):
        for name, n in (("Linear", 2), ("CubicSpline", 3), ("CubicSpline-natural", 33), ("Pchip", 33), ("Akima", 5), ("CubicHermite", 4)):
            x, y, k = table(n, 65, dt)
            tx, ty, tk = (torch.as_tensor(a, device="cuda:0") for a in (x, y, k))
            it, refs = build(pkg, name, x, y, k)
            dev = pkg.Interp1D.builder(ty).lane_axes(tx).strategy(STRATEGIES[name][1](pkg, tk, y.shape)).build()
            lo, hi = x[0].max(), x[-1].min()
            q = np.random.default_rng(n).uniform(lo, hi, 1500).astype(dt).clip(lo, hi)
            q2 = np.tile(own_queries(x), (20, 1))
            ref, ref2 = ref_rows(refs, q), ref_lanewise(refs, q2)
            for records in ("0", "1"):
                monkeypatch.setenv("NDI_LANE_AXES_RECORDS", records)
                monkeypatch.setenv("NDI_LANEWISE_WGS", "1")
                for h in (it, dev):
                    assert_bits(h.interp_array(q), ref, f"{name} rows records={records}")
                    assert_bits(h.interp_array(torch.as_tensor(q, device="cuda:0")).cpu().numpy(), ref, f"{name} device rows")
                    assert_bits(h.interp_lanewise(q2), ref2, f"{name} lane-wise records={records}")
                    buf = torch.empty(q2.shape, dtype=tx.dtype, device="cuda:0")
                    h.interp_lanewise_into(torch.as_tensor(q2, device="cuda:0"), buf)     # (with the pre-pass)
                    assert_bits(buf.cpu().numpy(), ref2, f"{name} device lane-wise")


# ---- the hostile list per column: the restatement and the oracle -----------------------------------------------------------------------
HOSTILE_L = 15
HOSTILE_NS = (2, 3, 4, 5, 6, 33)
TWIN_CLASSES = ("branch", "zero", "scale")
RULE_STRATEGY = {"pchip": "Pchip", "akima": "Akima", "hermite": "CubicHermite"}
HOSTILE_CASES = [(rule, n) for rule in hostile.RULES for n in HOSTILE_NS if not (rule == "akima" and n < 3)]


def oracle_columns(x, y, a, b, q, mode):
    """oracle.interp1d_cubic column by column on the tables (a, b): q (Q,) for every lane, or (Q, L) with a query per lane"""
    out = np.empty((q.shape[0], x.shape[1]), x.dtype)
    for l in range(x.shape[1]):
        ql = np.ascontiguousarray(q if q.ndim == 1 else q[:, l])
        out[:, l] = oracle.interp1d_cubic(np.ascontiguousarray(x[:, l]), np.ascontiguousarray(y[:, l]), np.ascontiguousarray(a[:, l:l + 1]),
                                          np.ascontiguousarray(b[:, l:l + 1]), ql, mode)[2][:, 0]
    return out


def check_hostile_columns(pkg, monkeypatch, rule, tag, x, y, k, device=False):
    """one array of lane_axes_cases on an extrapolating handle: the tables against the restatement of each column, the
    lane-wise call on hostile.queries of each lane's own knots and the row-wise call on the union of all lanes' finite
    queries against the oracle fed with the restatement's tables; from the record copy and from the plain tables"""
    make = STRATEGIES[RULE_STRATEGY[rule]][1]
    if device:
        import torch
        tx, ty, tk = (None if v is None else torch.as_tensor(v, device="cuda:0") for v in (x, y, k))
        it = pkg.Interp1D.builder(ty).lane_axes(tx).strategy(make(pkg, tk, y.shape).extrapolate(True)).build()
        tag += " (device arrays)"
    else:
        it = pkg.Interp1D.builder(y).lane_axes(x).strategy(make(pkg, k, y.shape).extrapolate(True)).build()
    a, b = it.strategy.coefficients()
    ra, rb = hostile.lane_axes_reference(rule, x, y, k)
    check_bits(a, ra, tag + ": a")
    check_bits(b, rb, tag + ": b")
    q2 = hostile.lane_axes_queries(x)
    q = np.unique(q2[np.isfinite(q2)])
    assert np.isinf(q2).any() and q.size >= 2 * x.shape[0]
    want2 = oracle_columns(x, y, ra, rb, q2, oracle.EXTRAPOLATE_YES)
    want = oracle_columns(x, y, ra, rb, q, oracle.EXTRAPOLATE_YES)
    for records in ("1", "0"):
        monkeypatch.setenv("NDI_LANE_AXES_RECORDS", records)
        check_bits(it.interp_lanewise(q2), want2, f"{tag}: lane-wise rows, records={records}")
        check_bits(it.interp_array(q), want, f"{tag}: rows, records={records}")


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("rule,n", HOSTILE_CASES, ids=[f"{r}-n{n}" for r, n in HOSTILE_CASES])
def test_hostile_columns_against_the_restatement_and_the_oracle(pkg, monkeypatch, dt, rule, n):
    """hostile_inputs.lane_axes_cases for the three local rules, 15 lanes: column l of part p is knot kind (l + p) mod 5 of the
    hostile list (even, uneven, adjacent floats, steps of 1e30 / 1e300, both), the data the recipe list on the unit grid.
    Beside every array with the inf / NaN recipes its twin without them (tests/test_hostile_inputs.py holds the twins' rows
    to a finite share of 75 %).  At n = 5 the first array is also built from device arrays."""
    seen = 0
    for classes in (hostile.CLASSES, TWIN_CLASSES):
        for tag, x, y, k in hostile.lane_axes_cases(rule, dt, n, HOSTILE_L, classes):
            check_hostile_columns(pkg, monkeypatch, rule, tag, x, y, k)
            if n == 5 and seen == 0:
                check_hostile_columns(pkg, monkeypatch, rule, tag, x, y, k, device=True)
            seen += 1
    assert seen >= 4


SPLINES = [name for name in STRATEGIES if name.startswith("CubicSpline")]


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("extrapolate", [False, True])
@pytest.mark.parametrize("n", [3, 4, 5, 33], ids=lambda n: f"n{n}")
@pytest.mark.parametrize("name", SPLINES)
def test_spline_columns_on_hostile_knots(pkg, dt, name, n, extrapolate):
    """The knot tables of lane_axes_cases (all five kinds across 15 lanes) under the scale recipes, CubicSpline with
    reference_order(True) and each end kind: tables and both calls against the single-column handles, in range and with
    extrapolation; for NotAKnot also against the oracle per column.  The build squares the spacings, so on the huge and mixed
    columns little is finite: what is compared there is where the infinities and NaN fall."""
    mode = oracle.EXTRAPOLATE_YES if extrapolate else oracle.EXTRAPOLATE_NO
    seen = 0
    for tag, x, y, _ in hostile.lane_axes_cases("pchip", dt, n, HOSTILE_L, ("scale",)):
        tag = f"{name} {tag} extrapolate={extrapolate}"
        it, refs = build(pkg, name, x, y, y, extrapolate=extrapolate)
        a, b = it.strategy.coefficients()
        check_bits(a, np.concatenate([r.strategy.coefficients()[0] for r in refs], axis=1), tag + ": a")
        check_bits(b, np.concatenate([r.strategy.coefficients()[1] for r in refs], axis=1), tag + ": b")
        q2 = hostile.lane_axes_queries(x, extrapolate)
        got2 = it.interp_lanewise(q2)
        check_bits(got2, ref_lanewise(refs, q2), tag + ": lane-wise rows")
        lo, hi = x[0].max(), x[-1].min()
        q = np.unique(q2[np.isfinite(q2)])
        if not extrapolate:
            q = q[(q >= lo) & (q <= hi)]
            assert (q.size > 0) == bool(lo <= hi) and it.is_in_range(lo) == bool(lo <= hi)
        got = it.interp_array(q) if q.size else np.empty((0, HOSTILE_L), dt)
        if q.size:
            check_bits(got, ref_rows(refs, q), tag + ": rows")
        else:       # (these tables have no common range -- the uneven columns start above the last adjacent float -- so
            #          without extrapolation the row-wise call refuses every query; the extrapolating case evaluates them)
            with pytest.raises(pkg.InterpolateError.OutOfBounds) as e:
                it.interp_array(np.array([lo, hi], dt))
            assert e.value.index == 0
        if name == "CubicSpline":
            for l in range(HOSTILE_L):
                xc, yc = np.ascontiguousarray(x[:, l]), np.ascontiguousarray(y[:, l])
                st, oa, ob = oracle.cubic_build(xc, yc)
                assert st == oracle.OK
                check_bits(a[:, l], oa[:, 0], f"{tag}: oracle a lane {l}")
                check_bits(b[:, l], ob[:, 0], f"{tag}: oracle b lane {l}")
            check_bits(got2, oracle_columns(x, y, a, b, q2, mode), tag + ": oracle lane-wise rows")
            if q.size:
                check_bits(got, oracle_columns(x, y, a, b, q, mode), tag + ": oracle rows")
        seen += 1
    assert seen >= 1


# ---- columns that are legal but odd ---------------------------------------------------------------------------------------------------
def infinite_end_table(dt):
    """(x, y, dydx, q2): three columns with an infinite end knot, each beside a finite twin; a query per lane on every finite
    knot, the midpoints of the finite intervals and points inside the infinite ones (the twins: outside their range only
    where the handle extrapolates, so they get their own knots and midpoints again)"""
    inf = np.inf
    cols = [[-inf, 0, 1, 2, 3], [-4, 0, 1, 2, 3], [0, 1, 2, 3, inf], [0, 1, 2, 3, 7], [-inf, 0, 1, 2, inf], [-4, 0, 1, 2, 7]]
    x = np.ascontiguousarray(np.array(cols, dtype=dt).T)
    rng = np.random.default_rng(91)
    y = rng.uniform(-1.0, 1.0, x.shape).astype(dt)
    k = rng.uniform(-1.0, 1.0, x.shape).astype(dt)
    per_lane = []
    for l in range(x.shape[1]):
        c = x[:, l]
        f = c[np.isfinite(c)]
        q = [f, 0.5 * (f[1:] + f[:-1])]
        if c[0] == -inf:
            q.append([-1e30, -5.0, np.nextafter(dt(0), dt(-1))])
        if c[-1] == inf:
            q.append([f[-1] + 2.5, 1e30, np.nextafter(f[-1], dt(inf))])
        per_lane.append(np.concatenate(q).astype(dt))
    Q = max(len(q) for q in per_lane)
    q2 = np.stack([np.concatenate([q, np.full(Q - len(q), q[0], dt)]) for q in per_lane], axis=1)
    return x, y, k, np.ascontiguousarray(q2)


def infinite_ends_case(pkg, dt, name):
    import torch
    x, y, k, q2 = infinite_end_table(dt)
    L = x.shape[1]
    lo, hi = dt(0), dt(3)
    assert x[0].max() == lo and x[-1].min() == hi
    q = np.array([0, 0.5, 1, 1.5, 2, 2.5, 3], dt)
    far = np.concatenate([q, [-1e30, -5.0, -4.5, 3.5, 9.5, 1e30]]).astype(dt)      # inside the infinite intervals, outside the twins
    tx, ty, tk = (torch.as_tensor(v, device="cuda:0") for v in (x, y, k))
    for extrapolate in (False, True):
        what = f"{name} {np.dtype(dt).name} infinite end knots, extrapolate={extrapolate}"
        host, refs = build(pkg, name, x, y, k, extrapolate=extrapolate)
        dev = pkg.Interp1D.builder(ty).lane_axes(tx).strategy(STRATEGIES[name][1](pkg, tk, y.shape).extrapolate(extrapolate)).build()
        for it, how in ((host, "host arrays"), (dev, "device arrays")):
            if name != "Linear":
                a, b = it.strategy.coefficients()
                check_bits(a, np.concatenate([r.strategy.coefficients()[0] for r in refs], axis=1), f"{what}, {how}: a")
                check_bits(b, np.concatenate([r.strategy.coefficients()[1] for r in refs], axis=1), f"{what}, {how}: b")
            assert it.is_in_range(lo) and it.is_in_range(hi) and it.is_in_range(dt(1.5))
            assert not it.is_in_range(np.nextafter(lo, dt(-np.inf))) and not it.is_in_range(np.nextafter(hi, dt(np.inf)))
            check_bits(it.interp_lanewise(q2), ref_lanewise(refs, q2), f"{what}, {how}: lane-wise rows")
            rows = far if extrapolate else q
            check_bits(it.interp_array(rows), ref_rows(refs, rows), f"{what}, {how}: rows")
            if not extrapolate:
                for bad in (np.nextafter(lo, dt(-np.inf)), np.nextafter(hi, dt(np.inf))):
                    with pytest.raises(pkg.InterpolateError.OutOfBounds) as e:
                        it.interp_array(np.array([1.0, bad], dt))
                    assert e.value.index == 1


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("name", list(STRATEGIES))
def test_infinite_end_knots(pkg, dt, name):
    """-inf as a first knot and +inf as a last knot pass both validations (a column is strictly rising with no NaN): the
    columns [-inf, 0, 1, 2, 3], [0, 1, 2, 3, +inf] and [-inf, 0, 1, 2, +inf], each beside a finite twin, from host arrays and
    from device arrays.  Tables and both calls agree with the single-column handles where those hold a number and where
    they hold NaN (an infinite interval has t = inf / inf); is_in_range is [Lo, Hi] = [0, 3]."""
    infinite_ends_case(pkg, dt, name)


def raw_create(pkg, x, y, device):
    """ndi_interp1d_create_lane_axes (Linear) on host arrays -- first_bad_lane_axis, before any device work -- or on device
    arrays -- lane_axes_check_kernel: (status, message); a handle that was made is destroyed"""
    from test_lane_axes_abi import _desc
    c = pkg._capi
    d = _desc(pkg, x, y)
    xp = x.ctypes.data
    if device:
        import torch
        tx, ty = torch.as_tensor(x, device="cuda:0"), torch.as_tensor(y, device="cuda:0")
        d.data, d.memspace, xp = ty.data_ptr(), c.MEM_DEVICE, tx.data_ptr()
    h = C.c_void_p()
    st = c.lib().ndi_interp1d_create_lane_axes(C.byref(d), xp, None, C.byref(h))
    msg = c.last_error() if st != c.OK else ""
    if h.value:
        c.lib().ndi_interp1d_destroy(h)
    return st, msg


def flawed_tables(n, dt):
    """(what, x, lane): tables of 5 lanes with one flawed column"""
    L, lane = 5, 3
    base = np.cumsum(np.arange(1, n * L + 1, dtype=np.float64).reshape(n, L), axis=0).astype(dt)
    assert np.all(base[1:] > base[:-1]) and np.all(base > 0)
    inf = dt(np.inf)

    def flawed(rows, values):
        x = base.copy()
        x[list(rows), lane] = values
        return x
    yield "a fall at the first pair", flawed((1,), [base[0, lane] - dt(0.5)]), lane
    yield "a tie at the last pair", flawed((n - 1,), [base[n - 2, lane]]), lane
    yield "NaN at row 0", flawed((0,), [np.nan]), lane
    yield "NaN at row n-1", flawed((n - 1,), [np.nan]), lane
    yield "-0.0, +0.0", flawed((0, 1), [-0.0, 0.0]), lane
    yield "+0.0, -0.0", flawed((0, 1), [0.0, -0.0]), lane
    yield "inf, inf", flawed((n - 2, n - 1), [inf, inf]), lane
    yield "a fall at the last pair", flawed((n - 1,), [np.nextafter(base[n - 2, lane], dt(0))]), lane


def flawed_tables_case(pkg, dt, n):
    c = pkg._capi
    seen = 0
    for what, x, lane in flawed_tables(n, dt):
        y = np.sin(np.arange(x.size, dtype=np.float64)).reshape(x.shape).astype(dt)
        for also in (False, True):
            if also:                        # and a lower lane as well: the lowest one is named
                x = x.copy()
                x[n - 1, 1] = x[n - 2, 1]
                lane = 1
            want = (c.MONOTONIC, f"Values in the x axis need to be strictly monotonic rising (lane {lane})")
            host, dev = raw_create(pkg, x, y, False), raw_create(pkg, x, y, True)
            assert host == want and dev == want, (what, n, np.dtype(dt).name, also, host, dev)
            seen += 1
    clean = next(flawed_tables(n, dt))[1]
    clean[1, 3] = clean[0, 3] + dt(1)
    y = np.zeros_like(clean)
    assert raw_create(pkg, clean, y, False) == (c.OK, "") and raw_create(pkg, clean, y, True) == (c.OK, "")
    assert seen == 16


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("n", [2, 3, 65, 129], ids=lambda n: f"n{n}")
def test_host_and_device_validation_give_the_same_verdict(pkg, dt, n):
    """first_bad_lane_axis (host arrays) and lane_axes_check_kernel (device arrays) on the same flawed tables: the same status
    and the same named lane.  n = 65 and 129: a thread of the kernel walks a run of 64 knots and its pairs reach one knot into
    the next run, so the last run holds a single knot and the pair (n-2, n-1) belongs to the run before it."""
    flawed_tables_case(pkg, dt, n)


def ties_case(pkg, dt):
    import torch
    inf = np.inf
    for col in ([-0.0, 0.0, 1.0], [0.0, -0.0, 1.0], [1.0, inf, inf], [-inf, -inf, 1.0]):
        x = np.stack([np.array([0.0, 1.0, 2.0]), np.array(col), np.array([-1.0, 0.0, 1.0])], axis=1).astype(dt)
        y = np.zeros_like(x)
        for arrays in ((x, y), (torch.as_tensor(x, device="cuda:0"), torch.as_tensor(y, device="cuda:0"))):
            with pytest.raises(pkg.BuilderError.Monotonic) as e:
                pkg.Interp1D.builder(arrays[1]).lane_axes(arrays[0]).build()
            assert str(e.value).endswith("Values in the x axis need to be strictly monotonic rising (lane 1)"), (col, str(e.value))


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_signed_zero_and_infinite_ties(pkg, dt):
    """-0.0, +0.0 as neighbouring knots (either order) is a tie, and so is inf, inf: Monotonic from host arrays and from
    device arrays, naming the lane"""
    ties_case(pkg, dt)


def test_the_bounds_checked_library_runs_clean():
    """the child runs, under libndinterp_hip_dbg.so (selected by NDI_LIB: no sanitizer, nothing preloaded), one case per kernel
    and the flawed device axes, and the small cases of this file and of tests/test_gpu_lane_axes_plans.py: the hostile columns
    at n <= 6, the legal-but-odd columns and the validation verdicts, the oracle per column at every end kind, the padded
    stride, the refused strides and empty batches, async_launch with finish, and the eight threads.  The large cases (4097
    knots, the record copy's second trip and its cap, the two chunks) stay out of it."""
    from test_gpu_checked_build import _ensure_debug_library
    _ensure_debug_library()
    env = dict(os.environ, NDI_LIB="libndinterp_hip_dbg.so")
    select = ("test_one_case_per_kernel or test_device_axes_are_checked or (test_hostile_columns_against and not n33) or "
              "test_infinite_end_knots or test_host_and_device_validation or test_signed_zero or "
              "test_against_the_oracle_per_column_for_every_end_kind or test_padded_out_row_stride or test_strides_below_lanes or "
              "test_async_launch_and_finish or test_eight_threads")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_lane_axes_hostile.py"),
                        os.path.join(ROOT, "tests", "test_gpu_lane_axes_plans.py"), "-m", "gpu", "-x", "-q", "-k", select],
                       capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "failed" not in r.stdout.splitlines()[-1]
