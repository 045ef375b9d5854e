"""GPU: lane-wise evaluation (ndi_interp1d_eval_lanewise): a query per lane, out[j, l] = f_l(xs[j, l]).  Every row is compared
BIT FOR BIT, zero signs included (hostile_inputs.check_bits), and the yardstick is always code that exists without this
entry point: `interp_array` of the same handle (column l of the result against `interp_array(xs[:, l])[:, l]`), for inverse
handles outside the common range the numpy restatement tests/inverse_ref.py.  Every forward case runs under the four
combinations of NDI_LANEWISE_RECORDS (0 plain tables, 1 the element-record copy) and NDI_LANEWISE_MODE (2 fused, 1 the
two-kernel form); the library's plan line (NDI_TRACE_PLAN) says which one ran."""
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
from test_gpu_inverse import build, device_tables, host

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
VARIANTS = ((0, 2), (1, 2), (0, 1), (1, 1))      # (NDI_LANEWISE_RECORDS, NDI_LANEWISE_MODE)


def set_variant(monkeypatch, records, mode):
    monkeypatch.setenv("NDI_LANEWISE_RECORDS", str(records))
    monkeypatch.setenv("NDI_LANEWISE_MODE", str(mode))


def forward(pkg, source, x, y, extrapolate=False):
    """the interpolator of a forward source name"""
    B = pkg.Interp1D.builder
    if source == "linear":
        return B(y).x(x).strategy(pkg.Linear.new().extrapolate(extrapolate)).build()
    if source == "natural":
        return B(y).x(x).strategy(pkg.CubicSpline.new().boundary(pkg.BoundaryCondition.Natural).extrapolate(extrapolate)).build()
    if source == "notaknot":
        return B(y).x(x).strategy(pkg.CubicSpline.new().extrapolate(extrapolate)).build()
    if source == "akima":
        return B(y).x(x).strategy(pkg.Akima.new().extrapolate(extrapolate)).build()
    pc = B(y).x(x).strategy(pkg.Pchip.new().extrapolate(extrapolate)).build()
    if source == "pchip":
        return pc
    if source == "dpchip":
        return pc.derivative(1)
    if source == "anti_pchip":
        return pc.antiderivative()
    assert source == "anti_linear", source
    return B(y).x(x).strategy(pkg.Linear.new().extrapolate(extrapolate)).build().antiderivative()


def lane_queries(rng, x, Q, L):
    """(Q, L) abscissae inside the knots: per lane both end knots, every knot (as many as fit), the floats one ulp either
    side of interior knots, uniform values between -- permuted independently per lane, so that neighbouring lanes sit in
    different intervals"""
    T = x.dtype.type
    inner = x[1:-1]
    special = np.concatenate([[x[0], x[-1]], inner, np.nextafter(inner, T(np.inf)), np.nextafter(inner, T(-np.inf))]).astype(x.dtype)
    out = np.empty((Q, L), x.dtype)
    for l in range(L):
        s = special
        if len(special) > Q:          # the end knots first, then as many of the others as fit
            s = np.concatenate([special[:2], rng.choice(special[2:], Q - 2, replace=False)]) if Q > 2 else special[:Q]
        col = np.concatenate([s, rng.uniform(x[0], x[-1], Q - len(s)).astype(x.dtype)])
        out[:, l] = np.clip(rng.permutation(col) if Q > 1 else col, x[0], x[-1])
    return out


def per_lane(it, xs):
    """the yardstick: column l of the result is interp_array(xs[:, l])[:, l] -- L row-wise evaluations of the same handle"""
    Q, L = xs.shape
    ref = np.empty((Q, L), xs.dtype)
    for l in range(L):
        ref[:, l] = it.interp_array(np.ascontiguousarray(xs[:, l])).reshape(Q, L)[:, l]
    return ref


def data_for(source, rng, n, L, dt):
    y = rng.normal(size=(n, L))
    if source.startswith("anti_"):
        y = np.abs(y)
    return y.astype(dt)


def axis(kind, rng, n, dt):
    """even: the O(1) guess of the search; clustered: uneven steps, one in five twenty times shorter"""
    return np.arange(n).astype(dt) if kind == "even" else ic.knots(rng, n, dt)


def all_variants(pkg, monkeypatch, it, xs, ref, what, two_kernel_only=False):
    import torch
    for records, mode in (((0, 1),) if two_kernel_only else VARIANTS):
        set_variant(monkeypatch, records, mode)
        w = f"{what}, records = {records}, mode = {mode}"
        hostile_inputs.check_bits(it.interp_lanewise(xs), ref, w + ": host")
        got = it.interp_lanewise(torch.as_tensor(xs, device="cuda:0"))
        assert got.is_cuda and tuple(got.shape) == xs.shape
        hostile_inputs.check_bits(got.cpu().numpy(), ref, w + ": device")


# ---- broadcast identity ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("source", ["linear", "natural", "notaknot", "pchip", "akima", "dpchip", "anti_pchip", "anti_linear"])
def test_broadcast_identity(pkg, monkeypatch, dt, source):
    """the same abscissa in every lane of a row: interp_array's row"""
    rng = np.random.default_rng(1)
    n, L, Q = 33, 7, 301
    x = ic.knots(rng, n, dt)
    it = forward(pkg, source, x, data_for(source, rng, n, L, dt))
    xs = lane_queries(rng, x, Q, 1)[:, 0]
    ref = it.interp_array(xs)
    wide = np.broadcast_to(xs[:, None], (Q, L)).copy()
    all_variants(pkg, monkeypatch, it, wide, ref, f"{source} broadcast {np.dtype(dt).name}", source.startswith("anti_"))


# ---- own query per lane -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("kind", ["even", "clustered"])
@pytest.mark.parametrize("source", ["linear", "pchip", "anti_pchip"])
def test_own_query_per_lane(pkg, monkeypatch, dt, kind, source):
    """the eight shapes of inverse_cases: 3 lanes (a wavefront spans 21 1/3 rows), 65 (a row straddles wavefronts), one
    lane, Q of 1, 63, 65 and 4097"""
    for n, L, Q in ic.SHAPES:
        rng = np.random.default_rng([n, L, Q, np.dtype(dt).itemsize])
        x = axis(kind, rng, n, dt)
        it = forward(pkg, source, x, data_for(source, rng, n, L, dt))
        xs = lane_queries(rng, x, Q, L)
        all_variants(pkg, monkeypatch, it, xs, per_lane(it, xs), f"{source} {kind} {n} x {L}, Q = {Q}, {np.dtype(dt).name}",
                     source.startswith("anti_"))


def test_an_axis_beyond_the_lds_budget(pkg, monkeypatch, capfd):
    """40001 f64 knots (320 KB) do not fit LDS: the fused kernel searches in global memory (stage=0) -- the pyramid for the
    batch of 257 rows (lut=0), the axis' bucket index from 4096 elements on (1400 rows: lut=2), as the row-wise search does"""
    rng = np.random.default_rng(2)
    n, L = 40001, 3
    x = ic.knots(rng, n, np.float64)
    for source in ("linear", "pchip"):
        it = forward(pkg, source, x, data_for(source, rng, n, L, np.float64))
        for Q, lut in ((257, "lut=0"), (1400, "lut=2")):
            xs = lane_queries(rng, x, Q, L)
            ref = per_lane(it, xs)
            monkeypatch.setenv("NDI_TRACE_PLAN", "1")
            capfd.readouterr()
            all_variants(pkg, monkeypatch, it, xs, ref, f"{source} 40001 x 3, Q = {Q}")
            plans = [ln for ln in capfd.readouterr().err.splitlines() if "lanewise form=fused" in ln]
            monkeypatch.delenv("NDI_TRACE_PLAN")
            assert plans and all("stage=0" in ln and lut in ln for ln in plans), plans
            assert any("records=1" in ln for ln in plans) and any("records=0" in ln for ln in plans), plans


def test_the_staged_bucket_index(pkg, monkeypatch, capfd):
    """257 clustered knots and 4097 x 64 elements: the bucket index is staged in LDS behind the pyramid (stage=1 lut=1); the
    evenly spaced axis, whose O(1) guess is exact, and a batch below 4096 elements keep the pyramid search (lut=0)"""
    for kind, (n, L, Q), lut in (("clustered", (257, 64, 4097), "lut=1"), ("even", (257, 64, 4097), "lut=0"), ("clustered", (257, 4, 65), "lut=0")):
        rng = np.random.default_rng([n, L, Q])
        x = axis(kind, rng, n, np.float32)
        it = forward(pkg, "pchip", x, data_for("pchip", rng, n, L, np.float32))
        xs = lane_queries(rng, x, Q, L)
        ref = per_lane(it, xs)
        monkeypatch.setenv("NDI_TRACE_PLAN", "1")
        capfd.readouterr()
        all_variants(pkg, monkeypatch, it, xs, ref, f"pchip {kind} {n} x {L}, Q = {Q}")
        plans = [ln for ln in capfd.readouterr().err.splitlines() if "lanewise form=fused" in ln]
        monkeypatch.delenv("NDI_TRACE_PLAN")
        assert plans and all("stage=1" in ln and lut in ln for ln in plans), (kind, plans)


@pytest.mark.parametrize("dt", DTYPES)
def test_the_stride_loop_runs_more_than_once(pkg, monkeypatch, capfd, dt):
    """one workgroup per CU (NDI_LANEWISE_WGS=1): 4097 x 64 elements are more than one pass of the launched grid in every form"""
    rng = np.random.default_rng(3)
    n, L, Q = 257, 64, 4097
    x = ic.knots(rng, n, dt)
    monkeypatch.setenv("NDI_LANEWISE_WGS", "1")
    for source in ("pchip", "anti_linear"):
        it = forward(pkg, source, x, data_for(source, rng, n, L, dt))
        xs = lane_queries(rng, x, Q, L)
        ref = per_lane(it, xs)
        monkeypatch.setenv("NDI_TRACE_PLAN", "1")
        capfd.readouterr()
        all_variants(pkg, monkeypatch, it, xs, ref, f"{source} one workgroup per CU", source.startswith("anti_"))
        plans = [ln for ln in capfd.readouterr().err.splitlines() if "[ndi plan] lanewise form=" in ln]
        monkeypatch.delenv("NDI_TRACE_PLAN")
        assert plans
        for ln in plans:
            grid = int(ln.rsplit("grid=", 1)[1].split()[0])
            assert grid * 256 * 2 <= Q * L, ln              # at least two full trips of every thread
    inv = forward(pkg, "pchip", x, np.cumsum(np.abs(data_for("pchip", rng, n, L, dt)) + dt(0.01), axis=0).astype(dt)).inverse()
    N = inv.strategy.data_table()
    vs = rng.uniform(N[0].max(), N[-1].min(), (Q, 1)).astype(dt) + np.zeros((1, L), dt)
    hostile_inputs.check_bits(inv.interp_lanewise(vs), inv.interp_array(np.ascontiguousarray(vs[:, 0])), "inverse, one workgroup per CU")


# ---- extrapolation modes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("source", ["linear", "pchip", "natural", "anti_pchip"])
def test_end_interval_extrapolation_and_nan(pkg, monkeypatch, dt, source):
    rng = np.random.default_rng(4)
    n, L, Q = 17, 5, 129
    x = ic.knots(rng, n, dt)
    y = data_for(source, rng, n, L, dt)
    it = forward(pkg, source, x, y, extrapolate=True)
    xs = lane_queries(rng, x, Q, L)
    w = x[-1] - x[0]
    xs[::7] = (x[0] - rng.uniform(0, 2, xs[::7].shape) * w).astype(dt)      # below and above the knots, other lanes in other rows
    xs[3::11] = (x[-1] + rng.uniform(0, 2, xs[3::11].shape) * w).astype(dt)
    xs[5, 1] = np.inf
    xs[6, 2] = -np.inf
    all_variants(pkg, monkeypatch, it, xs, per_lane(it, xs), f"{source} extrapolated {np.dtype(dt).name}", source.startswith("anti_"))
    # a NaN query: the search cannot place it, with extrapolation (NAN_QUERY) and without (out of range)
    bad = xs.copy()
    bad[40, 3] = np.nan
    for records, mode in (((0, 1),) if source.startswith("anti_") else VARIANTS):
        set_variant(monkeypatch, records, mode)
        with pytest.raises(pkg.Panic, match="NaN") as e:
            it.interp_lanewise(bad)
        assert e.value.index == 40 * L + 3
        strict = forward(pkg, source, x, y)
        inside = np.clip(bad, x[0], x[-1])
        with pytest.raises(pkg.InterpolateError.OutOfBounds, match="^x = NaN is not in range$") as e:
            strict.interp_lanewise(inside)
        assert e.value.index == 40 * L + 3 and np.isnan(e.value.value)


@pytest.mark.parametrize("dt", DTYPES)
def test_periodic_wrap(pkg, monkeypatch, dt):
    """queries far outside the knots wrap into them; +-inf wraps to NaN, which the search refuses (NDI_NAN_QUERY)"""
    rng = np.random.default_rng(5)
    n, L, Q = 19, 4, 200
    x = ic.knots(rng, n, dt)
    y = rng.normal(size=(n, L)).astype(dt)
    y[-1] = y[0]
    it = pkg.Interp1D.builder(y).x(x).strategy(
        pkg.CubicSpline.new().boundary(pkg.BoundaryCondition.Periodic).extrapolate(True)).build()
    w = x[-1] - x[0]
    xs = (x[0] + rng.uniform(-5, 6, (Q, L)) * w).astype(dt)
    xs[:n, 0] = x
    ref = per_lane(it, xs)
    all_variants(pkg, monkeypatch, it, xs, ref, f"periodic {np.dtype(dt).name}")
    for v, (j, l) in ((np.inf, (17, 2)), (-np.inf, (120, 0)), (np.nan, (3, 3))):
        bad = xs.copy()
        bad[j, l] = v
        bad[150, 1] = np.nan        # a later failure: the lowest element index is reported
        for records, mode in VARIANTS:
            set_variant(monkeypatch, records, mode)
            with pytest.raises(pkg.Panic, match="NaN") as e:
                it.interp_lanewise(bad)
            assert e.value.index == j * L + l
            buf = np.full((Q, L), 7.0, dt)
            with pytest.raises(pkg.Panic, match="NaN"):
                it.interp_lanewise_into(bad, buf)
            hostile_inputs.check_bits(buf[:j], ref[:j], "periodic: rows before the failing row")
            assert np.all(buf[j:] == 7.0)


# ---- the first-error rule ---------------------------------------------------------------------------------------------------
def raw_call(pkg, it, q, nq, q_stride, out, out_stride, *, q_dev, out_dev, flags=0, path=0, async_launch=0):
    cap = pkg._capi
    opts = cap.EvalOpts()
    opts.q_memspace = cap.MEM_DEVICE if q_dev else cap.MEM_HOST
    opts.out_memspace = cap.MEM_DEVICE if out_dev else cap.MEM_HOST
    opts.flags = flags
    opts.path = path
    opts.async_launch = async_launch
    info = cap.OobInfo()
    qp = (q.data_ptr() if q_dev else q.ctypes.data) if q is not None else None
    op = (out.data_ptr() if out_dev else out.ctypes.data) if out is not None else None
    st = cap.lib().ndi_interp1d_eval_lanewise(it.strategy._h, qp, nq, q_stride, op, out_stride, C.byref(opts), C.byref(info))
    return st, info


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("source", ["linear", "pchip", "anti_linear"])
def test_first_error_rule(pkg, monkeypatch, dt, source):
    """two failing elements (j1, l1), (j2, l2) with j1 < j2 and l1 > l2: the report names j1 * lanes + l1 and that element's
    value; rows before j1 are written, row j1 and all later rows keep the sentinel; padding of strided rows is untouched"""
    import torch
    cap = pkg._capi
    rng = np.random.default_rng(6)
    n, L, Q = 17, 5, 300
    x = ic.knots(rng, n, dt)
    it = forward(pkg, source, x, data_for(source, rng, n, L, dt))
    xs = lane_queries(rng, x, Q, L)
    ref = per_lane(it, xs)
    tdt = torch.float64 if dt == np.float64 else torch.float32
    j1, l1, j2, l2 = 131, 4, 140, 1
    above = np.nextafter(x[-1], dt(np.inf))
    for bad1, bad2 in ((above, dt(np.nan)), (dt(np.nan), above), (np.nextafter(x[0], dt(-np.inf)), dt(-np.inf))):
        qq = xs.copy()
        qq[j1, l1] = bad1
        qq[j2, l2] = bad2
        for records, mode in (((0, 1),) if source.startswith("anti_") else VARIANTS):
            set_variant(monkeypatch, records, mode)
            for q_dev in (False, True):
                for out_dev in (False, True):
                    for qs, os_ in ((L, L), (L + 3, L + 2)):
                        for flags in (0, cap.EVAL_FRESH_OUTPUT, cap.EVAL_ROWS_AFTER_ERROR_UNSPECIFIED):
                            what = (f"{source} bad = {bad1} at ({j1}, {l1}), records = {records}, mode = {mode}, q_dev = {q_dev}, "
                                    f"out_dev = {out_dev}, strides = ({qs}, {os_}), flags = {flags}")
                            qh = np.full((Q, qs), np.nan, dt)          # the padding would fail if it were read
                            qh[:, :L] = qq
                            qa = torch.as_tensor(qh, device="cuda:0") if q_dev else qh
                            out = torch.full((Q, os_), 7.0, dtype=tdt, device="cuda:0") if out_dev else np.full((Q, os_), 7.0, dtype=dt)
                            st, info = raw_call(pkg, it, qa, Q, qs, out, os_, q_dev=q_dev, out_dev=out_dev, flags=flags)
                            assert st == cap.OUT_OF_BOUNDS and info.status == st and info.axis == 0, what    # no extrapolation: NaN too
                            assert info.index == j1 * L + l1, (what, info.index)
                            msg = cap.last_error()
                            assert msg.startswith("x = ") and msg.endswith("is not in range"), (what, msg)
                            assert (np.isnan(info.value) if np.isnan(bad1) else info.value == float(bad1)), what
                            o = host(out)
                            assert np.all(o[:, L:] == 7.0), what
                            if flags and out_dev:
                                continue              # the rows at and after the failing row are the caller's to drop
                            hostile_inputs.check_bits(np.ascontiguousarray(o[:j1, :L]), ref[:j1], what + ": rows before the failing row")
                            assert np.all(o[j1:] == 7.0), what
        # the mirror: the same report as an exception, with the buffer's rows as the raw call leaves them
        buf = np.full((Q, L), 7.0, dt)
        with pytest.raises(pkg.InterpolateError.OutOfBounds, match="^x = .* is not in range$") as e:
            it.interp_lanewise_into(qq, buf)
        assert e.value.index == j1 * L + l1
        hostile_inputs.check_bits(buf[:j1], ref[:j1], "mirror: rows before the failing row")
        assert np.all(buf[j1:] == 7.0)
        with pytest.raises(pkg.InterpolateError.OutOfBounds) as e:
            it.interp_lanewise_into(torch.as_tensor(qq, device="cuda:0"), torch.full((Q, L), 7.0, dtype=tdt, device="cuda:0"), fresh=True)
        assert e.value.index == j1 * L + l1
    # the good batch through strided rows
    qh = np.full((Q, L + 3), np.nan, dt)
    qh[:, :L] = xs
    for q_dev in (False, True):
        for out_dev in (False, True):
            qa = torch.as_tensor(qh, device="cuda:0") if q_dev else qh
            out = torch.full((Q, L + 2), 7.0, dtype=tdt, device="cuda:0") if out_dev else np.full((Q, L + 2), 7.0, dtype=dt)
            st, info = raw_call(pkg, it, qa, Q, L + 3, out, L + 2, q_dev=q_dev, out_dev=out_dev)
            assert st == cap.OK, cap.last_error()
            o = host(out)
            hostile_inputs.check_bits(np.ascontiguousarray(o[:, :L]), ref, f"strided rows, q_dev = {q_dev}, out_dev = {out_dev}")
            assert np.all(o[:, L:] == 7.0)


# ---- inverse handles --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("source", ["linear", "pchip", "anti_pchip", "anti_linear"])
def test_inverse_values_per_lane_inside_the_common_range(pkg, dt, source):
    import torch
    for n, L, Q in ((257, 65, 63), (5, 4, 65), (3, 3, 63)):
        x, y, _ = ic.case(source, dt, n, L, Q)
        src, base = build(pkg, source, x, y)
        inv = src.inverse()
        N = inv.strategy.data_table()
        rng = np.random.default_rng([n, L, Q])
        vs = np.stack([ic.queries(rng, N, Q) for _ in range(L)], axis=1)
        ref = np.empty((Q, L), dt)
        for l in range(L):
            ref[:, l] = inv.interp_array(np.ascontiguousarray(vs[:, l])).reshape(Q, L)[:, l]
        what = f"inverse of {source} {n} x {L} {np.dtype(dt).name}"
        hostile_inputs.check_bits(inv.interp_lanewise(vs), ref, what + ": host")
        hostile_inputs.check_bits(inv.interp_lanewise(torch.as_tensor(vs, device="cuda:0")).cpu().numpy(), ref, what + ": device")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("source", ["linear", "pchip", "anti_pchip"])
def test_inverse_uses_the_lanes_own_range(pkg, dt, source):
    """lanes with different value ranges, rising and falling in one handle: values inside lane l's range but outside the
    range common to all lanes, against the restatement applied to that lane's column alone; a value outside its lane's
    range fails with that element's index"""
    import torch
    cap = pkg._capi
    rng = np.random.default_rng(7)
    n, L, Q = 33, 6, 97
    x = ic.knots(rng, n, dt)
    if source == "anti_pchip":
        y = (np.abs(rng.normal(size=(n, L))) * np.arange(1, L + 1)).astype(dt)          # every P rises from +0, to other totals
    else:
        inc = np.abs(rng.normal(size=(n - 1, L))) + 0.01
        c = np.concatenate([np.zeros((1, L)), np.cumsum(inc, axis=0)])
        y = ((c / c[-1]) * np.arange(1, L + 1) * np.where(np.arange(L) % 2 == 1, -1.0, 1.0)).astype(dt)   # lane l spans [0, +-(l + 1)]
    src, base = build(pkg, source, x, y)
    cls, N, ys, a, b = device_tables(source, src, base)
    inv = src.inverse()
    lo, hi = np.minimum(N[0], N[-1]), np.maximum(N[0], N[-1])
    clo, chi = ir.common_range(N)
    vs = np.empty((Q, L), dt)
    for l in range(L):
        col = np.concatenate([[lo[l], hi[l]], rng.uniform(lo[l], hi[l], Q - 2)]).astype(dt)
        vs[:, l] = np.clip(rng.permutation(col), lo[l], hi[l])
    assert np.any((vs < clo) | (vs > chi))
    ref = np.empty((Q, L), dt)
    for l in range(L):
        col = lambda t: None if t is None else np.ascontiguousarray(t[:, l:l + 1])      # noqa: E731
        ref[:, l] = ir.solve(cls, x, col(N), np.ascontiguousarray(vs[:, l]), col(ys), col(a), col(b))[0][:, 0]
    what = f"inverse of {source}, own ranges, {np.dtype(dt).name}"
    hostile_inputs.check_bits(inv.interp_lanewise(vs), ref, what + ": host")
    hostile_inputs.check_bits(inv.interp_lanewise(torch.as_tensor(vs, device="cuda:0")).cpu().numpy(), ref, what + ": device")
    # a row-wise call refuses the same values: they are outside the common range
    with pytest.raises(pkg.InterpolateError.OutOfBounds):
        inv.interp_array(np.ascontiguousarray(vs[:, L - 1]))
    # outside the lane's own range
    j1, l1, j2, l2 = 40, 4, 41, 0
    for bad1, status in ((np.nextafter(hi[l1], dt(np.inf)), cap.OUT_OF_BOUNDS), (np.nextafter(lo[l1], dt(-np.inf)), cap.OUT_OF_BOUNDS),
                         (dt(np.nan), cap.NAN_QUERY)):
        qq = vs.copy()
        qq[j1, l1] = bad1
        qq[j2, l2] = np.inf
        for q_dev in (False, True):
            for out_dev in (False, True):
                for flags in (0, cap.EVAL_FRESH_OUTPUT):
                    tdt = torch.float64 if dt == np.float64 else torch.float32
                    qa = torch.as_tensor(qq, device="cuda:0") if q_dev else qq
                    out = torch.full((Q, L), 7.0, dtype=tdt, device="cuda:0") if out_dev else np.full((Q, L), 7.0, dtype=dt)
                    st, info = raw_call(pkg, inv, qa, Q, L, out, L, q_dev=q_dev, out_dev=out_dev, flags=flags)
                    w = f"{what}: bad = {bad1}, q_dev = {q_dev}, out_dev = {out_dev}, flags = {flags}"
                    assert st == status and info.index == j1 * L + l1 and info.axis == 0, (w, st, info.index)
                    msg = cap.last_error()
                    if status == cap.NAN_QUERY:
                        assert np.isnan(info.value) and "NaN" in msg, (w, msg)
                    else:
                        assert info.value == float(bad1) and msg.startswith("v = ") and msg.endswith("is not in range"), (w, msg)
                    if flags and out_dev:
                        continue
                    o = host(out)
                    hostile_inputs.check_bits(o[:j1], ref[:j1], w + ": rows before the failing row")
                    assert np.all(o[j1:] == 7.0), w
        if status == cap.OUT_OF_BOUNDS:
            with pytest.raises(pkg.InterpolateError.OutOfBounds, match="^v = .* is not in range$") as e:
                inv.interp_lanewise(qq)
            assert e.value.index == j1 * L + l1 and e.value.value == float(bad1)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("source", ic.SOURCES)
def test_round_trip_in_one_call(pkg, dt, source):
    """the round trip of tests/test_gpu_inverse.py as ONE lane-wise call: bit for bit the diagonal that its round_trip takes
    from the (Q, L, L) evaluation"""
    for n, L, Q in ic.TRIP_SHAPES:
        if n < ic.MIN_N.get(source, 2):
            continue
        x, y, q = ic.case(source, dt, n, L, Q)
        src, _ = build(pkg, source, x, y)
        X = src.inverse().interp_array(q).reshape(Q, L)
        F = src.interp_array(np.ascontiguousarray(X.reshape(-1))).reshape(Q, L, L)
        hostile_inputs.check_bits(src.interp_lanewise(X), F[:, np.arange(L), np.arange(L)],
                                  f"{source} {n} x {L} {np.dtype(dt).name}: the round trip's diagonal")


# ---- hostile data -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("source", ["linear", "pchip"])
def test_hostile_data(pkg, monkeypatch, dt, source):
    """infinities, NaN data and subnormals in the tables (the recipes of tests/hostile_inputs.py): whatever a row-wise
    evaluation makes of them, the lane-wise one makes the same"""
    rng = np.random.default_rng(8)
    n, L = 9, 8
    for kind in ("even", "uneven"):
        for classes in (("scale",), ("nonfinite",)):
            for part in range(min(2, hostile_inputs.parts("pchip", n, L, classes))):
                x, y, _ = hostile_inputs.generate("pchip", dt, n, L, classes, kind, part)
                with np.errstate(all="ignore"):
                    it = forward(pkg, source, x, y)
                    xs = lane_queries(rng, x, 70, L)
                    all_variants(pkg, monkeypatch, it, xs, per_lane(it, xs), f"hostile {source} {kind} {classes[0]} part {part} {np.dtype(dt).name}")


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals(pkg):
    import torch
    cap = pkg._capi
    x = np.arange(8.0)
    y = np.stack([x * x, -x, x + 1.0], axis=1)
    L = 3
    xi = torch.arange(6, dtype=torch.int32, device="cuda:0")
    with pytest.raises(ValueError, match="eval_lanewise: an integer handle is a Linear interpolator"):
        pkg.Interp1D.builder(xi * 3).x(xi).build().interp_lanewise(xi)
    xh = torch.arange(6, dtype=torch.float16, device="cuda:0")
    with pytest.raises(ValueError, match="eval_lanewise: an f16 / bf16 handle is a Linear interpolator"):
        pkg.Interp1D.builder(xh * 0.5).x(xh).build().interp_lanewise(xh)
    pc = pkg.Interp1D.builder(y).x(x).strategy(pkg.Pchip.new()).build()
    handles = (("Pchip", pc), ("the antiderivative of Pchip", pkg.Interp1D.builder(np.abs(y)).x(x).strategy(pkg.Pchip.new()).build().antiderivative()),
               ("the inverse of Linear", pkg.Interp1D.builder(y).x(x).build().inverse()))
    q = np.full((4, L), 1.5)
    for name, it in handles:
        out = np.full((4, L), 7.0)
        st, _ = raw_call(pkg, it, q, 4, L, out, L, q_dev=False, out_dev=False, path=cap.PATH_BUCKETED)
        assert st == cap.BAD_ARG and cap.last_error().startswith(f"eval_lanewise of {name}: NDI_PATH_BUCKETED"), cap.last_error()
        st, _ = raw_call(pkg, it, q, 4, L, out, L, q_dev=False, out_dev=False, async_launch=1)
        assert st == cap.UNSUPPORTED and "async_launch is not provided" in cap.last_error()
        st, _ = raw_call(pkg, it, q, 4, L - 1, out, L, q_dev=False, out_dev=False)
        assert st == cap.BAD_ARG and cap.last_error() == "q_row_stride (2) < lanes (3)"
        st, _ = raw_call(pkg, it, q, 4, L, out, L - 1, q_dev=False, out_dev=False)
        assert st == cap.BAD_ARG and cap.last_error() == "out_row_stride (2) < lanes (3)"
        st, _ = raw_call(pkg, it, None, 4, L, out, L, q_dev=False, out_dev=False)
        assert st == cap.BAD_ARG and cap.last_error() == "null query / output pointer"
        st, _ = raw_call(pkg, it, q, 4, L, None, L, q_dev=False, out_dev=False)
        assert st == cap.BAD_ARG and cap.last_error() == "null query / output pointer"
        st, _ = raw_call(pkg, it, q, 4, L, out, L, q_dev=False, out_dev=False, flags=64)
        assert st == cap.BAD_ARG and "unknown bits" in cap.last_error()
        assert np.all(out == 7.0)
        st, info = raw_call(pkg, it, None, 0, L, None, L, q_dev=False, out_dev=False)      # nq == 0: nothing is touched
        assert st == cap.OK and info.status == cap.OK
        st, _ = raw_call(pkg, it, q, 0, L, out, L, q_dev=False, out_dev=False)
        assert st == cap.OK and np.all(out == 7.0)
    # the mirror's shapes
    with pytest.raises(pkg.Panic, match=r"ShapeError/IncompatibleShape: incompatible shapes expected: \[.., 3\], got: \[4, 2\]"):
        pc.interp_lanewise(np.zeros((4, 2)))
    with pytest.raises(pkg.Panic, match=r"ShapeError/IncompatibleShape: incompatible shapes expected: \[.., 3\], got: \[\]"):
        pc.interp_lanewise(np.zeros(()))
    with pytest.raises(pkg.Panic, match=r"ShapeError/IncompatibleShape: incompatible shapes expected: \[2, 4, 3\], got: \[8, 3\]"):
        pc.interp_lanewise_into(np.full((2, 4, 3), 1.5), np.zeros((8, 3)))
    with pytest.raises(TypeError, match="buffer has element type float32"):
        pc.interp_lanewise_into(np.full((4, 3), 1.5), np.zeros((4, 3), np.float32))
    # any leading rank; scalar data takes queries of any shape
    got = pc.interp_lanewise(np.full((2, 4, 3), 1.5))
    assert got.shape == (2, 4, 3)
    hostile_inputs.check_bits(got.reshape(8, 3), np.broadcast_to(pc.interp_array(np.array([1.5])), (8, 3)).copy(), "rank-3 queries")
    sc = pkg.Interp1D.builder(x * x).x(x).strategy(pkg.Pchip.new()).build()
    qs = np.linspace(0.0, 7.0, 12).reshape(3, 4)
    hostile_inputs.check_bits(sc.interp_lanewise(qs), sc.interp_array(qs), "scalar data")


# ---- lifetimes --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", ["linear", "pchip"])
def test_trim_rebuilds_the_record_copy_and_a_clone_builds_its_own(pkg, monkeypatch, capfd, source):
    rng = np.random.default_rng(9)
    n, L, Q = 65, 9, 257
    x = ic.knots(rng, n, np.float64)
    it = forward(pkg, source, x, data_for(source, rng, n, L, np.float64))
    xs = lane_queries(rng, x, Q, L)
    ref = per_lane(it, xs)
    set_variant(monkeypatch, 1, 2)
    monkeypatch.setenv("NDI_TRACE_PLAN", "1")
    capfd.readouterr()

    def built():
        return sum("lanewise records built" in ln for ln in capfd.readouterr().err.splitlines())
    hostile_inputs.check_bits(it.interp_lanewise(xs), ref, "first call")
    assert built() == 1
    hostile_inputs.check_bits(it.interp_lanewise(xs), ref, "second call")
    assert built() == 0                       # kept
    it.strategy.trim()
    hostile_inputs.check_bits(it.interp_lanewise(xs), ref, "after trim")
    assert built() == 1                       # released by trim, rebuilt
    rep = pkg.Interp1D(it.x, it.data, it.strategy.clone(0))
    hostile_inputs.check_bits(rep.interp_lanewise(xs), ref, "clone")
    assert built() == 1                       # the clone's own
    it.strategy.release()
    hostile_inputs.check_bits(rep.interp_lanewise(xs), ref, "clone, after the source is destroyed")
    for kind in ("anti", "inverse"):
        mono = np.cumsum(np.abs(data_for(source, rng, n, L, np.float64)) + 0.01, axis=0)
        h = forward(pkg, source, x, mono)
        h = h.antiderivative() if kind == "anti" else h.inverse()
        q = xs if kind == "anti" else rng.uniform(mono[0].max(), mono[-1].min(), (Q, L))
        want = h.interp_lanewise(q)
        h.strategy.trim()
        hostile_inputs.check_bits(h.interp_lanewise(q), want, kind + ": after trim")
        hostile_inputs.check_bits(pkg.Interp1D(h.x, h.data, h.strategy.clone(0)).interp_lanewise(q), want, kind + ": clone")


# ---- the bounds-checked library ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", ["linear", "pchip", "anti_pchip", "anti_linear"])
def test_one_case_per_kernel_class(pkg, monkeypatch, source):
    """one case per kernel class (fused with records and plain tables, LDS and global pyramid; the two-kernel form of all four
    kinds; the inverse kernel of every class; the pre-pass): what runs again under the bounds-checked library (below)"""
    import torch
    for dt, (n, L, Q) in ((np.float64, (257, 65, 63)), (np.float32, (5, 4, 65))):
        rng = np.random.default_rng([n, L])
        x = ic.knots(rng, n, dt)
        it = forward(pkg, source, x, data_for(source, rng, n, L, dt))
        xs = lane_queries(rng, x, Q, L)
        ref = per_lane(it, xs)
        all_variants(pkg, monkeypatch, it, xs, ref, f"{source} {n} x {L}", source.startswith("anti_"))
        buf = torch.full((Q, L), 7.0, dtype=torch.float64 if dt == np.float64 else torch.float32, device="cuda:0")
        it.interp_lanewise_into(torch.as_tensor(xs, device="cuda:0"), buf)             # a caller's buffer: the pre-pass runs
        hostile_inputs.check_bits(buf.cpu().numpy(), ref, f"{source}: with the pre-pass")
        xi, yi, q = ic.case(source, dt, n, L, Q)
        inv = build(pkg, source, xi, yi)[0].inverse()
        vs = np.broadcast_to(q[:, None], (Q, L)).copy()
        hostile_inputs.check_bits(inv.interp_lanewise(vs), inv.interp_array(q), f"inverse of {source}")
        inv.interp_lanewise_into(torch.as_tensor(vs, device="cuda:0"), buf)
        hostile_inputs.check_bits(buf.cpu().numpy(), inv.interp_array(q), f"inverse of {source}: with the pre-pass")
    if source == "pchip":       # the pyramid from global memory
        x = ic.knots(np.random.default_rng(1), 40001, np.float64)
        it = forward(pkg, source, x, data_for(source, np.random.default_rng(2), 40001, 3, np.float64))
        for Q in (65, 1400):        # the pyramid and, from 4096 elements on, the bucket index
            xs = lane_queries(np.random.default_rng(3), x, Q, 3)
            all_variants(pkg, monkeypatch, it, xs, per_lane(it, xs), f"40001 x 3, Q = {Q}")


def test_the_bounds_checked_library_runs_clean():
    from test_gpu_checked_build import _ensure_debug_library
    _ensure_debug_library()
    env = dict(os.environ, NDI_LIB="libndinterp_hip_dbg.so")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_lanewise.py"), "-m", "gpu", "-x", "-q",
                        "-k", "test_one_case_per_kernel_class"],
                       capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "failed" not in r.stdout.splitlines()[-1]
