"""GPU: Interp3D / Trilinear (include/ndinterp3d.h) against tests/trilinear_ref.py, bit for bit (integer views, NaN equal to
NaN): parity over dtypes, grids, trailing shapes, axes and memory spaces; the slab property against the project's own
Bilinear; every kernel instance by its plan line; errors and buffer state; hostile data; clone, scalar calls, streams,
threads; the bounds-checked library."""
import ctypes as C
import os
import re
import subprocess
import sys
import threading

import numpy as np
import pytest

import trilinear_ref as tr
from conftest import ROOT

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
GRIDS = [(2, 2, 2), (3, 2, 4), (5, 4, 3), (33, 17, 9)]
TRAILING = [(), (3,), (4,), (2, 3), (260,)]
SENTINEL = -77.25
PLAN = re.compile(r"\[ndi plan\] trilinear vec=(\d+) stage=(\d+) check=(\d+) grid=(\d+)")
WIDE = {np.float32: 4, np.float64: 2}
BLOCK = 256


class traced:
    """the trilinear plan lines (as dicts) of the calls inside"""

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
        self.plans = [dict(zip(("vec", "stage", "check", "grid"), map(int, m.groups()))) for m in PLAN.finditer(err)]


def expect(plans, what, n=1, **fields):
    assert len(plans) == n, (what, plans)
    for p in plans:
        for k, v in fields.items():
            assert p[k] == v, f"{what}: plan field {k} = {p[k]}, expected {v} in {p}"


def same_bits(got, ref, what):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.dtype == ref.dtype, (what, got.dtype, ref.dtype)
    a, b = tr.bits(got.reshape(ref.shape)), tr.bits(ref)
    if not np.array_equal(a, b):
        bad = np.argwhere(a != b)
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {bad.shape[0]} of {a.size} elements differ; first at {i}: got {got.reshape(ref.shape)[i]!r}, "
                             f"reference {ref[i]!r}")


def nonuniform(rng, n, dt, lo=0.0):
    return (lo + np.cumsum(rng.uniform(0.5, 1.5, n))).astype(dt)


def make(pkg, x, y, z, data, extrapolate=False):
    b = pkg.Interp3D.builder(data)
    if x is not None:
        b = b.x(x)
    if y is not None:
        b = b.y(y)
    if z is not None:
        b = b.z(z)
    return b.strategy(pkg.Trilinear.new().extrapolate(extrapolate)).build()


def inside(rng, k, q, dt):
    return np.clip(rng.uniform(k[0], k[-1], q).astype(dt), k[0], k[-1])


def dev(a):
    import torch
    return torch.as_tensor(a, device="cuda:0")


def raw_call(pkg, it, qx, qy, qz, nq, out, out_stride, *, q_dev=False, out_dev=False, flags=0, stream=None):
    cap = pkg._capi
    opts = cap.EvalOpts()
    opts.q_memspace = cap.MEM_DEVICE if q_dev else cap.MEM_HOST
    opts.out_memspace = cap.MEM_DEVICE if out_dev else cap.MEM_HOST
    opts.flags = flags
    opts.stream = stream
    info = cap.OobInfo()

    def ptr(a, on_dev):
        return None if a is None else (a.data_ptr() if on_dev else a.ctypes.data)
    st = cap.lib().ndi_interp3d_eval(it.strategy._h, ptr(qx, q_dev), ptr(qy, q_dev), ptr(qz, q_dev), nq, ptr(out, out_dev), out_stride,
                                     C.byref(opts), C.byref(info))
    return st, info


# ---- parity ----------------------------------------------------------------------------------------------------------------
def axes_of(kind, rng, shape, dt):
    if kind == "default":
        return [None] * 3, [np.arange(n).astype(dt) for n in shape]
    if kind == "uniform":
        ax = [np.linspace(-1.0, 2.0, n).astype(dt) for n in shape]
    else:
        ax = [nonuniform(rng, n, dt, lo) for n, lo in zip(shape, (-3.0, 0.0, 10.0))]
    return ax, ax


def query_sets(rng, ax, dt, extrapolate, small):
    km = [tr.knots_and_midpoints(k) for k in ax]
    if small:      # the full product: every knot and midpoint of every axis against every other
        sets = {"knots x midpoints": [np.ascontiguousarray(a.ravel()) for a in np.meshgrid(*km, indexing="ij")]}
    else:          # every knot and midpoint of each axis once, the shorter lists cycled
        m = max(len(k) for k in km)
        sets = {"knots and midpoints": [np.resize(k, m) for k in km]}
    sets["1 query"] = [inside(rng, k, 1, dt) for k in ax]
    sets["257 queries"] = [inside(rng, k, 257, dt) for k in ax]
    if extrapolate:
        span = [k[-1] - k[0] for k in ax]
        sets["far outside"] = [np.array([k[0] - 1e3 * s, k[-1] + 1e3 * s, k[0] - s / 3, k[-1] + s / 7, k[0]], dtype=dt)
                               for k, s in zip(ax, span)]
    return sets


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", GRIDS)
@pytest.mark.parametrize("trailing", TRAILING)
def test_parity(pkg, dt, shape, trailing):
    rng = np.random.default_rng(3)
    data = rng.uniform(-1, 1, shape + trailing).astype(dt)
    for kind in ("uniform", "default", "nonuniform"):
        given, ax = axes_of(kind, rng, shape, dt)
        for extrapolate in (False, True):
            it = make(pkg, *given, data, extrapolate)
            on_dev = make(pkg, *[None if k is None else dev(k) for k in given], dev(data), extrapolate)   # a builder on tensors
            for name, q in query_sets(rng, ax, dt, extrapolate, small=shape[0] <= 5).items():
                what = f"{np.dtype(dt)} {shape} {trailing} {kind} extrapolate={extrapolate} {name}"
                fail, _, ref = tr.trilinear_ref(*ax, data, *q, extrapolate)
                assert fail is None, what
                ref = ref.reshape(q[0].shape + trailing)
                got = it.interp_array(*q)
                assert isinstance(got, np.ndarray) and got.shape == ref.shape, what
                same_bits(got, ref, what + ": host arrays")
                for h in (it, on_dev):
                    got = h.interp_array(*[dev(a) for a in q])
                    assert got.is_cuda and tuple(got.shape) == ref.shape, what
                    same_bits(got.cpu().numpy(), ref, what + ": device tensors")


def test_queries_of_any_rank(pkg):
    rng = np.random.default_rng(4)
    dt, shape, trailing = np.float64, (5, 4, 3), (2, 3)
    ax = [nonuniform(rng, n, dt) for n in shape]
    data = rng.uniform(-1, 1, shape + trailing)
    it = make(pkg, *ax, data)
    q = [inside(rng, k, 24, dt).reshape(2, 3, 4) for k in ax]
    ref = tr.trilinear_ref(*ax, data, *q)[2].reshape((2, 3, 4) + trailing)
    same_bits(it.interp_array(*q), ref, "rank-3 queries")
    buf = np.full((4, 2, 3, 4) + trailing, SENTINEL)[1]              # contiguous; and a strided view below
    it.interp_array_into(*q, buf)
    same_bits(buf, ref, "interp_array_into")
    wide = np.full((2, 3, 4, 2, 6), SENTINEL)
    it.interp_array_into(*q, wide[..., ::2])
    same_bits(np.ascontiguousarray(wide[..., ::2]), ref, "a non-contiguous host buffer")
    assert np.all(wide[..., 1::2] == SENTINEL)


# ---- the slab property ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("lanes", [3, 4])
def test_slab_property_on_the_device(pkg, dt, lanes):
    """at qz = z[k], k < nz - 1, the row is the project's own Bilinear row on data[:, :, k], bit for bit"""
    rng = np.random.default_rng(5)
    shape = (5, 4, 3)
    x, y, z = (nonuniform(rng, n, dt) for n in shape)
    data = rng.uniform(-1, 1, shape + (lanes,)).astype(dt)
    it = make(pkg, x, y, z, data)
    qx, qy = inside(rng, x, 300, dt), inside(rng, y, 300, dt)
    for k in range(shape[2] - 1):
        slab = pkg.Interp2DBuilder.new(np.ascontiguousarray(data[:, :, k])).x(x).y(y).build()
        same_bits(it.interp_array(qx, qy, np.full(300, z[k], dt)), slab.interp_array(qx, qy), f"slab {k}")


# ---- every kernel instance ---------------------------------------------------------------------------------------------------
def run_instance(pkg, monkeypatch, capfd, dt, vec, stage, check):
    """one instance on an alignable shape (5 x 4 x 3 x 4), vec=1 and stage=0 forced by the knobs"""
    import torch
    rng = np.random.default_rng(6)
    shape, lanes, Q = (5, 4, 3), 4, 1031
    ax = [nonuniform(rng, n, dt) for n in shape]
    data = rng.uniform(-1, 1, shape + (lanes,)).astype(dt)
    q = [inside(rng, k, Q, dt) for k in ax]
    ref = tr.trilinear_ref(*ax, data, *q)[2]
    it = make(pkg, *ax, data)
    monkeypatch.setenv("NDI_TRILINEAR_VEC", "1" if vec == 1 else "-1")
    monkeypatch.setenv("NDI_TRILINEAR_STAGE", str(stage))
    what = f"{np.dtype(dt)} vec={vec} stage={stage} check={check}"
    qd = [dev(a) for a in q]
    with traced(capfd) as t:
        if check:
            got = it.interp_array(*qd)                       # its own output: the kernel tests the queries
        else:
            got = torch.full((Q, lanes), SENTINEL, dtype=qd[0].dtype, device="cuda:0")
            it.interp_array_into(*qd, got)                   # a caller's buffer: the pre-pass
    expect(t.plans, what, vec=vec, stage=stage, check=check)
    same_bits(got.cpu().numpy(), ref, what)
    monkeypatch.delenv("NDI_TRILINEAR_VEC")
    monkeypatch.delenv("NDI_TRILINEAR_STAGE")


@pytest.mark.parametrize("dt", DTYPES)
def test_every_instance_by_its_plan_line(pkg, monkeypatch, capfd, dt):
    for vec in (1, WIDE[dt]):
        for stage in (0, 1):
            for check in (0, 1):
                run_instance(pkg, monkeypatch, capfd, dt, vec, stage, check)


@pytest.mark.parametrize("dt", DTYPES)
def test_scalar_form_without_the_knob(pkg, capfd, dt):
    """vec=1 is the plan of lanes 3, of out_row_stride = lanes + 1 and of an output offset by one element"""
    import torch
    rng = np.random.default_rng(8)
    shape, Q = (5, 4, 3), 515
    ax = [nonuniform(rng, n, dt) for n in shape]
    q = [inside(rng, k, Q, dt) for k in ax]
    qd = [dev(a) for a in q]
    for lanes, what in ((3, "lanes 3"), (4, "stride"), (4, "offset")):
        data = rng.uniform(-1, 1, shape + (lanes,)).astype(dt)
        ref = tr.trilinear_ref(*ax, data, *q)[2]
        it = make(pkg, *ax, data)
        flat = torch.full((Q * (lanes + 1) + 8,), SENTINEL, dtype=qd[0].dtype, device="cuda:0")
        if what == "lanes 3":
            out, stride = flat[:Q * lanes].view(Q, lanes), lanes
        elif what == "stride":
            out, stride = flat[:Q * (lanes + 1)].view(Q, lanes + 1), lanes + 1
        else:
            out, stride = flat[1:1 + Q * lanes].view(Q, lanes), lanes
            assert out.data_ptr() % 16 != 0
        with traced(capfd) as t:
            st, _ = raw_call(pkg, it, *qd, Q, out, stride, q_dev=True, out_dev=True)
            torch.cuda.synchronize()
        assert st == pkg._capi.OK, pkg._capi.last_error()
        expect(t.plans, what, vec=1, stage=1, check=0)
        got = out.cpu().numpy()
        same_bits(np.ascontiguousarray(got[:, :lanes]), ref, what)
        if what == "stride":
            assert np.all(got[:, lanes] == SENTINEL), "the padding of a row is not written"
        if what == "offset":
            assert flat[0].item() == SENTINEL and flat[1 + Q * lanes].item() == SENTINEL
        # the same call on a vector-aligned buffer takes the wide form where lanes allow it
        with traced(capfd) as t:
            it.interp_array_into(*qd, torch.empty((Q, lanes), dtype=qd[0].dtype, device="cuda:0"))
        expect(t.plans, what + ": aligned", vec=WIDE[dt] if lanes % WIDE[dt] == 0 else 1)


@pytest.mark.parametrize("long_axis", [0, 1, 2])
def test_a_long_axis_is_bisected_in_global_memory(pkg, capfd, long_axis):
    """40 001 f32 knots do not fit the staging limit: stage=0 without the knob, on x, on y and on z in turn"""
    dt = np.float32
    rng = np.random.default_rng(9)
    shape = [2, 2, 2]
    shape[long_axis] = 40_001
    ax = [nonuniform(rng, n, dt) for n in shape]
    data = rng.uniform(-1, 1, tuple(shape) + (2,)).astype(dt)
    q = [inside(rng, k, 257, dt) for k in ax]
    for a in range(3):
        q[a][:4] = [ax[a][0], ax[a][-1], ax[a][1], ax[a][-2]]
    ref = tr.trilinear_ref(*ax, data, *q)[2]
    it = make(pkg, *ax, data)
    with traced(capfd) as t:
        got = it.interp_array(*q)
    expect(t.plans, f"long axis {long_axis}", vec=1, stage=0, check=1)
    same_bits(got, ref, f"long axis {long_axis}")
    with traced(capfd) as t:
        got = it.interp_array(*[dev(a) for a in q])
    expect(t.plans, f"long axis {long_axis}, device", vec=1, stage=0, check=1)
    same_bits(got.cpu().numpy(), ref, f"long axis {long_axis}, device")


@pytest.mark.parametrize("dt", DTYPES)
def test_a_batch_larger_than_one_pass_of_the_grid(pkg, capfd, dt):
    """70 001 queries on scalar data; the x axis fills more than half a CU's LDS, so the resident grid is one workgroup per
    CU and every thread walks the batch more than once"""
    rng = np.random.default_rng(10)
    shape = (100_000 // np.dtype(dt).itemsize, 2, 2)
    ax = [nonuniform(rng, n, dt) for n in shape]
    data = rng.uniform(-1, 1, shape).astype(dt)
    q = [inside(rng, k, 70_001, dt) for k in ax]
    ref = tr.trilinear_ref(*ax, data, *q)[2].reshape(-1)
    it = make(pkg, *ax, data)
    with traced(capfd) as t:
        got = it.interp_array(*[dev(a) for a in q])
    expect(t.plans, "70 001 queries", vec=1, stage=1, check=1)
    assert t.plans[0]["grid"] * BLOCK < 70_001, t.plans
    same_bits(got.cpu().numpy(), ref, "70 001 queries")


# ---- errors and buffer state -------------------------------------------------------------------------------------------------------
def error_fixture(pkg, dt, extrapolate):
    rng = np.random.default_rng(13)
    shape, lanes, Q = (5, 4, 3), 4, 300
    ax = [nonuniform(rng, n, dt) for n in shape]
    data = rng.uniform(-1, 1, shape + (lanes,)).astype(dt)
    q = [inside(rng, k, Q, dt) for k in ax]
    return ax, data, q, make(pkg, *ax, data, extrapolate)


def plant(q, changes):
    q = [a.copy() for a in q]
    for axis, index, value in changes:
        q[axis][index] = value
    return q


def failing_call(pkg, it, ax, data, q, on_device, extrapolate, **kw):
    """interp_array_into on a sentinel buffer; returns (the exception, the buffer as numpy, the reference)"""
    import torch
    Q, lanes = q[0].size, data.shape[3]
    fail, axis, ref = tr.trilinear_ref(*ax, data, *q, extrapolate)
    if on_device:
        buf = torch.full((Q, lanes), SENTINEL, dtype=dev(q[0]).dtype, device="cuda:0")
        args = [dev(a) for a in q]
    else:
        buf = np.full((Q, lanes), SENTINEL, data.dtype)
        args = q
    err = None
    try:
        it.interp_array_into(*args, buf, **kw)
    except (pkg.InterpolateError.OutOfBounds, pkg.Panic) as e:
        err = e
    return err, (buf.cpu().numpy() if on_device else buf), (fail, axis, ref)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("on_device", [False, True])
def test_errors_and_buffer_state(pkg, dt, on_device):
    from ndarray_interp_amd.errors import _rust_float
    ax, data, q, it = error_fixture(pkg, dt, False)
    above = [np.nextafter(k[-1], dt(np.inf)) for k in ax]
    below = [np.nextafter(k[0], dt(-np.inf)) for k in ax]
    cases = [
        ("x", [(0, 100, above[0])], (100, 0)),
        ("y", [(1, 57, below[1])], (57, 1)),
        ("z", [(2, 200, above[2])], (200, 2)),
        ("the first query", [(2, 0, below[2])], (0, 2)),
        ("the last query", [(1, 299, above[1])], (299, 1)),
        ("x and z in one query: x is reported", [(0, 80, below[0]), (2, 80, above[2])], (80, 0)),
        ("y and z in one query: y is reported", [(1, 81, below[1]), (2, 81, above[2])], (81, 1)),
        ("z at a lower index than x", [(2, 50, below[2]), (0, 120, above[0])], (50, 2)),
        ("NaN fails the range test", [(1, 30, np.nan), (0, 31, above[0])], (30, 1)),
        ("+inf", [(0, 10, np.inf)], (10, 0)),
        ("-inf", [(2, 11, -np.inf)], (11, 2)),
    ]
    for what, changes, (index, axis) in cases:
        qq = plant(q, changes)
        for mode in ({}, {"fresh": True}, {"rows_after_error_unspecified": True}):
            w = f"{what} {mode}"
            err, buf, (fail, faxis, ref) = failing_call(pkg, it, ax, data, qq, on_device, False, **mode)
            assert (fail, faxis) == (index, axis), w                                     # the reference agrees with the case
            assert isinstance(err, pkg.InterpolateError.OutOfBounds), (w, err)
            value = qq[axis][index]
            assert (err.index, err.axis) == (index, axis), (w, err.index, err.axis)
            assert err.value == float(value) or (np.isnan(value) and np.isnan(err.value)), (w, err.value)
            assert str(err) == f"{'xyz'[axis]} = {_rust_float(float(value))} is not in range", (w, str(err))
            same_bits(buf[:index], ref[:index], w + ": the rows before the failing query")
            if not mode:
                assert np.all(buf[index:] == SENTINEL), w + ": the failing row and all later rows are untouched"


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("on_device", [False, True])
def test_nan_and_infinities_while_extrapolating(pkg, dt, on_device):
    ax, data, q, it = error_fixture(pkg, dt, True)
    for axis, index in ((0, 40), (1, 41), (2, 42)):
        qq = plant(q, [(axis, index, np.nan), ((axis + 1) % 3, index + 9, np.nan)])
        for mode in ({}, {"fresh": True}):
            err, buf, (fail, faxis, ref) = failing_call(pkg, it, ax, data, qq, on_device, True, **mode)
            assert (fail, faxis) == (index, axis)
            assert isinstance(err, pkg.Panic) and err.index == index, (axis, mode, err)
            assert "failed to convert NaN to usize" in str(err)
            same_bits(buf[:index], ref[:index], f"NaN on axis {axis} {mode}: rows before")
            if not mode:
                assert np.all(buf[index:] == SENTINEL)
    qq = plant(q, [(0, 5, np.inf), (1, 6, -np.inf), (2, 7, np.inf), (0, 8, -np.inf), (2, 8, -np.inf)])
    err, buf, (fail, _, ref) = failing_call(pkg, it, ax, data, qq, on_device, True)
    assert err is None and fail is None                                                   # an infinite query extrapolates
    same_bits(buf, ref, "infinite queries while extrapolating")


@pytest.mark.parametrize("dt", DTYPES)
def test_a_host_batch_in_two_staging_chunks(pkg, monkeypatch, capfd, dt):
    ax, data, q, it = error_fixture(pkg, dt, False)
    lanes, Q = data.shape[3], q[0].size
    monkeypatch.setenv("NDI_TRILINEAR_CHUNK", str(160 * lanes * np.dtype(dt).itemsize))   # 160 rows per chunk: 160 + 140
    ref = tr.trilinear_ref(*ax, data, *q)[2]
    with traced(capfd) as t:
        got = it.interp_array(*q)
    expect(t.plans, "two chunks", n=2, check=1)
    same_bits(got, ref, "two chunks")
    with traced(capfd) as t:                                                              # host queries, a device buffer
        got = dev(np.full((Q, lanes), SENTINEL, dt))
        it.interp_array_into(*q, got)
    expect(t.plans, "two chunks, device buffer", n=2, check=0)
    same_bits(got.cpu().numpy(), ref, "two chunks, device buffer")
    # a failure in the second chunk: index and value are the batch's, the rows before it cross the chunk boundary
    bad = np.nextafter(ax[2][-1], dt(np.inf))
    qq = plant(q, [(2, 200, bad), (0, 250, np.nan)])
    for on_device in (False, True):
        with traced(capfd) as t:
            err, buf, (_, _, ref2) = failing_call(pkg, it, ax, data, qq, on_device, False)
        assert len(t.plans) == (1 if on_device else 2)          # (device queries and a device buffer are one chunk)
        assert isinstance(err, pkg.InterpolateError.OutOfBounds) and (err.index, err.axis, err.value) == (200, 2, float(bad))
        same_bits(buf[:200], ref2[:200], "rows before the failure, across the chunk boundary")
        assert np.all(buf[200:] == SENTINEL)
    # a failure in the first chunk ends the call there
    with traced(capfd) as t:
        err, buf, _ = failing_call(pkg, it, ax, data, plant(q, [(1, 3, np.nan)]), False, False)
    assert len(t.plans) == 1 and (err.index, err.axis) == (3, 1) and np.all(buf[3:] == SENTINEL)


def test_refusals_on_a_handle(pkg):
    cap = pkg._capi
    ax, data, q, it = error_fixture(pkg, np.float64, False)
    out = np.full((300, 4), SENTINEL)
    assert raw_call(pkg, it, *q, 300, out, 3)[0] == cap.BAD_ARG and "out_row_stride" in cap.last_error()
    for args in ((None, q[1], q[2], 300, out), (q[0], None, q[2], 300, out), (q[0], q[1], None, 300, out), (q[0], q[1], q[2], 300, None)):
        assert raw_call(pkg, it, *args, 4)[0] == cap.BAD_ARG and "null" in cap.last_error()
    assert raw_call(pkg, it, None, None, None, 0, None, 4)[0] == cap.OK                   # nq == 0 touches nothing
    assert raw_call(pkg, it, *q, 300, out, 4, flags=8)[0] == cap.BAD_ARG
    assert np.all(out == SENTINEL)
    assert raw_call(pkg, it, *q, 300, out, 4)[0] == cap.OK
    same_bits(out, tr.trilinear_ref(*ax, data, *q)[2], "after the refusals")


# ---- hostile data ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_hostile_data(pkg, dt):
    """3 x 3 x 3 with 4 lanes: +-0, +-inf and NaN entries, differences that overflow, subnormal and huge axis spacings"""
    rng = np.random.default_rng(14)
    fi = np.finfo(dt)
    big, tiny = dt(fi.max), dt(fi.smallest_subnormal)
    huge = dt(1e300 if dt == np.float64 else 1e30)
    data = rng.uniform(-1, 1, (3, 3, 3, 4)).astype(dt)
    data[0, 0, 0] = [0.0, -0.0, np.inf, -np.inf]
    data[1, 1, 1] = [np.nan, big, -big, tiny]
    data[2, 2, 2] = [-big, big, -0.0, -tiny]
    data[0, 1, 2] = [big, -big, big, -big]           # against neighbours of the other sign: the difference overflows
    data[1, 1, 2] = [-big, big, 0.0, -0.0]
    data[2, 0, 1] = 0.0
    axes = {
        "plain": [nonuniform(rng, 3, dt) for _ in range(3)],
        "subnormal spacing": [np.array([0, 3, 7], dt) * tiny, np.array([-2, 0, 5], dt) * tiny, nonuniform(rng, 3, dt)],
        "huge spacing": [np.array([-1, 0, 1], dt) * huge, nonuniform(rng, 3, dt), np.array([0, 1, 3], dt) * huge],
        "mixed": [np.array([0, 1, 2], dt) * tiny, np.array([-1, 0, 2], dt) * huge, np.array([1, 1 + 2 * fi.eps, 2], dt)],
    }
    for name, ax in axes.items():
        km = [tr.knots_and_midpoints(k) for k in ax]
        q = [np.ascontiguousarray(a.ravel()) for a in np.meshgrid(*km, indexing="ij")]
        for extrapolate in (False, True):
            if extrapolate:
                span = [k[-1] - k[0] for k in ax]
                q = [np.concatenate([a, np.array([k[0] - s, k[-1] + s / 2, k[0] - s / 4, k[-1]], dt)]) for a, k, s in zip(q, ax, span)]
            fail, _, ref = tr.trilinear_ref(*ax, data, *q, extrapolate)
            assert fail is None, name
            it = make(pkg, *ax, data, extrapolate)
            same_bits(it.interp_array(*q), ref.reshape(-1, 4), f"{name} extrapolate={extrapolate}: host")
            same_bits(it.interp_array(*[dev(a) for a in q]).cpu().numpy(), ref.reshape(-1, 4), f"{name} extrapolate={extrapolate}: device")
            got = dev(np.full((q[0].size, 4), SENTINEL, dt))
            it.interp_array_into(*[dev(a) for a in q], got)
            same_bits(got.cpu().numpy(), ref.reshape(-1, 4), f"{name} extrapolate={extrapolate}: device buffer")


# ---- other calls -------------------------------------------------------------------------------------------------------------------
def test_clone_and_replicate(pkg):
    ax, data, q, it = error_fixture(pkg, np.float32, False)
    ref = it.interp_array(*q)
    twin = it.strategy.clone(0)
    got = np.empty_like(ref)
    twin.interp_array_into(None, *q, got)
    assert np.array_equal(got, ref)
    reps = it.replicate([0, 0])
    assert len(reps) == 2 and all(np.array_equal(r.interp_array(*q), ref) for r in reps)
    it.strategy.release()                                          # the replicas own their copies
    assert np.array_equal(reps[1].interp_array(*[dev(a) for a in q]).cpu().numpy(), ref)
    twin.release()
    twin.release()


@pytest.mark.parametrize("dt", DTYPES)
def test_scalar_calls_agree_with_the_batch(pkg, dt):
    rng = np.random.default_rng(15)
    shape = (5, 4, 3)
    ax = [nonuniform(rng, n, dt) for n in shape]
    q = [inside(rng, k, 9, dt) for k in ax]
    scalar = make(pkg, *ax, rng.uniform(-1, 1, shape).astype(dt))
    lanes = make(pkg, *ax, rng.uniform(-1, 1, shape + (2, 3)).astype(dt))
    batch_s, batch_l = scalar.interp_array(*q), lanes.interp_array(*q)
    assert batch_s.shape == (9,) and batch_l.shape == (9, 2, 3)
    for i in range(9):
        p = [a[i] for a in q]
        v = scalar.interp_scalar(*p)
        assert v.dtype == dt and tr.bits(np.array([v]))[0] == tr.bits(batch_s[i:i + 1])[0]
        same_bits(scalar.interp(*p), batch_s[i], "interp on scalar data")
        same_bits(lanes.interp(*p), batch_l[i], "interp")
    with pytest.raises(TypeError):
        lanes.interp_scalar(*[a[0] for a in q])
    with pytest.raises(pkg.InterpolateError.OutOfBounds, match="z = .* is not in range"):
        scalar.interp_scalar(q[0][0], q[1][0], ax[2][-1] + 1)
    assert scalar.get_index_left_of(ax[0][2], ax[1][-1], np.nextafter(ax[2][1], dt(-np.inf))) == (2, 2, 0)


def test_a_callers_stream_is_honoured(pkg):
    """work enqueued on the caller's stream before the call is seen by it: the queries are written by a copy on that stream"""
    import torch
    ax, data, q, it = error_fixture(pkg, np.float64, False)
    ref = tr.trilinear_ref(*ax, data, *q)[2]
    s = torch.cuda.Stream()
    pinned = [torch.as_tensor(a).pin_memory() for a in q]
    with torch.cuda.stream(s):
        spin = torch.zeros(1 << 24, device="cuda:0")
        for _ in range(20):
            spin = spin * 1.0001 + 1.0                       # keeps the stream busy ahead of the copies
        qd = [torch.empty(300, dtype=torch.float64, device="cuda:0") for _ in range(3)]
        for d, p in zip(qd, pinned):
            d.copy_(p, non_blocking=True)
        got = it.interp_array(*qd)
        out = torch.full((300, 4), SENTINEL, dtype=torch.float64, device="cuda:0")
        st, _ = raw_call(pkg, it, *qd, 300, out, 4, q_dev=True, out_dev=True, stream=s.cuda_stream)
        assert st == pkg._capi.OK
    s.synchronize()
    same_bits(got.cpu().numpy(), ref, "on a caller's stream")
    same_bits(out.cpu().numpy(), ref, "on a caller's stream, the raw call")


def test_two_host_threads_on_one_handle(pkg):
    ax, data, q, it = error_fixture(pkg, np.float32, False)
    ref = tr.trilinear_ref(*ax, data, *q)[2]
    results, errors = {}, []

    def work(tid):
        try:
            for r in range(5):
                qq = [np.roll(a, tid + r) for a in q]
                results[(tid, r)] = (it.interp_array(*qq), np.roll(ref, tid + r, axis=0))
        except BaseException as e:  # noqa: BLE001
            errors.append(e)
    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert len(results) == 10
    for key, (got, want) in results.items():
        same_bits(got, want, f"thread {key}")


# ---- the bounds-checked library ------------------------------------------------------------------------------------------------------
def test_checked_cases(pkg, monkeypatch, capfd):
    """what runs again under the bounds-checked library (below): one case per kernel instance"""
    for dt in DTYPES:
        for vec in (1, WIDE[dt]):
            for stage in (0, 1):
                for check in (0, 1):
                    run_instance(pkg, monkeypatch, capfd, dt, vec, stage, check)


def test_the_bounds_checked_library_runs_clean():
    """NDI_CHK on the row, the vector of the row and the three cell indices: a violation fails the call"""
    from test_gpu_checked_build import _ensure_debug_library
    _ensure_debug_library()
    env = dict(os.environ, NDI_LIB="libndinterp_hip_dbg.so")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_trilinear.py"), "-m", "gpu", "-x",
                        "-q", "-k", "test_checked_cases"],
                       capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "failed" not in r.stdout.splitlines()[-1]
