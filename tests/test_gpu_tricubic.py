"""GPU: Interp3D / Tricubic (include/ndinterp3d_cubic.h) against tests/tricubic_ref.py, bit for bit (integer views, NaN
equal to NaN): the seven node tables and the rows over dtypes, grids, trailing shapes, end sets and memory spaces; every
kernel instance by its plan line; a second trip of the grid-stride loop; hostile queries and data; errors and buffer state;
smoothness against Trilinear; clone, replicate, streams, threads; the example and the bounds-checked library."""
import ctypes as C
import os
import re
import subprocess
import sys
import threading

import numpy as np
import pytest

import tricubic_ref as tc
from conftest import ROOT

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
GRIDS = [(3, 3, 3), (4, 4, 4), (3, 5, 4), (9, 6, 12), (33, 17, 9)]
SENTINEL = -77.25
PLAN = re.compile(r"\[ndi plan\] tricubic vec=(\d+) stage=(\d+) check=(\d+) grid=(\d+)")
WIDE = {np.float32: 4, np.float64: 2}
BLOCK = 256
ENDS = {"default": tc.DEFAULT_BC, "mixed": tc.MIXED_BC}


class traced:
    """the tricubic plan lines (as dicts) of the calls inside"""

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
    a, b = tc.bits(got.reshape(ref.shape)), tc.bits(ref)
    if not np.array_equal(a, b):
        bad = np.argwhere(a != b)
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {bad.shape[0]} of {a.size} elements differ; first at {i}: got {got.reshape(ref.shape)[i]!r}, "
                             f"reference {ref[i]!r}")


def nonuniform(rng, n, dt, lo=0.0):
    return (lo + np.cumsum(rng.uniform(0.5, 1.5, n))).astype(dt)


def dev(a):
    import torch
    return torch.as_tensor(a, device="cuda:0")


def strategy(pkg, bc, extrapolate=False):
    """a Tricubic builder with the six (kind, value) ends of tricubic_ref"""
    S = pkg.SingleBoundary
    one = lambda e: S(int(e[0]), float(e[1]))   # noqa: E731
    s = pkg.Tricubic.new().extrapolate(extrapolate)
    return s.boundary_x(pkg.RowBoundary.Mixed(one(bc[0]), one(bc[1]))).boundary_y(pkg.RowBoundary.Mixed(one(bc[2]), one(bc[3]))) \
        .boundary_z(pkg.RowBoundary.Mixed(one(bc[4]), one(bc[5])))


def make(pkg, x, y, z, data, bc=tc.DEFAULT_BC, extrapolate=False):
    return pkg.Interp3D.builder(data).x(x).y(y).z(z).strategy(strategy(pkg, bc, extrapolate)).build()


def flat4(data):
    return np.ascontiguousarray(data).reshape(data.shape[:3] + (-1,))


def reference(ax, data, q, bc=tc.DEFAULT_BC, extrapolate=False, tabs=None):
    """(fail, axis, rows): the lowest failing query and its axis (None: none), and every row by the rule (rows at and after
    `fail` are not the library's business)"""
    f = flat4(data)
    tabs = tc.tables(*ax, f, bc) if tabs is None else tabs
    fail, axis = tc.first_failure(*ax, *q, extrapolate)
    return fail, axis, tc.evaluate(*ax, f, tabs, *q)


def inside(rng, k, n, dt):
    return np.clip(rng.uniform(k[0], k[-1], n).astype(dt), k[0], k[-1])


def hostile_queries(ax, dt, extrapolate):
    """every knot, the last knot, nextafter on either side of every knot (inside the range), +-0 where the axis holds 0, and
    with `extrapolate` points outside; per axis, cycled to one length"""
    per = []
    for k in ax:
        lo, hi = np.nextafter(k, dt(-np.inf)), np.nextafter(k, dt(np.inf))
        p = np.concatenate([k, [k[-1]], lo[1:], hi[:-1], ((k[:-1].astype(np.float64) + k[1:]) / 2).astype(dt)])
        if k[0] <= 0 <= k[-1]:
            p = np.concatenate([p, np.array([0.0, -0.0], dt)])
        if extrapolate:
            s = k[-1] - k[0]
            p = np.concatenate([p, np.array([k[0] - 1e3 * s, k[-1] + 1e3 * s, k[0] - s / 3, k[-1] + s / 7, lo[0], hi[-1]], dt)])
        per.append(p.astype(dt))
    m = max(len(p) for p in per) + 1
    return [np.resize(p, m) for p in per]


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


# ---- tables ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", GRIDS)
def test_tables(pkg, dt, shape):
    rng = np.random.default_rng(31)
    ax = [nonuniform(rng, n, dt, lo) for n, lo in zip(shape, (-3.0, 0.0, 10.0))]
    for trailing in [(), (1,), (3,), (4,), (2, 4)]:
        data = rng.uniform(-1, 1, shape + trailing).astype(dt)
        for ends, bc in ENDS.items():
            ref = tc.tables(*ax, flat4(data), bc)
            what = f"{np.dtype(dt)} {shape} {trailing} {ends}"
            got = make(pkg, *ax, data, bc).strategy.tables()
            assert len(got) == 7 and all(g.shape == data.shape for g in got), what
            for name, g, r in zip(("fx", "fy", "fz", "fxy", "fxz", "fyz", "fxyz"), got, ref):
                same_bits(g, r.reshape(data.shape), f"{what}: {name}, host inputs")
            on_dev = make(pkg, *[dev(k) for k in ax], dev(data), bc).strategy.tables(on_device=True)
            for name, g, r in zip(("fx", "fy", "fz", "fxy", "fxz", "fyz", "fxyz"), on_dev, ref):
                assert g.is_cuda
                same_bits(g.cpu().numpy(), r.reshape(data.shape), f"{what}: {name}, device inputs")


def test_tables_with_null_entries_and_on_a_trilinear_handle(pkg):
    cap, lib = pkg._capi, pkg._capi.lib()
    rng = np.random.default_rng(32)
    shape = (4, 3, 5)
    ax = [nonuniform(rng, n, np.float64) for n in shape]
    data = rng.uniform(-1, 1, shape + (2,))
    it = make(pkg, *ax, data)
    ref = tc.tables(*ax, data)
    only = np.full(data.shape, SENTINEL)
    ptrs = (C.c_void_p * 7)()
    ptrs[5] = only.ctypes.data                               # fyz alone
    assert lib.ndi_interp3d_tables(it.strategy._h, ptrs, cap.MEM_HOST) == cap.OK
    same_bits(only, ref[5], "fyz alone")
    assert lib.ndi_interp3d_tables(it.strategy._h, ptrs, 7) == cap.BAD_ARG and "memspace" in cap.last_error()
    assert lib.ndi_interp3d_tables(it.strategy._h, None, cap.MEM_HOST) == cap.BAD_ARG
    lin = pkg.Interp3D.builder(data).x(ax[0]).y(ax[1]).z(ax[2]).strategy(pkg.Trilinear.new()).build()
    assert lib.ndi_interp3d_tables(lin.strategy._h, ptrs, cap.MEM_HOST) == cap.BAD_ARG
    assert "takes a Tricubic handle" in cap.last_error()


# ---- rows --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", GRIDS)
def test_rows(pkg, dt, shape):
    import torch
    rng = np.random.default_rng(33)
    ax = [nonuniform(rng, n, dt, lo) for n, lo in zip(shape, (-3.0, 0.0, 10.0))]
    ax[0] = ax[0] - ax[0][1]                                     # 0 is a knot of x: the queries +0 and -0 lie on it
    assert ax[0][1] == 0 and np.all(np.diff(ax[0]) > 0)
    for trailing in [(), (3,), (4,), (2, 3), (260,)]:
        data = rng.uniform(-1, 1, shape + trailing).astype(dt)
        lanes = int(np.prod(trailing, dtype=np.int64))
        for ends, bc in ENDS.items():
            tabs = tc.tables(*ax, flat4(data), bc)
            for extrapolate in (False, True):
                what = f"{np.dtype(dt)} {shape} {trailing} {ends} extrapolate={extrapolate}"
                it = make(pkg, *ax, data, bc, extrapolate)
                q = [np.concatenate([h, inside(rng, k, 67, dt)]) for h, k in zip(hostile_queries(ax, dt, extrapolate), ax)]
                fail, _, ref = reference(ax, data, q, bc, extrapolate, tabs)
                assert fail is None, what
                Q = q[0].size
                got = it.interp_array(*q)
                assert isinstance(got, np.ndarray) and got.shape == (Q,) + trailing, what
                same_bits(got, ref, what + ": host arrays")
                qd = [dev(a) for a in q]
                got = it.interp_array(*qd)
                assert got.is_cuda and tuple(got.shape) == (Q,) + trailing, what
                same_bits(got.cpu().numpy(), ref, what + ": device tensors")
                buf = np.full((Q,) + trailing, SENTINEL, dt)                     # device queries, a host buffer
                it.interp_array_into(*qd, buf)
                same_bits(buf, ref, what + ": device queries, host buffer")
                out = torch.full((Q, lanes + 4), SENTINEL, dtype=qd[0].dtype, device="cuda:0")     # a strided output
                st, _ = raw_call(pkg, it, *qd, Q, out, lanes + 4, q_dev=True, out_dev=True)
                torch.cuda.synchronize()
                assert st == pkg._capi.OK, pkg._capi.last_error()
                o = out.cpu().numpy()
                same_bits(np.ascontiguousarray(o[:, :lanes]), ref, what + ": a strided output")
                assert np.all(o[:, lanes:] == SENTINEL), what + ": the padding of a row is not written"


# ---- every kernel instance ---------------------------------------------------------------------------------------------------
def run_instance(pkg, monkeypatch, capfd, dt, vec, stage, check):
    """one instance on an alignable shape (5 x 4 x 3 x 4), vec=1 and stage=0 forced by the knobs"""
    import torch
    rng = np.random.default_rng(36)
    shape, lanes, Q = (5, 4, 3), 4, 1031
    ax = [nonuniform(rng, n, dt) for n in shape]
    data = rng.uniform(-1, 1, shape + (lanes,)).astype(dt)
    q = [inside(rng, k, Q, dt) for k in ax]
    ref = reference(ax, data, q, tc.MIXED_BC)[2]
    it = make(pkg, *ax, data, tc.MIXED_BC)
    monkeypatch.setenv("NDI_TRICUBIC_VEC", "1" if vec == 1 else "-1")
    monkeypatch.setenv("NDI_TRICUBIC_STAGE", str(stage))
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
    monkeypatch.delenv("NDI_TRICUBIC_VEC")
    monkeypatch.delenv("NDI_TRICUBIC_STAGE")


@pytest.mark.parametrize("dt", DTYPES)
def test_every_instance_by_its_plan_line(pkg, monkeypatch, capfd, dt):
    for vec in (1, WIDE[dt]):
        for stage in (0, 1):
            for check in (0, 1):
                run_instance(pkg, monkeypatch, capfd, dt, vec, stage, check)


@pytest.mark.parametrize("dt", DTYPES)
def test_scalar_form_without_the_knob(pkg, capfd, dt):
    """vec=1 is the plan of lanes 3 and of an output offset by one element"""
    import torch
    rng = np.random.default_rng(38)
    shape, Q = (5, 4, 3), 515
    ax = [nonuniform(rng, n, dt) for n in shape]
    q = [inside(rng, k, Q, dt) for k in ax]
    qd = [dev(a) for a in q]
    for lanes, what in ((3, "lanes 3"), (4, "offset")):
        data = rng.uniform(-1, 1, shape + (lanes,)).astype(dt)
        ref = reference(ax, data, q)[2]
        it = make(pkg, *ax, data)
        flat = torch.full((Q * lanes + 8,), SENTINEL, dtype=qd[0].dtype, device="cuda:0")
        off = 0 if what == "lanes 3" else 1
        out = flat[off:off + Q * lanes].view(Q, lanes)
        assert off == 0 or out.data_ptr() % 16 != 0
        with traced(capfd) as t:
            st, _ = raw_call(pkg, it, *qd, Q, out, lanes, q_dev=True, out_dev=True)
            torch.cuda.synchronize()
        assert st == pkg._capi.OK, pkg._capi.last_error()
        expect(t.plans, what, vec=1, stage=1, check=0)
        same_bits(out.cpu().numpy(), ref, what)
        assert flat[off + Q * lanes].item() == SENTINEL and (off == 0 or flat[0].item() == SENTINEL)


def test_a_long_axis_is_bisected_in_global_memory(pkg, capfd):
    """40 000 f32 knots on x do not fit the staging limit: stage=0 without the knob, on a small grid otherwise"""
    dt = np.float32
    rng = np.random.default_rng(39)
    shape = (40_000, 3, 3)
    ax = [nonuniform(rng, n, dt) for n in shape]
    data = rng.uniform(-1, 1, shape + (2,)).astype(dt)
    q = [inside(rng, k, 257, dt) for k in ax]
    for a in range(3):
        q[a][:4] = [ax[a][0], ax[a][-1], ax[a][1], ax[a][-2]]
    ref = reference(ax, data, q)[2]
    it = make(pkg, *ax, data)
    with traced(capfd) as t:
        got = it.interp_array(*q)
    expect(t.plans, "long x axis", vec=1, stage=0, check=1)
    same_bits(got, ref, "long x axis")
    with traced(capfd) as t:
        got = it.interp_array(*[dev(a) for a in q])
    expect(t.plans, "long x axis, device", vec=1, stage=0, check=1)
    same_bits(got.cpu().numpy(), ref, "long x axis, device")


def test_a_batch_larger_than_one_pass_of_the_grid(pkg, capfd):
    """10 000 queries x 260 f32 lanes: 650 000 vectors, more than one pass of the resident grid, so rows of a trip other than
    the first are checked, with the (row, vector) carry live (65 vectors per row)"""
    dt = np.float32
    rng = np.random.default_rng(40)
    shape, lanes, Q = (4, 3, 5), 260, 10_000
    ax = [nonuniform(rng, n, dt) for n in shape]
    data = rng.uniform(-1, 1, shape + (lanes,)).astype(dt)
    q = [inside(rng, k, Q, dt) for k in ax]
    ref = reference(ax, data, q)[2]
    it = make(pkg, *ax, data)
    with traced(capfd) as t:
        got = it.interp_array(*[dev(a) for a in q])
    expect(t.plans, "10 000 x 260", vec=4, stage=1, check=1)
    step = t.plans[0]["grid"] * BLOCK
    assert step < Q * lanes // 4, t.plans
    same_bits(got.cpu().numpy(), ref, "10 000 x 260")
    assert np.array_equal(tc.bits(got.cpu().numpy()[-1]), tc.bits(ref[-1]))      # the last row lies in a later trip


# ---- hostile data ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_hostile_data(pkg, dt):
    """a NaN and an infinity in one lane leave the other lanes' bits unchanged; huge and subnormal values"""
    rng = np.random.default_rng(44)
    fi = np.finfo(dt)
    shape = (4, 3, 5)
    ax = [nonuniform(rng, n, dt) for n in shape]
    clean = rng.uniform(-1, 1, shape + (4,)).astype(dt)
    q = hostile_queries(ax, dt, True)
    ref_clean = reference(ax, clean, q, tc.MIXED_BC, True)[2]
    data = clean.copy()
    data[1, 1, 2, 1] = np.nan
    data[2, 0, 3, 1] = np.inf
    data[:, :, :, 3] *= dt(fi.max / 4)                           # huge: differences overflow
    data[:, :, :, 2] *= dt(fi.smallest_subnormal * 64)           # subnormal values
    ref = reference(ax, data, q, tc.MIXED_BC, True)[2]
    assert np.isnan(ref[:, 1]).any()
    same_bits(ref[:, 0], ref_clean[:, 0], "the reference itself: lane 0 does not see lane 1")
    it = make(pkg, *ax, data, tc.MIXED_BC, True)
    for name, t, r in zip(("fx", "fy", "fz", "fxy", "fxz", "fyz", "fxyz"), it.strategy.tables(), tc.tables(*ax, data, tc.MIXED_BC)):
        same_bits(t, r, f"hostile data: {name}")
    got = it.interp_array(*q)
    same_bits(got, ref, "hostile data: host")
    same_bits(got[:, 0], ref_clean[:, 0], "a NaN and an infinity in lane 1 leave lane 0's bits unchanged")
    same_bits(it.interp_array(*[dev(a) for a in q]).cpu().numpy(), ref, "hostile data: device")


# ---- errors and buffer state -------------------------------------------------------------------------------------------------------
def error_fixture(pkg, dt, extrapolate):
    rng = np.random.default_rng(43)
    shape, lanes, Q = (5, 4, 3), 4, 300
    ax = [nonuniform(rng, n, dt) for n in shape]
    data = rng.uniform(-1, 1, shape + (lanes,)).astype(dt)
    q = [inside(rng, k, Q, dt) for k in ax]
    return ax, data, q, make(pkg, *ax, data, tc.DEFAULT_BC, extrapolate)


def plant(q, changes):
    q = [a.copy() for a in q]
    for axis, index, value in changes:
        q[axis][index] = value
    return q


def failing_call(pkg, it, ax, data, q, on_device, extrapolate, **kw):
    """interp_array_into on a sentinel buffer; returns (the exception, the buffer as numpy, the reference)"""
    import torch
    Q, lanes = q[0].size, data.shape[3]
    ref = reference(ax, data, q, tc.DEFAULT_BC, extrapolate)
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
    return err, (buf.cpu().numpy() if on_device else buf), ref


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
    ]
    for what, changes, (index, axis) in cases:
        qq = plant(q, changes)
        for mode in ({}, {"fresh": True}):
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
def test_nan_while_extrapolating(pkg, dt, on_device):
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


@pytest.mark.parametrize("dt", DTYPES)
def test_a_host_batch_in_two_staging_chunks(pkg, monkeypatch, capfd, dt):
    ax, data, q, it = error_fixture(pkg, dt, False)
    lanes = data.shape[3]
    monkeypatch.setenv("NDI_TRILINEAR_CHUNK", str(160 * lanes * np.dtype(dt).itemsize))   # 160 rows per chunk: 160 + 140
    ref = reference(ax, data, q)[2]
    with traced(capfd) as t:
        got = it.interp_array(*q)
    expect(t.plans, "two chunks", n=2, check=1)
    same_bits(got, ref, "two chunks")
    # a failure in the second chunk: index and value are the batch's, the rows before it cross the chunk boundary
    bad = np.nextafter(ax[2][-1], dt(np.inf))
    qq = plant(q, [(2, 200, bad), (0, 250, np.nan)])
    with traced(capfd) as t:
        err, buf, (_, _, ref2) = failing_call(pkg, it, ax, data, qq, False, False)
    assert len(t.plans) == 2
    assert isinstance(err, pkg.InterpolateError.OutOfBounds) and (err.index, err.axis, err.value) == (200, 2, float(bad))
    same_bits(buf[:200], ref2[:200], "rows before the failure, across the chunk boundary")
    assert np.all(buf[200:] == SENTINEL)


def test_refusals_on_a_handle_keep_their_order_and_text(pkg):
    cap = pkg._capi
    ax, data, q, it = error_fixture(pkg, np.float64, False)
    out = np.full((300, 4), SENTINEL)
    assert raw_call(pkg, it, *q, 300, out, 3)[0] == cap.BAD_ARG and "out_row_stride" in cap.last_error()
    assert raw_call(pkg, it, None, q[1], q[2], 300, out, 4)[0] == cap.BAD_ARG and "null" in cap.last_error()
    assert raw_call(pkg, it, None, None, None, 0, None, 4)[0] == cap.OK                   # nq == 0 touches nothing
    assert raw_call(pkg, it, *q, 300, out, 4, flags=8)[0] == cap.BAD_ARG
    opts = cap.EvalOpts()
    opts.path = cap.PATH_BUCKETED
    st = cap.lib().ndi_interp3d_eval(it.strategy._h, q[0].ctypes.data, q[1].ctypes.data, q[2].ctypes.data, 300, out.ctypes.data, 4,
                                     C.byref(opts), None)
    assert st == cap.BAD_ARG and "NDI_PATH_BUCKETED" in cap.last_error()
    assert np.all(out == SENTINEL)
    assert raw_call(pkg, it, *q, 300, out, 4)[0] == cap.OK
    same_bits(out, reference(ax, data, q)[2], "after the refusals")


# ---- smoothness ----------------------------------------------------------------------------------------------------------------
def test_the_first_derivative_is_continuous_across_a_grid_plane_and_trilinears_jumps(pkg):
    """One-sided difference quotients of the result on either side of an interior x-plane, step h = 1e-5 of a spacing of
    about 1: for a C2 interpolant the two quotients differ by h times the second derivative, 1e-3 at the most for data in
    [-1, 1] on spacings above 0.5 (|f''| stays below 100 there), plus rounding 2 eps |f| / h = 5e-11; Trilinear's slope
    changes by the difference of two cell slopes, of the order of 1."""
    rng = np.random.default_rng(46)
    dt, shape = np.float64, (6, 5, 7)
    ax = [nonuniform(rng, n, dt) for n in shape]
    data = rng.uniform(-1, 1, shape + (3,))
    cubic = make(pkg, *ax, data)
    linear = pkg.Interp3D.builder(data).x(ax[0]).y(ax[1]).z(ax[2]).strategy(pkg.Trilinear.new()).build()
    n, h = 200, 1e-5
    qy, qz = inside(rng, ax[1], n, dt), inside(rng, ax[2], n, dt)
    plane = np.full(n, ax[0][3])

    def jump(it):
        lo, mid, hi = (it.interp_array(plane + d, qy, qz) for d in (-h, 0.0, h))
        return np.abs((hi - mid) / h - (mid - lo) / h)
    jc, jl = jump(cubic), jump(linear)
    print(f"slope change across the plane: tricubic {jc.max():.3e}, trilinear median {np.median(jl):.3e}")
    assert jc.max() <= 2e-3
    assert np.median(jl) > 0.05 and np.median(jl) > 50 * jc.max()


# ---- other calls -------------------------------------------------------------------------------------------------------------------
def test_clone_and_replicate(pkg):
    ax, data, q, it = error_fixture(pkg, np.float32, False)
    ref = it.interp_array(*q)
    same_bits(ref, reference(ax, data, q)[2], "the original")
    twin = it.strategy.clone(0)
    got = np.empty_like(ref)
    twin.interp_array_into(None, *q, got)
    assert np.array_equal(got, ref)
    assert all(np.array_equal(a, b) for a, b in zip(twin.tables(), it.strategy.tables()))
    reps = it.replicate([0, 0])
    assert len(reps) == 2 and all(np.array_equal(r.interp_array(*q), ref) for r in reps)
    it.strategy.release()                                          # the replicas own their copies
    assert np.array_equal(reps[1].interp_array(*[dev(a) for a in q]).cpu().numpy(), ref)
    twin.release()
    twin.release()


def test_a_callers_stream_is_honoured(pkg):
    """work enqueued on the caller's stream before the call is seen by it: the queries are written by a copy on that stream"""
    import torch
    ax, data, q, it = error_fixture(pkg, np.float64, False)
    ref = reference(ax, data, q)[2]
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
    ref = reference(ax, data, q)[2]
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


# ---- cross-build runs ------------------------------------------------------------------------------------------------------------
def test_the_example_runs_to_completion(pkg, tmp_path):
    exe = tmp_path / "c_abi_tricubic"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "c_abi_tricubic.c"), "-L", os.path.join(ROOT, "ndarray-interp_amd"),
                        "-lndinterp_hip", "-Wl,-rpath," + os.path.join(ROOT, "ndarray-interp_amd"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    f = lambda x, y, z: (1 + x ** 3) * (2 - y + y * y) * (1 + z - z ** 3)   # noqa: E731
    pts = list(zip((0.0, 0.25, 1.0, 2.0, 1.75), (-1.0, -0.5, 0.25, 1.0, 0.0), (0.0, 0.5, 1.125, 2.0, 1.5)))
    got = [float(v) for v in run.stdout.split()]
    assert len(got) == 5 and all(abs(g - f(*p)) <= 1e-12 * (1 + abs(f(*p))) for g, p in zip(got, pts))


def test_checked_cases(pkg, monkeypatch, capfd):
    """what runs again under the bounds-checked library (below): one parity case per kernel instance, and the build's pack /
    unpack kernels through tables()"""
    for dt in DTYPES:
        for vec in (1, WIDE[dt]):
            for stage in (0, 1):
                for check in (0, 1):
                    run_instance(pkg, monkeypatch, capfd, dt, vec, stage, check)
    rng = np.random.default_rng(47)
    shape = (3, 5, 4)
    ax = [nonuniform(rng, n, np.float64) for n in shape]
    data = rng.uniform(-1, 1, shape + (3,))
    for t, r in zip(make(pkg, *ax, data, tc.MIXED_BC).strategy.tables(), tc.tables(*ax, data, tc.MIXED_BC)):
        same_bits(t, r, "tables under the bounds-checked library")


def test_the_bounds_checked_library_runs_clean():
    """NDI_CHK on the row, the vector of the row, the three cell indices and the pack kernel's source index: a violation
    fails the call"""
    from test_gpu_checked_build import _ensure_debug_library
    _ensure_debug_library()
    env = dict(os.environ, NDI_LIB="libndinterp_hip_dbg.so")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_tricubic.py"), "-m", "gpu", "-x",
                        "-q", "-k", "test_checked_cases"],
                       capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "failed" not in r.stdout.splitlines()[-1]
